// The plans of the persistent chains (chain_plan.h): pure host arithmetic, pinned by tests/test_chain_plan_cpu.py on the
// decisions recorded before this file existed (tests/golden/chain_plans.jsonl).
#include <algorithm>

#include "chain_plan.h"
#include "chain_shape.h"

namespace t2 {

using namespace chain;

namespace {

constexpr int kLdsBytes = 160 * 1024;
size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }
ChainPlan refuse(ChainRefusal r) { ChainPlan p{}; p.refusal = r; return p; }
// lays a finished plan out in the pass's exchange space; parts carved from the back get their offsets here
size_t space_of(const ChainShape& z, const ChainPlan& p) { return z.ws_bytes ? z.ws_bytes : p.total; }

// ---- forward exchange space (chain_fwd_ws_floats), every part sized for the largest tiling plan_chain_fwd can choose:
//   [status words | query partials | fragments of the attention chain ...... fragments of the decoder-LSTM chain | mel fragments | counters]
// The attention chain's parts are carved from the front, the decoder-LSTM chain's (decode loop: dec_h) from the back, so that
// each chain finds its own from its own shape; the mel fragments and the arrival counters are the decode loop's.
constexpr size_t kStatusBytes = 256;                                        // ChainStatus words (kernels.h)
constexpr size_t kXmBytes = 16 * 1024;                                      // mel fragments [2][8][1 KB]
constexpr size_t kCntBytes = (size_t)16 * CNT_STRIDE * sizeof(unsigned);    // counters 0-3 (h / ctx of each stream), 8 (dec_h), 9 (mel), 10-11 (prenets)
// fragment-ordered operands of a K-wide product: [parity][stream][k tile of 16][row tile of 32][1 KB]
size_t x_part_bytes(int NS, int B, int K) { return (size_t)2 * NS * (K / 16) * ((B + 31) / 32) * 1024; }
// query partials: one 32-row tile per 32 batch rows, one unit group per 8 hidden units
size_t q_part_bytes(int NS, int B, int H, int A) { return (size_t)NS * ((B + 31) / 32) * 32 * (H / 8) * A * sizeof(float); }
// query partials of a tiling: [stream][row group][unit group][32 RT rows][A]
size_t q_bytes_of(const ChainDesc& d, const Geo& g) { return (size_t)d.NS * g.NRG * g.NUG * 32 * d.RT * d.A * sizeof(float); }

// ---- backward exchange space (chain_bwd_ws_floats): the attention chain's parts from the front — dg fragments, h and ctx
// K-split partials, dq partials, boundary carries (all of them tagged), then (LSA) the bf16 Wd^T copies — and the decoder-LSTM
// chain's from the back — dg fragments, K-split partials.
struct AttParts { size_t x, pbh, pbc, dqx, carry, wdt; };
AttParts att_parts(int kind, int NS, int B, int H, int E, int A, int F, int Kc) {
    const size_t MT = (B + 31) / 32;
    AttParts p;
    p.x = (size_t)2 * NS * (4 * H / 16) * MT * 1024;
    p.pbh = (size_t)2 * NS * AKP * (H / PU) * MT * 32 * PU * sizeof(float);
    p.pbc = al256((size_t)2 * NS * AKP * B * E * sizeof(float));
    p.dqx = al256((size_t)NS * 2 * B * A * sizeof(float));
    // SMA: one carry per (parity, stream, item); LSA: halo rows of dloc and softmax-dot slots (rsK in chain_bwd_att_kernel)
    p.carry = al256(kind == CHAIN_LSA ? (size_t)(((Kc - 1) / 2) * F + 2) * 2 * NS * B * 2 * sizeof(float) : (size_t)2 * NS * B * sizeof(float));
    p.wdt = kind == CHAIN_LSA ? al256((size_t)NS * F * A * sizeof(__bf16)) : 0;
    return p;
}
size_t lstm_x_bytes(int B, int H) { return (size_t)2 * (4 * H / 16) * ((B + 31) / 32) * 1024; }                           // [2][4H/16][MT][1 KB]
size_t lstm_pb_bytes(int B, int H) { return (size_t)2 * GKP * (H / PU) * ((B + 31) / 32) * 32 * PU * sizeof(float); }     // [2][GKP][H/PU][MT][32][PU]

}  // namespace

const char* chain_refusal_text(ChainRefusal r) {
    static const char* const text[CHAIN_REFUSALS] = {
        "covered",
        "a dimension is off the sizes the chain kernels are written for",
        "the tiling of this shape has no kernel instance",
        "the device has fewer than 256 compute units",
        "another process holds the persistent kernels of this device",
        "the tiling's query partials outgrow their part of the exchange space",
        "the LDS carve exceeds 160 KB",
        "LSA reads processed memory from LDS only and the longest memory does not fit",
        "a memory is shorter than 16 positions",
        "an LSA position split is shorter than the conv halo or longer than 64 positions",
        "the forward pass saved no tanh tile and location features",
        "the exchange space is too small",
    };
    return r >= 0 && r < CHAIN_REFUSALS ? text[r] : "?";
}
const char* chain_instance_name(int i) {
    static const char* const name[CHAIN_INSTANCES] = {"fwd_lstm_11", "fwd_lstm_12", "fwd_sma_11", "fwd_sma_21", "fwd_sma_22", "fwd_lsa_11", "fwd_lsa_21",
                                                      "fwd_lsa_22", "fwd_sma_dec", "fwd_lsa_dec", "bwd_lstm_1", "bwd_lstm_2", "bwd_sma_1", "bwd_sma_2",
                                                      "bwd_lsa_1", "bwd_lsa_2", "enc_fwd", "enc_bwd"};
    return i >= 0 && i < CHAIN_INSTANCES ? name[i] : "?";
}
const char* chain_part_name(int i) {
    static const char* const name[CHAIN_PARTS] = {"status", "Q", "X", "XD", "XM", "cnt", "PB", "PBC", "DQX", "CARRYX", "WDT"};
    return i >= 0 && i < CHAIN_PARTS ? name[i] : "?";
}

ChainShape enc_chain_shape(int ND, int B, int H, int backward, size_t ws_bytes) {
    ChainShape z{};
    z.kind = CHAIN_ENC; z.NS = ND; z.B = B; z.H = H; z.backward = backward; z.ws_bytes = ws_bytes;
    return z;
}

size_t chain_fwd_ws_floats(int NS, int B, int Ha, int E, int P, int Hd, int A) {
    return (kStatusBytes + q_part_bytes(NS, B, Ha, A) + x_part_bytes(NS, B, Ha + E + P) + x_part_bytes(1, B, Hd) + kXmBytes + kCntBytes) / sizeof(float);
}
size_t chain_bwd_ws_floats(int kind, int NS, int B, int Ha, int E, int A, int F, int Kc, int Hd) {
    const AttParts p = att_parts(kind, NS, B, Ha, E, A, F, Kc);
    return (p.x + p.pbh + p.pbc + p.dqx + p.carry + p.wdt + lstm_x_bytes(B, Hd) + lstm_pb_bytes(B, Hd)) / sizeof(float);
}

ChainPart chain_fwd_clear_range(size_t ws_bytes, ChainWsClear what) {
    if (ws_bytes < kStatusBytes + kXmBytes + kCntBytes) return ChainPart{0, 0};
    return ChainPart{0, what == CHAIN_WS_STATUS ? kStatusBytes : what == CHAIN_WS_TEACHER ? ws_bytes - kXmBytes - kCntBytes : ws_bytes};
}

// Forward chains and the decode loop: the tiling for a shape, the kernel instance, the LDS residency, the exchange parts.
ChainPlan plan_chain_fwd(const ChainShape& z, const ChainEnv& env) {
    ChainDesc d{};                                                      // the fields geo_of / lds_of read
    d.kind = z.kind; d.dec = z.dec; d.NS = z.NS; d.B = z.B; d.H = z.H; d.E = z.E; d.A = z.A; d.P = z.P; d.M = z.M; d.Hd = z.Hd; d.F = z.F; d.Kc = z.Kc;
    d.st[0].Tin = z.Tin[0]; d.st[1].Tin = z.Tin[1];
    if (d.kind != CHAIN_LSTM && d.kind != CHAIN_SMA && d.kind != CHAIN_LSA) return refuse(CHAIN_REFUSE_SHAPE);
    if (d.H != 1024 || d.B < 1 || d.B > 128) return refuse(CHAIN_REFUSE_SHAPE);
    if (d.kind != CHAIN_LSTM && (d.E != 512 || d.A != 128 || d.NS < 1 || d.NS > 2)) return refuse(CHAIN_REFUSE_SHAPE);
    if (d.kind == CHAIN_LSA && (d.F + 1 > 64 || d.F % 16 != 0 || d.A % 32 != 0)) return refuse(CHAIN_REFUSE_SHAPE);
    const int MT = (d.B + 31) / 32;
    if (d.dec && (MT != 1 || d.NS != 2 || d.kind == CHAIN_LSTM || d.P != 256 || d.Hd != 1024 || d.M + 1 > 96 || d.M % 8 != 0)) return refuse(CHAIN_REFUSE_SHAPE);
    // decoder-LSTM chain: one row tile per item while the items still fit the chip (B <= 64: 128 unit groups x 2 row groups = 256
    // workgroups; with both tiles in one item half the CUs idled and every step did twice the work per workgroup)
    if (d.kind == CHAIN_LSTM) { d.UT = 1; d.RT = (d.H / 8) * MT <= 256 ? 1 : 2; d.CS = 1; d.NS = 1; }
    else {
        d.RT = MT <= 2 ? 1 : 2;
        d.UT = (d.NS * (d.H / 8) * ((MT + d.RT - 1) / d.RT) <= 256) ? 1 : 2;
        d.CS = (!d.dec && d.NS * d.B * 4 <= 256) ? 4 : d.NS * d.B * 2 <= 256 ? 2 : 1;      // (decode: 2, see the D / P items)
    }
    ChainPlan p{};
    p.UT = d.UT; p.RT = d.RT; p.CS = d.CS;
    // the instances that exist: <1,1> and <1,2> of the LSTM kernel, <1,1>, <2,1>, <2,2> of each attention kind, <1,1> of each decode loop
    const int tiling = d.UT == 1 && d.RT == 1 ? 0 : d.UT == 2 && d.RT == 1 ? 1 : d.UT == 2 && d.RT == 2 ? 2 : -1;
    if (d.kind == CHAIN_LSTM) p.instance = d.RT == 1 ? CI_FWD_LSTM_11 : CI_FWD_LSTM_12;
    else if (d.dec) p.instance = tiling == 0 ? (d.kind == CHAIN_LSA ? CI_FWD_LSA_DEC : CI_FWD_SMA_DEC) : -1;
    else p.instance = tiling < 0 ? -1 : (d.kind == CHAIN_LSA ? CI_FWD_LSA_11 : CI_FWD_SMA_11) + tiling;
    const Geo g = geo_of(d, d.UT, d.RT);
    if (g.nL > 256 || g.nA > 256) return refuse(CHAIN_REFUSE_SHAPE);
    if (env.cus < 256) return refuse(CHAIN_REFUSE_DEVICE);
    if (!env.claimed) return refuse(CHAIN_REFUSE_CLAIM);
    // (one stream at 65-96 rows: two row groups of two row tiles pad the query partials beyond their part of the exchange space)
    if (d.kind != CHAIN_LSTM && q_bytes_of(d, g) > q_part_bytes(d.NS, d.B, d.H, d.A)) return refuse(CHAIN_REFUSE_QUERY_PART);
    // LDS residency: processed-memory rows first, then (bf16) memory rows, in what the largest stream leaves free
    const int budget = (kLdsBytes - 256) / 4;
    int tmax = 4;
    for (int s = 0; s < d.NS && d.kind != CHAIN_LSTM; ++s) tmax = std::max(tmax, d.st[s].Tin);
    p.lds_Tin = tmax; p.lds_Jp = 0; p.lds_Jm = 0;
    const int fixed = lds_of(d, d.UT, d.RT, tmax, 0, 0).total;
    if (fixed > budget) return refuse(CHAIN_REFUSE_LDS);
    if (d.kind != CHAIN_LSTM) {
        const int EC = d.E / d.CS;
        int left = budget - fixed + (d.dec ? 16384 : 0);                        // (dec: `fixed` holds the 64 KB pad the rows will take the place of)
        const int pmp = d.kind == CHAIN_LSA ? d.A + 1 : d.A;
        p.lds_Jp = std::min(tmax, left / pmp); left -= p.lds_Jp * pmp;
        if (d.kind == CHAIN_LSA && (p.lds_Jp < tmax || (d.dec && g.nA > 128))) return refuse(CHAIN_REFUSE_LSA_RESIDENT);   // LSA energies read pm from LDS only
        p.lds_Jm = std::min(tmax, left / (EC / 2)) & ~1;
        for (int s = 0; s < d.NS; ++s) { p.Jp[s] = std::min(d.st[s].Tin, p.lds_Jp); p.Jm[s] = std::min(d.st[s].Tin, p.lds_Jm); }
        if (env.no_resident) { if (d.kind != CHAIN_LSA) p.Jp[0] = p.Jp[1] = 0; p.Jm[0] = p.Jm[1] = 0; }
    }
    const int lds = lds_of(d, d.UT, d.RT, tmax, p.lds_Jp, p.lds_Jm).total;
    if (lds > budget) return refuse(CHAIN_REFUSE_LDS);
    // (one stream at 97-128 rows: UT = 1, RT = 2 passes every check above and has no kernel; such a pass takes the per-step launches)
    if (p.instance < 0) return refuse(CHAIN_REFUSE_NO_INSTANCE);
    p.lds_bytes = (size_t)lds * sizeof(float);
    p.grid = d.dec ? 256 : std::max(g.nL, g.nA);
    // exchange parts
    const size_t tail = kXmBytes + kCntBytes;
    if (d.kind == CHAIN_LSTM) {
        const size_t xb = x_part_bytes(1, d.B, d.H);
        p.total = kStatusBytes + xb + tail;
        p.ws_bytes = space_of(z, p);
        p.part[CP_X] = ChainPart{p.ws_bytes - tail - xb, xb};
    } else {
        // (the attention chain's shape carries the pass's P and Hd: a space of at least chain_fwd_ws_floats keeps the parts
        //  carved here clear of the decoder-LSTM chain's part at the back)
        const size_t qb = q_part_bytes(d.NS, d.B, d.H, d.A);
        p.total = chain_fwd_ws_floats(d.NS, d.B, d.H, d.E, d.P, d.Hd, d.A) * sizeof(float);
        p.ws_bytes = space_of(z, p);
        p.q_bytes = q_bytes_of(d, g);
        p.part[CP_Q] = ChainPart{kStatusBytes, qb};
        p.part[CP_X] = ChainPart{kStatusBytes + qb, x_part_bytes(d.NS, d.B, d.H + d.E + d.P)};
        if (d.dec) {
            const size_t xd = x_part_bytes(1, d.B, d.Hd);
            p.part[CP_XD] = ChainPart{p.ws_bytes - tail - xd, xd};
            p.part[CP_XM] = ChainPart{p.ws_bytes - tail, kXmBytes};
            p.part[CP_CNT] = ChainPart{p.ws_bytes - kCntBytes, kCntBytes};
            p.clear = p.part[CP_CNT];                                           // (the decode loop's counters count the steps of one launch)
        }
    }
    p.part[CP_STATUS] = ChainPart{0, kStatusBytes};
    return p;
}

// Backward chains.  Attention chain: every buffer but Wd^T carries step tags (tag 0 = not written yet) and is cleared per
// launch; decoder-LSTM chain: both of its buffers.
ChainPlan plan_chain_bwd(const ChainShape& z, const ChainEnv& env) {
    if (z.kind != CHAIN_LSTM && z.kind != CHAIN_SMA && z.kind != CHAIN_LSA) return refuse(CHAIN_REFUSE_SHAPE);
    if (z.H != 1024 || z.B < 1 || z.B > 64) return refuse(CHAIN_REFUSE_SHAPE);
    ChainPlan p{};
    p.MT = (z.B + 31) / 32;
    const bool lsa = z.kind == CHAIN_LSA;
    if (z.kind != CHAIN_LSTM) {
        if (z.E != 512 || z.A != 128 || z.NS < 1 || z.NS > 2) return refuse(CHAIN_REFUSE_SHAPE);
        if (lsa && (z.F != 32 || z.Kc < 3 || z.Kc > 31 || z.Kc % 2 == 0)) return refuse(CHAIN_REFUSE_SHAPE);     // (F = 32: the reference's attention_location_n_filters)
        const int pad = lsa ? (z.Kc - 1) / 2 : 0;
        int tc = 0;
        for (int s = 0; s < z.NS; ++s) {
            const int Tin = z.Tin[s], chunk = (((Tin + 1) / 2) + 3) & ~3;
            if (Tin < 16) return refuse(CHAIN_REFUSE_SHORT_MEMORY);     // (two position splits per item, as the launch path at these sizes)
            // LSA: both splits hold at least the `pad` rows they hand to each other; one [positions x A] tile row pair per wave
            if (lsa && (Tin - chunk < pad || chunk < pad || chunk > 64)) return refuse(CHAIN_REFUSE_LSA_SPLIT);
            tc = std::max(tc, chunk);
        }
        if (lsa && !z.saved_tiles) return refuse(CHAIN_REFUSE_NO_SAVED_TILES);   // the forward chain's tanh tile / location features
        p.lds_Tc = tc;
        p.lds_bytes = (size_t)bwd_lds_of(z.A, z.E, tc, p.MT, z.kind, z.F, z.Kc).total * sizeof(float);
        if (p.lds_bytes > (size_t)kLdsBytes) return refuse(CHAIN_REFUSE_LDS);
    }
    if (env.cus < 256) return refuse(CHAIN_REFUSE_DEVICE);
    if (!env.claimed) return refuse(CHAIN_REFUSE_CLAIM);
    if (z.kind == CHAIN_LSTM) {
        const size_t xb = lstm_x_bytes(z.B, z.H), pb = lstm_pb_bytes(z.B, z.H);
        p.instance = p.MT == 1 ? CI_BWD_LSTM_1 : CI_BWD_LSTM_2;
        p.lds_bytes = (size_t)(4 + NWV * p.MT * 32 * PPR) * sizeof(float);
        p.grid = (z.H / GNC) * GKP;
        p.total = xb + pb;
        p.ws_bytes = space_of(z, p);
        p.part[CP_X] = ChainPart{p.ws_bytes - xb - pb, xb};
        p.part[CP_PB] = ChainPart{p.ws_bytes - pb, pb};
        p.clear = ChainPart{p.part[CP_X].off, xb + pb};                 // tagged hand-offs: tag 0 = invalid for the first two steps
        return p;
    }
    const AttParts a = att_parts(z.kind, z.NS, z.B, z.H, z.E, z.A, z.F, z.Kc);
    p.instance = (lsa ? CI_BWD_LSA_1 : CI_BWD_SMA_1) + (p.MT == 1 ? 0 : 1);
    p.grid = std::max(std::max(z.NS * (z.E + z.H) / ANC * AKP, z.NS * (z.H / PU) * p.MT), z.NS * z.B * 2);
    size_t off = 0;
    auto take = [&](int id, size_t n) { p.part[id] = ChainPart{off, n}; off += n; };
    take(CP_X, a.x); take(CP_PB, a.pbh); take(CP_PBC, a.pbc); take(CP_DQX, a.dqx); take(CP_CARRYX, a.carry);
    p.clear = ChainPart{0, off};
    take(CP_WDT, a.wdt);                                                // LSA: loc_dense [A][F] as bf16 [F][A] per stream
    p.total = off;
    p.ws_bytes = space_of(z, p);
    return p;
}

// Encoder BiLSTM chains, in floats: [status 64 | counters | h or (dg + partials) | 64]; status words and counters are cleared
// per launch.  (Callers size their space before they know whether the chain covers the shape: any shape has a size.)
size_t enc_chain_ws_floats(int ND, int B, int H, int backward) {
    const size_t NRG = (B + 31) / 32, Bp = NRG * 32;
    const size_t cnt = (size_t)ND * NRG * (backward ? 1 + H / 32 : 1) * CNT_STRIDE;
    const size_t x = backward ? (size_t)2 * ND * (4 * H * Bp + EGKP * H * Bp) : (size_t)2 * ND * H * Bp;
    return 64 + cnt + x + 64;
}
ChainPlan plan_enc_chain(const ChainShape& z, const ChainEnv& env) {
    const int ND = z.NS, B = z.B, H = z.H;
    if (!(ND >= 1 && ND <= 2 && H == EH && B >= 1 && B <= 128)) return refuse(CHAIN_REFUSE_SHAPE);
    ChainPlan p{};
    p.total = enc_chain_ws_floats(ND, B, H, z.backward) * sizeof(float);
    p.ws_bytes = space_of(z, p);
    if (p.ws_bytes < p.total) return refuse(CHAIN_REFUSE_WORKSPACE);
    if (env.cus < 256) return refuse(CHAIN_REFUSE_DEVICE);
    if (!env.claimed) return refuse(CHAIN_REFUSE_CLAIM);
    const int NRG = (B + 31) / 32;
    const size_t Bp = (size_t)NRG * 32, cnt = (size_t)ND * NRG * (z.backward ? 1 + EH / 32 : 1) * CNT_STRIDE;
    p.instance = z.backward ? CI_ENC_BWD : CI_ENC_FWD;
    p.grid = z.backward ? ND * NRG * std::max((EH / 32) * EGKP, EH / EPU) : ND * (EH / 8) * NRG;
    p.lds_bytes = (size_t)(4 + NWV * 32 * PPR + (z.backward ? 0 : 32 * 8)) * sizeof(float);
    size_t off = 0;
    auto take = [&](int id, size_t floats) { p.part[id] = ChainPart{off, floats * sizeof(float)}; off += floats * sizeof(float); };
    take(CP_STATUS, 64); take(CP_CNT, cnt);
    p.clear = ChainPart{0, off};
    take(CP_X, z.backward ? 2 * ND * 4 * EH * Bp : 2 * ND * EH * Bp);
    if (z.backward) take(CP_PB, 2 * ND * EGKP * EH * Bp);
    return p;
}

// ---- plan -> kernel arguments ------------------------------------------------------------------------------------------------
namespace {
template <class T> T* at(float* ws, const ChainPart& part) { return part.bytes ? reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(ws) + part.off) : nullptr; }
}
void apply(const ChainPlan& p, float* ws, ChainDesc* d) {
    d->UT = p.UT; d->RT = p.RT; d->CS = p.CS;
    d->lds_Tin = p.lds_Tin; d->lds_Jp = p.lds_Jp; d->lds_Jm = p.lds_Jm;
    for (int s = 0; s < 2; ++s) { d->Jp[s] = p.Jp[s]; d->Jm[s] = p.Jm[s]; }
    d->Q = at<float>(ws, p.part[CP_Q]); d->q_bytes = (unsigned)p.q_bytes;
    d->X = at<unsigned char>(ws, p.part[CP_X]); d->XD = at<unsigned char>(ws, p.part[CP_XD]); d->XM = at<unsigned char>(ws, p.part[CP_XM]);
    d->cnt = at<unsigned>(ws, p.part[CP_CNT]);
}
void apply(const ChainPlan& p, float* ws, ChainBwdDesc* d) {
    d->X = at<unsigned char>(ws, p.part[CP_X]); d->PB = at<unsigned char>(ws, p.part[CP_PB]); d->pb_bytes = (unsigned)p.part[CP_PB].bytes;
    d->PBC = at<unsigned char>(ws, p.part[CP_PBC]); d->pbc_bytes = (unsigned)p.part[CP_PBC].bytes;
    d->DQX = at<float>(ws, p.part[CP_DQX]); d->CARRYX = at<float>(ws, p.part[CP_CARRYX]);
    d->lds_Tc = p.lds_Tc;
    for (int s = 0; s < d->NS && p.part[CP_WDT].bytes; ++s) d->st[s].wdt16 = at<const __bf16>(ws, p.part[CP_WDT]) + (size_t)s * d->F * d->A;
}
void apply(const ChainPlan& p, float* ws, EncChainDesc* d) {
    d->err = at<unsigned>(ws, p.part[CP_STATUS]); d->cnt = at<unsigned>(ws, p.part[CP_CNT]); d->X = at<float>(ws, p.part[CP_X]);
}
void apply(const ChainPlan& p, float* ws, EncChainBwdDesc* d) {
    d->err = at<unsigned>(ws, p.part[CP_STATUS]); d->cnt = at<unsigned>(ws, p.part[CP_CNT]); d->X = at<float>(ws, p.part[CP_X]);
    d->PB = at<float>(ws, p.part[CP_PB]);
}

}  // namespace t2
