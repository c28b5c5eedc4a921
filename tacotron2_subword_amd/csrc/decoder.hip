// Host drivers of the three decoder passes (t2_decoder_forward, t2_decoder_backward, t2_decoder_infer): per-stream tables,
// step and chain descriptors, and the stages that execute the pass's plan (decoder_plan.h decides; nothing here does).
// No device allocation, no synchronisation except where include/t2amd.h says so.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "../../include/t2amd.h"
#include "kernels.h"
#include "chain_plan.h"
#include "decoder_plan.h"
#include "driver.h"

using namespace t2;

// After the persistent kernels of a pass: if one of them aborted (non-zero status word of the pass), its outputs are
// garbage — overwrite them with NaN so that whatever consumes them (a loss, a vocoder, a file) cannot take them for data.
__global__ __launch_bounds__(256) void poison_if_aborted_kernel(const unsigned* __restrict__ status, int nwords, float* __restrict__ a, size_t na,
                                                                float* __restrict__ b, size_t nb) {
    unsigned any = 0;
    for (int i = 0; i < nwords; ++i) any |= status[i];
    if (!any) return;
    const float qnan = __builtin_nanf("");
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na; i += (size_t)gridDim.x * 256) a[i] = qnan;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (size_t)gridDim.x * 256) b[i] = qnan;
}

namespace {

int check_dims(const t2_dims& d) {
    T2_REQUIRE(d.n_mel % 4 == 0, "n_mel %d must be a multiple of 4", d.n_mel);
    T2_REQUIRE(d.prenet_dim % 64 == 0 && d.enc_dim % 64 == 0 && d.att_rnn_dim % 64 == 0 && d.dec_rnn_dim % 64 == 0,
               "prenet/encoder/rnn dims must be multiples of 64 (got %d %d %d %d)", d.prenet_dim, d.enc_dim, d.att_rnn_dim, d.dec_rnn_dim);
    T2_REQUIRE(d.att_dim % 4 == 0 && d.att_dim <= 256, "attention_dim %d unsupported", d.att_dim);
    T2_REQUIRE(d.attention_kind == T2_ATTN_SMA || d.attention_kind == T2_ATTN_LSA || d.attention_kind == T2_ATTN_FWD2 || d.attention_kind == T2_ATTN_GMM || d.attention_kind == T2_ATTN_DCA, "unknown attention kind %d", d.attention_kind);
    return 0;
}

// ForwardAttentionV2 as the reference runs it (attention.py:87-151; the caller never updates log_alpha, model.py:266-270,
// 355): log_alpha stays [0, -1e4, -1e4, ...], so the "forward" bias logsumexp(log_alpha_j, log_alpha_{j-1}) is exactly 0
// for j < 2 and about -1e4 beyond, and softmax(bias + energy) is the LSA softmax over the first two positions with
// exact zeros elsewhere.  It therefore runs on the LSA kernels with the valid length clamped to 2.
t2_dims canon_dims(const t2_dims& in, int* max_pos) {
    t2_dims d = in;
    *max_pos = 0;
    if (d.attention_kind == T2_ATTN_FWD2) { d.attention_kind = T2_ATTN_LSA; *max_pos = 2; }
    return d;
}
// Prologue of every entry point: the caller's dims checked and made canonical, or the error
int entry_dims(const t2_dims& in, t2_dims* d, int* max_pos) {
    T2_TRY(check_dims(in));
    *d = canon_dims(in, max_pos);
    return 0;
}

// score_mask_value `v` of a stream's attention module; a zero-initialised t2_dims (0.0) means the default, -inf
float mask_value_of(const t2_dims& d, float v) {
    return (v == 0.f && !d.score_mask_given) ? -INFINITY : v;
}

// The status words of a pass (ChainStatus, kernels.h): the head of the forward workspace's chain region
unsigned* status_words(const float* ws, const t2_decoder_layout& L) { return reinterpret_cast<unsigned*>(const_cast<float*>(ws) + L.chain); }

// One attention stream of a pass (row 0: text, row 1: sub-word): everything that differs between the two.  stream_refs
// fills both rows once per pass; with bwd_stream_refs it is the only place that names a *_sub field or an ...s offset.
struct StreamRef {
    int Tin, hoff, coff, ctx2off;                    // columns: the stream's h and ctx in a DIN row, its ctx in a DOUT row
    const t2_lstm_weights* lw; const t2_attention_weights* aw; const float *prenet_w1, *prenet_w2;
    const float* memory; const int32_t* lengths; float* align;
    size_t p1, p2, pm, prea, ga, cna, ca, psel, wcum, qs, w16, wt16, usave, locsave;     // forward workspace (t2_decoder_layout)
    uint32_t site_h, site_c, site_noise, site_p1, site_p2;
    float mask_value;                                // attention.py:37,79 / train.py:77-78
};
void stream_refs(const t2_dims& d, const t2_decoder_weights& w, const Sizes& z, const t2_decoder_layout& L, const float* memory,
                 const float* memory_sub, const int32_t* len, const int32_t* len_sub, float* align, float* align_sub, StreamRef* st) {
    for (int s = 0; s < 2; ++s) {
        StreamRef& r = st[s];
        r.Tin = s ? z.Tsub : z.Tin; r.hoff = s ? z.Ha + z.E : 0; r.coff = r.hoff + z.Ha; r.ctx2off = z.Hd + (s ? z.E : 0);
        r.lw = s ? &w.att_sub : &w.att; r.aw = s ? &w.attn_sub : &w.attn;
        r.prenet_w1 = s ? w.prenet_sub_w1 : w.prenet_w1; r.prenet_w2 = s ? w.prenet_sub_w2 : w.prenet_w2;
        r.memory = s ? memory_sub : memory; r.lengths = s ? len_sub : len; r.align = s ? align_sub : align;
        r.p1 = s ? L.p1s : L.p1; r.p2 = s ? L.p2s : L.p2; r.pm = s ? L.pms : L.pm; r.prea = s ? L.preas : L.prea;
        r.ga = s ? L.gas : L.ga; r.cna = s ? L.cnas : L.cna; r.ca = s ? L.cas : L.ca;
        r.psel = s ? L.psels : L.psel; r.wcum = s ? L.wcums : L.wcum; r.qs = s ? L.qss : L.qs;
        r.w16 = s ? L.w16as : L.w16a; r.wt16 = s ? L.wt16as : L.wt16a;
        r.usave = s ? L.usaves : L.usave; r.locsave = s ? L.locsaves : L.locsave;
        r.site_h = s ? T2_SITE_ATT_H_SUB : T2_SITE_ATT_H; r.site_c = s ? T2_SITE_ATT_C_SUB : T2_SITE_ATT_C;
        r.site_noise = s ? T2_SITE_NOISE_SUB : T2_SITE_NOISE;
        r.site_p1 = s ? T2_SITE_PRENET1_SUB : T2_SITE_PRENET1; r.site_p2 = s ? T2_SITE_PRENET2_SUB : T2_SITE_PRENET2;
        r.mask_value = mask_value_of(d, s ? d.score_mask_value_sub : d.score_mask_value);
    }
}

// The LSA backward chain reads the tanh tile and the location features the forward CHAIN saved (layout.usave / locsave); a
// workspace filled by the per-step launch path does not hold them.  Which workspaces do is kept here, per base pointer
// (every forward pass notes its own; host-side only, no device round trip).
std::mutex g_saved_mu;
std::unordered_map<const void*, bool> g_saved_tiles;
void saved_tiles_note(const void* ws, bool saved) {
    std::lock_guard<std::mutex> lk(g_saved_mu);
    if (g_saved_tiles.size() > 4096) g_saved_tiles.clear();
    g_saved_tiles[ws] = saved;
}
bool saved_tiles_have(const void* ws) {
    std::lock_guard<std::mutex> lk(g_saved_mu);
    auto it = g_saved_tiles.find(ws);
    return it != g_saved_tiles.end() && it->second;
}

// The one reader of the process and the device for a pass plan: the mode and the switches in force, for a backward pass
// whether its forward workspace holds saved tiles (fwd_ws), and, for a pass that will run (device), chain_env() without the claim
PassEnv pass_env_here(const void* fwd_ws, bool device) {
    PassEnv env{get_precision(), g_split_steps != 0, g_chain != 0, g_chain_bwd != 0, g_overlap != 0, ChainEnv{0, false, false}, fwd_ws && saved_tiles_have(fwd_ws),
                g_dg_handoff != 0, gemm_env_here().stage, gemm_env_here().tiles256};
    if (device && env.chain) env.chain_env = chain_env(false);
    return env;
}
// The plan of a pass here, in the style of plan_here: the pure plan first, with the claim taken for granted; the per-GPU claim
// is asked for only once that plan has accepted a chain, so a process whose passes take no chain takes no claim.
template <class Plan>
auto pass_plan_here(PassEnv env, Plan plan) {
    auto p = plan(env);
    if (p.chain_a.on || p.chain_b.on) { env.chain_env = chain_env(true); p = plan(env); }
    return p;
}

// The shape fields of a chain descriptor are the planned ones (ChainUse::shape); the builders below add T, the row widths and pointers
void shape_into(const ChainShape& z, ChainDesc* d) {
    d->kind = z.kind; d->dec = z.dec; d->NS = z.NS; d->B = z.B; d->H = z.H; d->E = z.E; d->A = z.A; d->P = z.P; d->M = z.M; d->Hd = z.Hd; d->F = z.F; d->Kc = z.Kc;
    d->st[0].Tin = z.Tin[0]; d->st[1].Tin = z.Tin[1];
}
void shape_into(const ChainShape& z, ChainBwdDesc* d) {
    d->kind = z.kind; d->NS = z.NS; d->B = z.B; d->H = z.H; d->E = z.E; d->A = z.A; d->F = z.F; d->Kc = z.Kc;
    d->st[0].Tin = z.Tin[0]; d->st[1].Tin = z.Tin[1];
}

// A teacher-forced forward pass or a decode loop in execution: the plan, the caller's arguments, the streams' rows
struct Dec {
    const t2_dims& d; const t2_decoder_weights& w; const DecPlan p; float* ws;
    bool training; bool prenet_dropout; uint64_t seed; hipStream_t s;
    int max_pos;                                     // > 0: attention restricted to the first max_pos positions (ForwardAttentionV2)
    const Sizes& z = p.z; const t2_decoder_layout& L = p.L; const InferShadows& I = p.I; const bool teacher = p.teacher;
    StreamRef st[2]{};
    hipStream_t sd = nullptr;                        // stream of the decoder-LSTM chain (== s unless overlapped)
    Dec(const Dec&) = delete;                        // (z, L, I refer to this object's plan)
    __bf16* RowA(int parity, int s) const { return reinterpret_cast<__bf16*>(ws + I.rows_a) + (size_t)(parity * 2 + s) * z.B * I.Ka; }
    __bf16* RowD(int parity) const { return reinterpret_cast<__bf16*>(ws + I.rows_d) + (size_t)parity * z.B * I.Kd; }
    float* P(size_t off) const { return ws + off; }
    __bf16* P16(size_t off) const { return reinterpret_cast<__bf16*>(ws + off); }
    // a part of the GEMM scratch (ScratchCarve, decoder_plan.h): its address, a product working in it
    unsigned char* scratch(size_t off) const { return reinterpret_cast<unsigned char*>(ws + L.gemm_ws) + off; }
    GemmDesc in(const ScratchPart& part, GemmDesc m) const { m.ws = reinterpret_cast<float*>(scratch(part.off)); m.ws_bytes = part.bytes; return m; }
    long R(int t) const { return (long)t * z.B; }      // first row of step t in a time-major [T,B,*] buffer
};

// C[M,N] = A . B with element strides (sam, sak) of A and (sbn, sbk) of B
GemmDesc product(const float* A, long sam, long sak, const float* B, long sbn, long sbk, float* C, long ldc, int M, int N, int K) {
    GemmDesc g = gemm_desc();
    g.A = A; g.sam = sam; g.sak = sak;
    g.B = B; g.sbn = sbn; g.sbk = sbk;
    g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    return g;
}
// C[M,N] = X[M,K] . W[N,K]^T   (a torch Linear without its bias)
GemmDesc linear(const float* X, long ldx, const float* W, long ldw, float* Y, long ldy, int M, int N, int K) {
    return product(X, ldx, 1, W, ldw, 1, Y, ldy, M, N, K);
}

// prenet of stream s for rows [row0, row0+rows) of the [B,T] grid.  teacher: all B*T rows at once.
int prenet(const Dec& c, int s, const float* X, long ldx, int M, float* P1, float* P2, long ldp, uint32_t base, uint32_t mstride) {
    const Sizes& z = c.z; const StreamRef& r = c.st[s];
    auto layer = [&](const float* in, long ldin, const float* W, int K, float* out, uint32_t site) {
        GemmDesc g = linear(in, ldin, W, K, out, ldp, M, z.P, K);
        g.act = ACT_RELU;
        if (c.prenet_dropout) {
            g.drop_p = c.d.p_prenet_dropout; g.seed = c.seed; g.site = site;
            g.drop_base = base; g.drop_mstride = mstride;
        }
        return gemm(g, c.s);
    };
    T2_TRY(layer(X, ldx, r.prenet_w1, z.M, P1, r.site_p1));
    return layer(P1, ldp, r.prenet_w2, z.P, P2, r.site_p2);
}

// One part of a weight shadow: `rows` x `cols` of src, kept K-contiguous or transposed, as one bf16 plane or (split) as
// hi / lo planes `lo` elements apart
int cast_part(const float* src, long lds, __bf16* dst, size_t lo, long ldd, int rows, int cols, bool transpose, bool split, hipStream_t s) {
    if (split) return transpose ? cast_transpose_split_bf16(src, lds, dst, dst + lo, ldd, rows, cols, s) : cast_rows_split_bf16(src, lds, dst, dst + lo, ldd, rows, cols, s);
    return transpose ? cast_transpose_bf16(src, lds, dst, ldd, rows, cols, s) : cast_rows_bf16(src, lds, dst, ldd, rows, cols, s);
}
// weight shadows for one teacher-forced pass: [W_hh | W_ih[:,P:]] (K-contiguous, forward) and its transpose laid out
// [ctx columns | h columns] x 4H (backward), per attention stream; W_hh and W_hh^T of the decoder LSTM.  split: as hi / lo
// planes for the split-bf16 steps (the layout then has a lo plane behind each shadow)
int cast_shadows(const Dec& c, bool split) {
    const Sizes& z = c.z;
    const long K = z.Ha + z.E, ldi = z.P + z.E;
    const size_t loa = (size_t)4 * z.Ha * K, lod = (size_t)4 * z.Hd * z.Hd;        // split_lo_a / split_lo_d in bf16 elements
    for (int s = 0; s < z.NS; ++s) {
        const t2_lstm_weights& lw = *c.st[s].lw;
        __bf16 *f = c.P16(c.st[s].w16), *tr = c.P16(c.st[s].wt16);
        T2_TRY(cast_part(lw.w_hh, z.Ha, f, loa, K, 4 * z.Ha, z.Ha, false, split, c.s));
        T2_TRY(cast_part(lw.w_ih + z.P, ldi, f + z.Ha, loa, K, 4 * z.Ha, z.E, false, split, c.s));
        T2_TRY(cast_part(lw.w_ih + z.P, ldi, tr, loa, 4 * z.Ha, 4 * z.Ha, z.E, true, split, c.s));
        T2_TRY(cast_part(lw.w_hh, z.Ha, tr + (long)z.E * 4 * z.Ha, loa, 4 * z.Ha, 4 * z.Ha, z.Ha, true, split, c.s));
    }
    T2_TRY(cast_part(c.w.dec.w_hh, z.Hd, c.P16(c.L.w16d), lod, z.Hd, 4 * z.Hd, z.Hd, false, split, c.s));
    return cast_part(c.w.dec.w_hh, z.Hd, c.P16(c.L.wt16d), lod, 4 * z.Hd, 4 * z.Hd, z.Hd, true, split, c.s);
}

// attention kind of the ABI (T2_ATTN_*; ForwardAttentionV2 has become LSA by now, normalise()) -> the kernels' kind
AttnKind kernel_kind(int kind) {
    return kind == T2_ATTN_GMM ? AttnKind::GMM : kind == T2_ATTN_DCA ? AttnKind::DCA : kind == T2_ATTN_SMA ? AttnKind::SMA : AttnKind::LSA;
}

DcaWeights dca_weights(const t2_attention_weights& aw) {
    DcaWeights w{};
    w.bW = aw.mlp_b1; w.V = aw.mlp_w2; w.F = aw.loc_conv; w.U = aw.loc_dense; w.T = aw.dca_T; w.bT = aw.dca_bT; w.v = aw.v; w.P = aw.dca_P;
    return w;
}

int att_lstm_step(const Dec& c, int t) {
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L;
    LstmStepDesc d{};
    d.nstreams = z.NS; d.B = z.B; d.H = z.Ha; d.seed = c.seed;
    d.drop_p = c.training ? c.d.p_att_dropout : 0.f;
    float* DIN = c.P(L.din);
    for (int s = 0; s < z.NS; ++s) {
        LstmStream& st = d.st[s]; const StreamRef& r = c.st[s];
        const t2_lstm_weights& lw = *r.lw;
        const int hoff = r.hoff, coff = r.coff;
        int n = 0;
        if (!c.teacher) {
            st.seg[n++] = LstmSeg{c.P(r.p2) + c.R(t) * z.P, (long)z.P, lw.w_ih, (long)(z.P + z.E), z.P};
            st.bias1 = lw.b_ih; st.bias2 = lw.b_hh;
        } else {
            st.pre = c.P(r.prea) + c.R(t) * 4 * z.Ha; st.ldpre = 4 * z.Ha;
        }
        if (t > 0) {
            st.seg[n++] = LstmSeg{DIN + c.R(t - 1) * z.WD + coff, (long)z.WD, lw.w_ih + z.P, (long)(z.P + z.E), z.E};
            st.seg[n++] = LstmSeg{DIN + c.R(t - 1) * z.WD + hoff, (long)z.WD, lw.w_hh, (long)z.Ha, z.Ha};
            st.c_prev = c.P(r.ca) + c.R(t - 1) * z.Ha; st.ldc_prev = z.Ha;
        }
        st.nseg = n;
        st.gates = c.P(r.ga) + c.R(t) * 4 * z.Ha; st.ldgates = 4 * z.Ha;
        st.c_new = c.P(r.cna) + c.R(t) * z.Ha; st.ldc_new = z.Ha;
        st.c_out = c.P(r.ca) + c.R(t) * z.Ha; st.ldc_out = z.Ha;
        st.h_out = DIN + c.R(t) * z.WD + hoff; st.ldh_out = z.WD;
        st.site_h = r.site_h; st.site_c = r.site_c;
        st.idx_base = (uint32_t)(c.R(t) * z.Ha); st.idx_bstride = (uint32_t)z.Ha;       // logical [T,B,Ha]
        st.wq = r.aw->wq; st.A = z.A;
        st.qpart = c.P(L.qpart) + (size_t)s * (z.Ha / 8) * z.B * z.A;
        if (c.p.use16 && !c.teacher) {                 // decode loop: [h | ctx | prenet] x [W_hh | W_ih[:,P:] | W_ih[:,:P]]
            st.nseg = 0;
            st.x16 = c.RowA(t & 1, s); st.ldx16 = c.I.Ka; st.w16 = c.P16(c.I.wa[s]); st.ldw16 = c.I.Ka; st.k16 = c.I.Ka;
            st.h16_out = c.RowA((t + 1) & 1, s); st.ldh16 = c.I.Ka;
            st.h16_out2 = c.RowD(t & 1) + hoff; st.ldh16_2 = c.I.Kd;
        } else if (c.p.use16) {                        // one K-contiguous bf16 segment [h | ctx] x [W_hh | W_ih[:,P:]]
            __bf16* D16 = c.P16(L.din16);
            st.nseg = 0;
            st.x16 = D16 + (t > 0 ? c.R(t - 1) * z.WD + hoff : 0); st.ldx16 = z.WD;
            st.w16 = c.P16(r.w16); st.ldw16 = z.Ha + z.E; st.k16 = t > 0 ? z.Ha + z.E : 0;
            st.h16_out = D16 + c.R(t) * z.WD + hoff; st.ldh16 = z.WD;
        } else if (c.p.split && c.teacher) {           // the same product on fp32 rows [h | ctx] of DIN and hi / lo shadows
            st.nseg = 0;
            st.xs = DIN + (t > 0 ? c.R(t - 1) * z.WD + hoff : 0); st.ldxs = z.WD;
            st.w16 = c.P16(r.w16); st.w16lo = c.P16(split_lo_a(z, r.w16)); st.ldw16 = z.Ha + z.E; st.k16 = t > 0 ? z.Ha + z.E : 0;
        }
    }
    ProfScope ps(PK_LSTM_ATT_FWD, c.s);
    int family = 0;
    return counted(lstm_step_fwd(d, c.s, &family), 0, family);
}

int attention_step(const Dec& c, int t) {
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L;
    AttnStepDesc d{};
    d.nstreams = z.NS; d.B = z.B; d.A = z.A; d.E = z.E;
    const int abi_kind = c.d.attention_kind; d.kind = kernel_kind(abi_kind);
    d.F = c.d.loc_filters; d.Kc = c.d.loc_kernel; d.seed = c.seed; d.first = t == 0;
    d.noise_std = (c.training && abi_kind == T2_ATTN_SMA) ? 2.0f : 0.f;   // attention.py:315,346-348
    d.max_pos = c.max_pos;
    for (int s = 0; s < z.NS; ++s) {
        AttnStream& st = d.st[s]; const StreamRef& r = c.st[s];
        const t2_attention_weights& aw = *r.aw;
        const int Tin = r.Tin;
        float* al = r.align;                                         // [B,T,Tin]: the reference's output layout
        const long ldA = (long)z.T * Tin;
        st.Tin = Tin;
        st.qpart = c.P(L.qpart) + (size_t)s * (z.Ha / 8) * z.B * z.A; st.nparts = z.Ha / 8;
        st.q_out = c.P(r.qs) + c.R(t) * z.A; st.ldq_out = z.A;
        st.pm = c.P(r.pm); st.memory = r.memory; st.lengths = r.lengths;
        st.a_prev = t > 0 ? al + (long)(t - 1) * Tin : nullptr; st.lda_prev = ldA;
        st.a_out = al + (long)t * Tin; st.lda_out = ldA;
        if (abi_kind == T2_ATTN_DCA) {
            st.dca = dca_weights(aw);
        } else if (abi_kind == T2_ATTN_GMM) {
            float* mu = c.P(r.wcum);                    // [T,B,kGmmPad]
            st.mu_prev = t > 0 ? mu + c.R(t - 1) * kGmmPad : nullptr; st.mu_out = mu + c.R(t) * kGmmPad;
            st.gmm_b1 = aw.mlp_b1; st.gmm_w2 = aw.mlp_w2; st.gmm_b2 = aw.mlp_b2;
        } else if (abi_kind == T2_ATTN_SMA) {
            st.p_out = c.P(r.psel) + (long)t * Tin; st.ldp_out = ldA;
        } else {
            float* wc = c.P(r.wcum);
            st.wcum_prev = t > 0 ? wc + (long)(t - 1) * Tin : nullptr; st.ldwcum_prev = ldA;
            st.wcum_out = wc + (long)t * Tin; st.ldwcum_out = ldA;
        }
        st.ctx1 = c.P(L.din) + c.R(t) * z.WD + r.coff; st.ldctx1 = z.WD;
        st.ctx2 = c.P(L.dout) + c.R(t) * z.WO + r.ctx2off; st.ldctx2 = z.WO;
        if (c.p.use16 && !c.teacher) {
            st.ctx16 = c.RowA((t + 1) & 1, s) + z.Ha; st.ldctx16 = c.I.Ka;
            st.ctx16b = c.RowD(t & 1) + r.coff; st.ldctx16b = c.I.Kd;
        } else if (c.p.use16) { st.ctx16 = c.P16(L.din16) + c.R(t) * z.WD + r.coff; st.ldctx16 = z.WD; }
        st.v = aw.v; st.loc_conv = aw.loc_conv; st.loc_dense = aw.loc_dense;
        st.site_noise = r.site_noise; st.mask_value = r.mask_value;
        st.idx_base = (uint32_t)(c.R(t) * Tin); st.idx_bstride = (uint32_t)Tin;          // logical [T,B,Tin]
    }
    ProfScope ps(PK_ATTN_FWD, c.s);
    return attention_step_fwd(d, c.s);
}

int dec_lstm_step(const Dec& c, int t) {
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L;
    LstmStepDesc d{};
    d.nstreams = 1; d.B = z.B; d.H = z.Hd; d.seed = c.seed;
    d.drop_p = c.training ? c.d.p_dec_dropout : 0.f;
    LstmStream& st = d.st[0];
    int n = 0;
    if (!c.teacher) {
        st.seg[n++] = LstmSeg{c.P(L.din) + c.R(t) * z.WD, (long)z.WD, c.w.dec.w_ih, (long)z.WD, z.WD};
        st.bias1 = c.w.dec.b_ih; st.bias2 = c.w.dec.b_hh;
    } else {
        st.pre = c.P(L.pred) + c.R(t) * 4 * z.Hd; st.ldpre = 4 * z.Hd;
    }
    if (t > 0) {
        st.seg[n++] = LstmSeg{c.P(L.dout) + c.R(t - 1) * z.WO, (long)z.WO, c.w.dec.w_hh, (long)z.Hd, z.Hd};
        st.c_prev = c.P(L.cd) + c.R(t - 1) * z.Hd; st.ldc_prev = z.Hd;
    }
    st.nseg = n;
    st.gates = c.P(L.gd) + c.R(t) * 4 * z.Hd; st.ldgates = 4 * z.Hd;
    st.c_new = c.P(L.cnd) + c.R(t) * z.Hd; st.ldc_new = z.Hd;
    st.c_out = c.P(L.cd) + c.R(t) * z.Hd; st.ldc_out = z.Hd;
    st.h_out = c.P(L.dout) + c.R(t) * z.WO; st.ldh_out = z.WO;
    st.site_h = T2_SITE_DEC_H; st.site_c = T2_SITE_DEC_C;
    st.idx_base = (uint32_t)(c.R(t) * z.Hd); st.idx_bstride = (uint32_t)z.Hd;             // logical [T,B,Hd]
    if (c.p.use16 && !c.teacher) {                     // decode loop: [att_h | ctx | att_h_sub | ctx_sub | dec_h] x [W_ih | W_hh]
        st.nseg = 0;
        st.x16 = c.RowD(t & 1); st.ldx16 = c.I.Kd; st.w16 = c.P16(c.I.wd); st.ldw16 = c.I.Kd; st.k16 = c.I.Kd;
        st.h16_out = c.RowD((t + 1) & 1) + z.WD; st.ldh16 = c.I.Kd;
    } else if (c.p.use16) {
        __bf16* H16 = c.P16(L.dh16);
        st.nseg = 0;
        st.x16 = H16 + (t > 0 ? c.R(t - 1) * z.Hd : 0); st.ldx16 = z.Hd;
        st.w16 = c.P16(L.w16d); st.ldw16 = z.Hd; st.k16 = t > 0 ? z.Hd : 0;
        st.h16_out = H16 + c.R(t) * z.Hd; st.ldh16 = z.Hd;
    } else if (c.p.split && c.teacher) {               // fp32 dec_h rows of DOUT, hi / lo shadows of W_hh
        st.nseg = 0;
        st.xs = c.P(L.dout) + (t > 0 ? c.R(t - 1) * z.WO : 0); st.ldxs = z.WO;
        st.w16 = c.P16(L.w16d); st.w16lo = c.P16(split_lo_d(z, L.w16d)); st.ldw16 = z.Hd; st.k16 = t > 0 ? z.Hd : 0;
    }
    hipStream_t sd = c.sd ? c.sd : c.s;
    ProfScope ps(PK_LSTM_DEC_FWD, sd);
    int family = 0;
    return counted(lstm_step_fwd(d, sd, &family), 0, family);
}

// Persistent-kernel descriptors of the two teacher-forced chains (chain.hip): the shape and the pointers.  Whether a chain
// runs, and its ChainPlan, is the pass plan's (c.p.chain_a / chain_b): a builder is called for a chain that is on.
ChainDesc chain_a_desc(const Dec& c) {
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L;
    ChainDesc d{};
    shape_into(c.p.chain_a.shape, &d);
    d.T = z.T; d.WD = z.WD; d.WO = z.WO;
    d.din = c.P(L.din); d.din16 = c.P16(L.din16); d.dout = c.P(L.dout);
    d.max_pos = c.max_pos;
    d.drop_p = c.training ? c.d.p_att_dropout : 0.f;
    d.noise_std = (c.training && d.kind == CHAIN_SMA) ? 2.0f : 0.f;
    d.seed = c.seed;
    for (int s = 0; s < z.NS; ++s) {
        ChainStream& st = d.st[s]; const StreamRef& r = c.st[s];
        const t2_attention_weights& aw = *r.aw;
        const int hoff = r.hoff;
        st.w16 = c.P16(r.w16); st.ldw16 = z.Ha + z.E;
        st.pre = c.P(r.prea); st.wq = aw.wq;
        st.gates = c.P(r.ga); st.c_new = c.P(r.cna); st.c_out = c.P(r.ca);
        st.h_out = c.P(L.din) + hoff; st.ldh = z.WD; st.h16_out = c.P16(L.din16) + hoff; st.ldh16 = z.WD;
        st.coff = r.coff; st.ctx2off = r.ctx2off;
        st.pm = c.P(r.pm); st.memory = r.memory; st.lengths = r.lengths;
        st.align = r.align; st.psel = c.P(r.psel); st.wcum = c.P(r.wcum);
        st.qs = c.P(r.qs);
        st.v = aw.v; st.loc_conv = aw.loc_conv; st.loc_dense = aw.loc_dense;
        if (d.kind == CHAIN_LSA) { st.usave = c.P(r.usave); st.locsave = c.P(r.locsave); }
        st.site_h = r.site_h; st.site_c = r.site_c; st.site_noise = r.site_noise;
        st.mask_value = r.mask_value;
    }
    d.err = status_words(c.ws, L) + CHAIN_STATUS_FWD_ATT;
    return d;
}
ChainDesc chain_b_desc(const Dec& c) {
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L;
    ChainDesc d{};
    shape_into(c.p.chain_b.shape, &d);
    d.T = z.T; d.WD = z.WD; d.WO = z.WO;
    d.drop_p = c.training ? c.d.p_dec_dropout : 0.f;
    d.seed = c.seed;
    ChainStream& st = d.st[0];
    st.w16 = c.P16(L.w16d); st.ldw16 = z.Hd; st.pre = c.P(L.pred);
    st.gates = c.P(L.gd); st.c_new = c.P(L.cnd); st.c_out = c.P(L.cd);
    st.h_out = c.P(L.dout); st.ldh = z.WO; st.h16_out = c.P16(L.dh16); st.ldh16 = z.Hd;
    st.site_h = T2_SITE_DEC_H; st.site_c = T2_SITE_DEC_C;
    d.err = status_words(c.ws, L) + CHAIN_STATUS_FWD_LSTM;
    return d;
}

// Persistent decode loop (chain.hip, dec mode): every phase of Decoder.inference's step inside one launch per step range
ChainDesc chain_dec_desc(const Dec& c, const t2_decoder_infer_args& a) {
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L; const t2_decoder_weights& w = c.w;
    ChainDesc d{};
    shape_into(c.p.chain_a.shape, &d);
    d.T = z.T; d.WD = z.WD; d.WO = z.WO; d.max_pos = c.max_pos;
    d.drop_p = 0.f; d.noise_std = 0.f; d.seed = c.seed;                 // inference runs in eval mode (inference.py:263)
    for (int s = 0; s < z.NS; ++s) {
        ChainStream& st = d.st[s]; const StreamRef& r = c.st[s];
        const t2_attention_weights& aw = *r.aw;
        st.w16 = c.P16(c.I.wa[s]); st.ldw16 = c.I.Ka; st.wq = aw.wq;
        st.pm = c.P(r.pm); st.memory = r.memory; st.lengths = r.lengths;
        st.align = r.align; st.wcum = c.P(r.wcum);
        st.v = aw.v; st.loc_conv = aw.loc_conv; st.loc_dense = aw.loc_dense;
        st.site_h = r.site_h; st.site_c = r.site_c; st.site_noise = r.site_noise;
        st.mask_value = r.mask_value;
        d.bias1[s] = r.lw->b_ih; d.bias2[s] = r.lw->b_hh;
        d.att_c[s] = c.P(r.ca);                              // (row 0 of the per-frame buffers: unused in decode)
        d.pw1[s] = r.prenet_w1; d.pw2[s] = r.prenet_w2;
        d.psite1[s] = r.site_p1; d.psite2[s] = r.site_p2;
    }
    d.wd16 = c.P16(c.I.wd); d.ldwd = c.I.Kd; d.dbias1 = w.dec.b_ih; d.dbias2 = w.dec.b_hh; d.dec_c = c.P(L.cd);
    d.proj_w = w.proj_w; d.proj_b = w.proj_b; d.gate_w = w.gate_w; d.gate_b = w.gate_b;
    d.mel_out = a.mel_out; d.ldmel = (long)z.T * z.M; d.gate_out = a.gate_out; d.ldgate = z.T;
    d.thr = a.gate_threshold; d.stop_index = a.stop_index; d.done = a.done_count;
    d.pdrop = c.prenet_dropout ? c.d.p_prenet_dropout : 0.f;
    d.err = status_words(c.ws, L) + CHAIN_STATUS_FWD_ATT;
    return d;
}

// mel / gate projection (model.py:382-388); permute_tb: rows come time-major, outputs are [B,T,*]
int projection(const Dec& c, const float* X, long ldx, int M, float* mel, long ldmel, float* gate, long ldgate, bool permute_tb) {
    const Sizes& z = c.z;
    auto head = [&](const float* W, const float* bias, float* out, long ldo, int N) {
        GemmDesc g = linear(X, ldx, W, z.WO, out, ldo, M, N, z.WO);
        g.bias1 = bias;
        if (permute_tb) { g.crow_mod = z.B; g.crow_mul = z.T; }      // row (t,b) of DOUT -> row (b,t) of the output
        return gemm(g, c.s);
    };
    T2_TRY(head(c.w.proj_w, c.w.proj_b, mel, ldmel, z.M));
    return head(c.w.gate_w, c.w.gate_b, gate, ldgate, 1);
}

int processed_memory(const Dec& c) {
    const Sizes& z = c.z;
    if (c.d.attention_kind == T2_ATTN_GMM || c.d.attention_kind == T2_ATTN_DCA) return 0;   // purely location-based: memory_layer is never used
    for (int s = 0; s < z.NS; ++s) {
        const StreamRef& r = c.st[s];
        T2_TRY(gemm(linear(r.memory, z.E, r.aw->wm, z.E, c.P(r.pm), z.A, z.B * r.Tin, z.A, z.E), c.s));
    }
    return 0;
}

__global__ void init_stop_kernel(int32_t* stop_index, int32_t* done, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) stop_index[b] = -1;
    if (b == 0) *done = 0;
}

// ------------------------------------------------------------------------------- backward
// Backward row of a stream (bwd_stream_refs): its gradient outputs and its offsets in the backward workspace
struct BwdStreamRef {
    const t2_lstm_grads* lg; const t2_attention_grads* ag; float *prenet_w1, *prenet_w2;
    const float* d_align; float* d_memory;
    size_t dg, dctx, dq, dv, dpm, carry, carryc, dlconv, dldense, dc, dp2;              // t2_decoder_bwd_layout
};
void bwd_stream_refs(const t2_decoder_grads& g, const t2_decoder_bwd_args& a, const t2_decoder_bwd_layout& BL, BwdStreamRef* st) {
    for (int s = 0; s < 2; ++s) {
        BwdStreamRef& b = st[s];
        b.lg = s ? &g.att_sub : &g.att; b.ag = s ? &g.attn_sub : &g.attn;
        b.prenet_w1 = s ? g.prenet_sub_w1 : g.prenet_w1; b.prenet_w2 = s ? g.prenet_sub_w2 : g.prenet_w2;
        b.d_align = s ? a.d_align_sub : a.d_align; b.d_memory = s ? a.d_memory_sub : a.d_memory;
        b.dg = s ? BL.dgas : BL.dga; b.dctx = s ? BL.dctxs : BL.dctx; b.dq = s ? BL.dqs : BL.dq; b.dv = s ? BL.dvs : BL.dv;
        b.dpm = s ? BL.dpms : BL.dpm; b.carry = s ? BL.carrys : BL.carry; b.carryc = s ? BL.carrycs : BL.carryc;
        b.dlconv = s ? BL.dlconvs : BL.dlconv; b.dldense = s ? BL.dldenses : BL.dldense;
        b.dc = s ? BL.dcas : BL.dca; b.dp2 = s ? BL.dp2s : BL.dp2;
    }
}

// bf16 mode: ONE row-major bf16 copy of dG ([B*T][H4], the dg16 part of a ScratchCarve) serves every product that reads
// dG: as the k-major A operand of a weight gradient (whose dG rows start row0 rows in) or as the K-contiguous A operand of
// an input gradient; either then works in the scratch behind the copy.  on == false: no copy, descriptors pass untouched.
struct Dg16 {
    bool on; __bf16* p; long H4; float* rest; size_t rest_bytes;
    GemmDesc operand(GemmDesc m, long row0, int kmajor) const {
        if (on) { m.A16 = p + row0 * H4; m.lda16 = H4; m.a16_kmajor = kmajor; m.ws = rest; m.ws_bytes = rest_bytes; }
        return m;
    }
    GemmDesc wgrad(GemmDesc m, long row0) const { return operand(m, row0, 1); }
    GemmDesc igrad(GemmDesc m, long row0) const { return operand(m, row0, 0); }
};

// A backward pass in execution: the plan, the caller's arguments, the streams' rows, and what the stages hand on
struct Bwd {
    const t2_dims& d; const t2_decoder_weights& w; const t2_decoder_grads& g; const t2_decoder_bwd_args& a; const BwdPlan p; hipStream_t s;
    const Sizes& z = p.z; const t2_decoder_layout& L = p.L; const t2_decoder_bwd_layout& BL = p.BL;
    const float* W(size_t off) const { return a.ws + off; }
    float* S(size_t off) const { return a.bws + off; }
    long R(int t) const { return (long)t * z.B; }
    hipStream_t sd = nullptr;                        // stream of the decoder-LSTM chain (== s unless overlapped)
    const __bf16* W16(size_t off) const { return reinterpret_cast<const __bf16*>(a.ws + off); }
    __bf16* S16(size_t off) const { return reinterpret_cast<__bf16*>(a.bws + off); }
    // a part of the GEMM scratch (ScratchCarve, decoder_plan.h): its address, a product working in it, a carve's dG copy
    unsigned char* scratch(size_t off) const { return reinterpret_cast<unsigned char*>(a.bws + BL.gemm_ws) + off; }
    GemmDesc in(const ScratchPart& part, GemmDesc m) const { m.ws = reinterpret_cast<float*>(scratch(part.off)); m.ws_bytes = part.bytes; return m; }
    // rows: the dG region whose head holds the bf16 rows a chain stored (BwdPlan::dg_rows_d / dg_rows_a) — they are the copy
    // then, and the carve's own part stays unused so that the products keep their scratch; null: the carve's copy
    Dg16 dg16(const ScratchCarve& cv, int H4, const float* rows = nullptr) const {
        __bf16* p = rows ? reinterpret_cast<__bf16*>(const_cast<float*>(rows)) : reinterpret_cast<__bf16*>(scratch(cv.dg16.off));
        return Dg16{cv.dg16.bytes != 0, p, H4, reinterpret_cast<float*>(scratch(cv.rest.off)), cv.rest.bytes};
    }
    // a cast of dG into its shared copy, or its place where a chain stored the rows (t2_dg_handoff_counts)
    int dg_cast(bool stored, const float* src, const Dg16& dg, long row0, int rows, hipStream_t st) const {
        ++g_dg_cast_counts[stored ? 0 : 1];
        return stored ? 0 : stage_bf16(src + row0 * dg.H4, true, dg.H4, dg.p + row0 * dg.H4, rows, (int)dg.H4, st);
    }
    // a product that reads dG.  stored: the fp32 rows do not exist, so a product that would not take the copy is an error (the
    // plan has asked plan_gemm about each of them: BwdPlan::dg_rows_d / dg_rows_a)
    int dg_gemm(bool stored, const GemmDesc& m, hipStream_t st) const {
        if (stored) {
            GemmPlan gp;
            T2_TRY(gemm_plan(m, &gp));
            T2_REQUIRE(gp.a.src == GemmSrc::caller, "t2_decoder_backward: a product over dG (M=%d N=%d K=%d) does not take the bf16 rows the chain stored", m.M, m.N, m.K);
        }
        return gemm(m, st);
    }
    StreamRef st[2]{}; BwdStreamRef bst[2]{};
    // the reverse-time chains of this pass (bwd_chains): descriptors of the persistent ones, side stream, next free event slot
    ChainBwdDesc cab{}, cbb{};
    Side* side = nullptr; size_t ne = 0;
    Bwd(const Bwd&) = delete;                        // (z, L, BL refer to this object's plan)
};

// C[M,N] = X[M,K] . W[K,N]   (W row-major with leading dimension ldw: "NN")
GemmDesc matmul_nn(const float* X, long ldx, const float* W, long ldw, float* Y, long ldy, int M, int N, int K) {
    return product(X, ldx, 1, W, 1, ldw, Y, ldy, M, N, K);
}
// C[M,N] = G[K,M]^T . X[K,N]   (weight gradients: K = B*T rows)
GemmDesc matmul_tn(const Bwd& c, const float* G, long ldg, const float* X, long ldx, float* Y, long ldy, int M, int N, int K) {
    return c.in(c.p.scratch.whole(), product(G, 1, ldg, X, 1, ldx, Y, ldy, M, N, K));
}

int dec_bwd_step(const Bwd& c, int t) {
    const Sizes& z = c.z;
    const int ks = lstm_bwd_ksplit(4 * z.Hd);
    LstmBwdPointDesc p{};
    p.nstreams = 1; p.B = z.B; p.H = z.Hd; p.seed = c.a.seed; p.first = t == z.T - 1;
    p.drop_p = c.a.training ? c.d.p_dec_dropout : 0.f;
    LstmBwdStream& st = p.st[0];
    st.dh1 = c.S(c.BL.ddout) + c.R(t) * z.WO; st.lddh1 = z.WO;
    st.part = c.S(c.BL.partd); st.nparts = ks; st.part_stride = (long)z.B * z.Hd; st.ldpart = z.Hd; st.part_col = 0;
    st.gates = c.W(c.L.gd) + c.R(t) * 4 * z.Hd; st.ldgates = 4 * z.Hd;
    st.c_new = c.W(c.L.cnd) + c.R(t) * z.Hd; st.ldc_new = z.Hd;
    if (t > 0) { st.c_prev = c.W(c.L.cd) + c.R(t - 1) * z.Hd; st.ldc_prev = z.Hd; }
    st.dc_state = c.S(c.BL.dcd);
    st.dg = c.S(c.BL.dgd) + c.R(t) * 4 * z.Hd; st.lddg = 4 * z.Hd;
    st.site_h = T2_SITE_DEC_H; st.site_c = T2_SITE_DEC_C;
    st.idx_base = (uint32_t)(c.R(t) * z.Hd); st.idx_bstride = (uint32_t)z.Hd;
    if (c.p.use16) st.dg16 = c.S16(c.BL.dg16d);
    hipStream_t sd = c.sd ? c.sd : c.s;
    { ProfScope ps(PK_LSTM_DEC_BWD_PW, sd); T2_TRY(lstm_bwd_pointwise(p, sd)); }
    if (t == 0) return 0;
    LstmBwdGemmDesc g{};
    g.nstreams = 1; g.B = z.B; g.H4 = 4 * z.Hd; g.KS = ks; g.NC = z.Hd;
    g.st[0].dg = st.dg; g.st[0].lddg = st.lddg;
    g.st[0].seg[0] = LstmBwdSeg{c.w.dec.w_hh, (long)z.Hd, z.Hd}; g.st[0].nseg = 1;
    g.st[0].part = c.S(c.BL.partd);
    if (c.p.use16) { g.st[0].dg16 = c.S16(c.BL.dg16d); g.st[0].wt16 = c.W16(c.L.wt16d); }
    else if (c.p.split) { g.st[0].wt16 = c.W16(c.L.wt16d); g.st[0].wt16lo = c.W16(split_lo_d(z, c.L.wt16d)); }
    ProfScope ps(PK_LSTM_DEC_BWD_GEMM, sd);
    int family = 0;
    return counted(lstm_bwd_gemm(g, sd, &family), 3, family);
}

// Persistent BPTT of the decoder LSTM (chain_bwd.hip): shape and pointers, for a chain the plan has on (c.p.chain_b)
ChainBwdDesc chain_b_bwd_desc(const Bwd& c) {
    const Sizes& z = c.z;
    ChainBwdDesc d{};
    shape_into(c.p.chain_b.shape, &d);
    d.T = z.T;
    d.drop_p = c.a.training ? c.d.p_dec_dropout : 0.f; d.seed = c.a.seed;
    ChainBwdStream& st = d.st[0];
    st.wt16 = c.W16(c.L.wt16d); st.ldwt = 4 * z.Hd;
    st.dh1 = c.S(c.BL.ddout); st.lddh1 = z.WO;
    st.gates = c.W(c.L.gd); st.c_new = c.W(c.L.cnd); st.c_out = c.W(c.L.cd);
    st.dg = c.S(c.BL.dgd); st.dc_state = c.S(c.BL.dcd);
    if (c.p.dg_rows_d) st.dg16rows = c.S16(c.BL.dgd);
    st.dbias_part = c.S(c.BL.partd);                                 // (the launch path's K-split scratch: idle when the chain runs) [MT][4Hd]
    st.site_h = T2_SITE_DEC_H; st.site_c = T2_SITE_DEC_C;
    d.err = status_words(c.a.ws, c.L) + CHAIN_STATUS_BWD_LSTM;
    return d;
}

// Persistent BPTT of the attention chain (both attention LSTMs + SMA or LSA attention), for a chain the plan has on (c.p.chain_a)
ChainBwdDesc chain_a_bwd_desc(const Bwd& c) {
    const Sizes& z = c.z;
    const bool lsa = c.d.attention_kind == T2_ATTN_LSA;
    ChainBwdDesc d{};
    shape_into(c.p.chain_a.shape, &d);
    d.T = z.T;
    d.drop_p = c.a.training ? c.d.p_att_dropout : 0.f; d.seed = c.a.seed;
    for (int s = 0; s < z.NS; ++s) {
        ChainBwdStream& st = d.st[s]; const StreamRef& r = c.st[s]; const BwdStreamRef& b = c.bst[s];
        const t2_attention_weights& aw = *r.aw;
        st.wt16 = c.W16(r.wt16); st.ldwt = 4 * z.Ha;
        st.dh1 = c.S(c.BL.ddin) + r.hoff; st.lddh1 = z.WD;
        st.gates = c.W(r.ga); st.c_new = c.W(r.cna); st.c_out = c.W(r.ca);
        st.dg = c.S(b.dg); st.dc_state = c.S(b.dc);
        if (c.p.dg_rows_a) st.dg16rows = c.S16(b.dg);
        st.dbias_part = c.S(c.BL.parta) + (size_t)s * 2 * 4 * z.Ha;     // [MT][4Ha] per stream (the launch path's K-split scratch)
        st.site_h = r.site_h; st.site_c = r.site_c;
        st.dctx_a = c.S(c.BL.ddout) + r.ctx2off; st.lddctx_a = z.WO;
        st.dctx_b = c.S(c.BL.ddin) + r.coff; st.lddctx_b = z.WD;
        st.dalign = b.d_align;
        st.qs = c.W(r.qs); st.pm = c.W(r.pm); st.memory = r.memory;
        st.psel = c.W(r.psel); st.align = r.align;
        st.v = aw.v; st.wq = aw.wq;
        st.dctx_out = c.S(b.dctx); st.dq_out = c.S(b.dq);
        st.dv_acc = c.S(b.dv); st.dpm_acc = c.S(b.dpm);
        if (lsa) {
            st.wcum = c.W(r.wcum); st.loc_conv = aw.loc_conv; st.loc_dense = aw.loc_dense;
            st.usave = c.W(r.usave); st.locsave = c.W(r.locsave);
            st.dconv_acc = c.S(b.dlconv); st.ddense_acc = c.S(b.dldense);
        }
    }
    d.err = status_words(c.a.ws, c.L) + CHAIN_STATUS_BWD_ATT;
    return d;
}

int att_bwd_step(const Bwd& c, int t) {
    const Sizes& z = c.z;
    const int ks = lstm_bwd_ksplit(4 * z.Ha);
    const int NC = z.E + z.Ha;
    const bool first = t == z.T - 1;
    // 1. attention backward (needs dctx(t) incl. the recurrent partials of step t+1)
    AttnBwdDesc ab{};
    ab.nstreams = z.NS; ab.B = z.B; ab.A = z.A; ab.E = z.E; ab.first = first;
    const int abi_kind = c.d.attention_kind;
    ab.kind = kernel_kind(abi_kind); ab.F = c.d.loc_filters; ab.Kc = c.d.loc_kernel;
    ab.nsplit = c.p.nsplit;
    for (int s = 0; s < z.NS; ++s) {
        AttnBwdStream& st = ab.st[s]; const StreamRef& r = c.st[s]; const BwdStreamRef& b = c.bst[s];
        const int Tin = r.Tin;
        st.Tin = Tin;
        st.dctx[0] = c.S(c.BL.ddout) + c.R(t) * z.WO + r.ctx2off; st.lddctx[0] = z.WO;
        st.dctx[1] = c.S(c.BL.ddin) + c.R(t) * z.WD + r.coff; st.lddctx[1] = z.WD;
        st.part = c.S(c.BL.parta) + (size_t)s * ks * z.B * NC; st.nparts = ks; st.part_stride = (long)z.B * NC; st.ldpart = NC; st.part_col = 0;
        if (b.d_align) { st.dalign = b.d_align + (long)t * Tin; st.lddalign = (long)z.T * Tin; }
        st.q = c.W(r.qs) + c.R(t) * z.A; st.ldq = z.A;
        st.pm = c.W(r.pm); st.memory = r.memory;
        const float* al = r.align;
        const long ldA = (long)z.T * Tin;
        if (t > 0) { st.a_prev = al + (long)(t - 1) * Tin; st.lda_prev = ldA; }
        const t2_attention_weights& aw = *r.aw;
        st.v = aw.v;
        if (abi_kind == T2_ATTN_DCA) {
            st.w = al + (long)t * Tin; st.ldw = ldA;
            st.dca = dca_weights(aw);
            st.dca_acc = c.S(b.dldense);
        } else if (abi_kind == T2_ATTN_GMM) {
            st.w = al + (long)t * Tin; st.ldw = ldA;
            st.gmm_w2 = aw.mlp_w2; st.gmm_b2 = aw.mlp_b2;
            st.mu = c.W(r.wcum) + c.R(t) * kGmmPad; st.ldmu = kGmmPad;
            st.mu_carry = c.S(b.carryc);
            st.db2_acc = c.S(b.dlconv);
            st.dw2_acc = c.S(b.dldense);
        } else if (abi_kind == T2_ATTN_SMA) {
            st.p = c.W(r.psel) + (long)t * Tin; st.ldp = ldA;
        } else {
            st.w = al + (long)t * Tin; st.ldw = ldA;
            if (t > 0) { st.wcum_prev = c.W(r.wcum) + (long)(t - 1) * Tin; st.ldwcum_prev = ldA; }
            st.loc_conv = aw.loc_conv; st.loc_dense = aw.loc_dense;
            st.carry_cum = c.S(b.carryc);
            st.dconv_acc = c.S(b.dlconv);
            st.ddense_acc = c.S(b.dldense);
        }
        float* cbuf = c.S(b.carry);
        if (abi_kind == T2_ATTN_SMA) { st.carry = cbuf + (size_t)((t + 1) & 1) * z.B * Tin; st.carry_out = cbuf + (size_t)(t & 1) * z.B * Tin; }
        else st.carry = cbuf;
        st.dctx_out = c.S(b.dctx) + c.R(t) * z.E; st.lddctx_out = z.E;
        st.dq_out = c.S(b.dq) + c.R(t) * 2 * z.A; st.lddq_out = 2 * z.A;
        st.dv_acc = c.S(b.dv);
        st.dpm_acc = c.S(b.dpm);
    }
    { ProfScope ps(PK_ATTN_BWD, c.s); T2_TRY(attention_step_bwd(ab, c.s)); }
    // 2. LSTM pointwise backward
    LstmBwdPointDesc p{};
    p.nstreams = z.NS; p.B = z.B; p.H = z.Ha; p.seed = c.a.seed; p.first = first;
    p.drop_p = c.a.training ? c.d.p_att_dropout : 0.f;
    for (int s = 0; s < z.NS; ++s) {
        LstmBwdStream& st = p.st[s]; const StreamRef& r = c.st[s]; const BwdStreamRef& b = c.bst[s];
        st.dh1 = c.S(c.BL.ddin) + c.R(t) * z.WD + r.hoff; st.lddh1 = z.WD;
        st.part = c.S(c.BL.parta) + (size_t)s * ks * z.B * NC; st.nparts = ks; st.part_stride = (long)z.B * NC; st.ldpart = NC; st.part_col = z.E;
        st.dq = c.S(b.dq) + c.R(t) * 2 * z.A; st.lddq = 2 * z.A; st.dq_parts = ab.nsplit;
        st.wq = r.aw->wq; st.A = z.A;
        st.gates = c.W(r.ga) + c.R(t) * 4 * z.Ha; st.ldgates = 4 * z.Ha;
        st.c_new = c.W(r.cna) + c.R(t) * z.Ha; st.ldc_new = z.Ha;
        if (t > 0) { st.c_prev = c.W(r.ca) + c.R(t - 1) * z.Ha; st.ldc_prev = z.Ha; }
        st.dc_state = c.S(b.dc);
        st.dg = c.S(b.dg) + c.R(t) * 4 * z.Ha; st.lddg = 4 * z.Ha;
        st.site_h = r.site_h; st.site_c = r.site_c;
        st.idx_base = (uint32_t)(c.R(t) * z.Ha); st.idx_bstride = (uint32_t)z.Ha;
        if (c.p.use16) st.dg16 = c.S16(c.BL.dg16a) + (size_t)s * z.B * 4 * z.Ha;
    }
    { ProfScope ps(PK_LSTM_ATT_BWD_PW, c.s); T2_TRY(lstm_bwd_pointwise(p, c.s)); }
    if (t == 0) return 0;
    // 3. recurrent-input gradients of this step: dg(t) . [W_ih[:, P:] | W_hh]  ->  partials for step t-1
    LstmBwdGemmDesc g{};
    g.nstreams = z.NS; g.B = z.B; g.H4 = 4 * z.Ha; g.KS = ks; g.NC = NC;
    for (int s = 0; s < z.NS; ++s) {
        const StreamRef& r = c.st[s];
        const t2_lstm_weights& lw = *r.lw;
        g.st[s].dg = p.st[s].dg; g.st[s].lddg = p.st[s].lddg;
        g.st[s].seg[0] = LstmBwdSeg{lw.w_ih + z.P, (long)(z.P + z.E), z.E};
        g.st[s].seg[1] = LstmBwdSeg{lw.w_hh, (long)z.Ha, z.Ha};
        g.st[s].nseg = 2;
        g.st[s].part = c.S(c.BL.parta) + (size_t)s * ks * z.B * NC;
        if (c.p.use16) { g.st[s].dg16 = c.S16(c.BL.dg16a) + (size_t)s * z.B * 4 * z.Ha; g.st[s].wt16 = c.W16(r.wt16); }
        else if (c.p.split) { g.st[s].wt16 = c.W16(r.wt16); g.st[s].wt16lo = c.W16(split_lo_a(z, r.wt16)); }
    }
    ProfScope ps(PK_LSTM_ATT_BWD_GEMM, c.s);
    int family = 0;
    return counted(lstm_bwd_gemm(g, c.s, &family), 3, family);
}

// An aborted chain must not pass for data: NaN over the pass's outputs when one of the status words of its chains
// (the first c.p.poison_words) is set; nothing for a pass without a chain
int poison_if_aborted(const Dec& c, float* mel_out, float* gate_out) {
    const size_t BT = (size_t)c.z.B * c.z.T;
    if (!c.p.poison_words) return 0;
    hipLaunchKernelGGL(poison_if_aborted_kernel, dim3(64), dim3(256), 0, c.s, status_words(c.ws, c.L), c.p.poison_words, mel_out, BT * c.z.M, gate_out, BT);
    T2_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------- forward, stage by stage
// Phase-1 prologue: everything that does not read the memories
int fwd_prologue(const Dec& c, const float* mels) {
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L;
    const int BT = z.B * z.T;
    if (c.p.use16 || c.p.split) T2_TRY(cast_shadows(c, c.p.split));
    // teacher inputs and both prenets over all frames (model.py:407-413)
    T2_TRY(teacher_inputs(mels, c.P(L.x), z.B, z.M, z.T, c.s));
    for (int s = 0; s < z.NS; ++s) T2_TRY(prenet(c, s, c.P(L.x), z.M, BT, c.P(c.st[s].p1), c.P(c.st[s].p2), z.P, 0, 0));      // rows time-major: (t,b)
    // hoisted input half of both attention LSTMs:  P2 . W_ih[:, :P]^T + b_ih + b_hh
    for (int s = 0; s < z.NS; ++s) {
        const StreamRef& r = c.st[s];
        GemmDesc g = linear(c.P(r.p2), z.P, r.lw->w_ih, z.P + z.E, c.P(r.prea), 4 * z.Ha, BT, 4 * z.Ha, z.P);
        g.bias1 = r.lw->b_ih; g.bias2 = r.lw->b_hh;
        T2_TRY(gemm(c.in(c.p.scratch.whole(), g), c.s));                              // bf16 staging (gemm.hip)
    }
    if (c.p.pre16) T2_TRY(stage_bf16(c.w.dec.w_ih, true, z.WD, reinterpret_cast<__bf16*>(c.scratch(c.p.scratch.w_ih16.off)), 4 * z.Hd, z.WD, c.s));
    return 0;
}

// Two serial chains, overlapped in chunks of steps:
//   A (caller's stream): attention LSTMs + attention — the only truly recurrent chain through the contexts
//   B (side stream):     hoisted input half of the decoder LSTM for the chunk A just finished
//                        ([att_h|ctx|att_h_sub|ctx_sub] . W_ih^T + b), then the decoder-LSTM recurrence over it
// Persistent chains (chain.hip): every step of a chain in ONE launch, weights resident on chip.  Two persistent
// grids must never be in flight together (each needs the whole device to make progress), so with them the chains
// run back to back on the caller's stream: A over all steps, one input GEMM, B over all steps.
int fwd_chains(Dec& c) {
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L;
    const bool chain_a = c.p.chain_a.on, chain_b = c.p.chain_b.on, overlap = c.p.overlap;
    const ChainPlan &pa = c.p.chain_a.plan, &pb = c.p.chain_b.plan;
    const std::vector<int>& bounds = c.p.bounds;
    ChainDesc ca{}, cb{};
    if (chain_a) ca = chain_a_desc(c);
    if (chain_b) cb = chain_b_desc(c);
    saved_tiles_note(c.ws, c.p.saves_tiles);
    T2_TRY(chain_fwd_ws_clear(c.P(L.chain), L.chain_floats, c.p.clear, c.s));
    Side* side = nullptr;
    if (overlap) { T2_TRY(side_get(&side)); c.sd = side->s; }
    size_t ne = 0;
    for (size_t ci = 0; ci + 1 < bounds.size(); ++ci) {
        const int t0 = bounds[ci], t1 = bounds[ci + 1];
        if (chain_a) {
            ca.t0 = t0; ca.t1 = t1;
            ProfScope ps(PK_CHAIN_A_FWD, c.s);
            T2_TRY(chain_fwd(ca, pa, c.P(L.chain), L.chain_floats, c.s));
        } else {
            for (int t = t0; t < t1; ++t) {
                T2_TRY(att_lstm_step(c, t));
                T2_TRY(attention_step(c, t));
            }
        }
        hipStream_t sb = overlap ? side->s : c.s;
        if (overlap) T2_TRY(stream_edge(*side, ne++, c.s, sb));
        GemmDesc g = linear(c.P(L.din) + c.R(t0) * z.WD, z.WD, c.w.dec.w_ih, z.WD, c.P(L.pred) + c.R(t0) * 4 * z.Hd, 4 * z.Hd,
                            (t1 - t0) * z.B, 4 * z.Hd, z.WD);
        g.bias1 = c.w.dec.b_ih; g.bias2 = c.w.dec.b_hh;
        if (c.p.pre16) {
            g.A16 = c.P16(L.din16) + c.R(t0) * z.WD; g.lda16 = z.WD;
            g.B16 = reinterpret_cast<const __bf16*>(c.scratch(c.p.scratch.w_ih16.off)); g.ldb16 = z.WD;
        }
        T2_TRY(gemm(c.in(c.p.scratch.rest, g), sb));                                  // chain A launches no GEMM: the scratch is chain B's
        if (chain_b) {
            cb.t0 = t0; cb.t1 = t1;
            ProfScope ps(PK_CHAIN_B_FWD, sb);
            T2_TRY(chain_fwd(cb, pb, c.P(L.chain), L.chain_floats, sb));
        } else {
            for (int t = t0; t < t1; ++t) T2_TRY(dec_lstm_step(c, t));
        }
    }
    if (overlap) T2_TRY(stream_edge(*side, ne++, side->s, c.s));         // join
    return 0;
}

// Projections over all frames, and the poison of an aborted chain (its status words: CHAIN_STATUS_FWD_ATT and _FWD_LSTM)
int fwd_outputs(const Dec& c, float* mel_out, float* gate_out) {
    const Sizes& z = c.z;
    T2_TRY(projection(c, c.P(c.L.dout), z.WO, z.B * z.T, mel_out, z.M, gate_out, 1, true));
    return poison_if_aborted(c, mel_out, gate_out);
}

// ------------------------------------------------------------------------------- backward, stage by stage
// Incoming gradients arrive in the output layout [B,T,*]; everything inside is time-major.  Then the projections
// (model.py:382-388): dDOUT = d_mel . Wproj + d_gate . Wgate ; weight gradients
int bwd_projections(const Bwd& c) {
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L; const t2_decoder_bwd_layout& BL = c.BL;
    const int BT = z.B * z.T;
    float* cws = c.S(BL.colsum_ws);
    float* dmel = c.S(BL.dmel_t); float* dgate = c.S(BL.dgate_t);
    T2_TRY(permute_rows(c.a.d_mel, dmel, z.B, z.T, z.M, c.s));
    T2_TRY(permute_rows(c.a.d_gate, dgate, z.B, z.T, 1, c.s));
    // the gate term is one multiply per element: it rides on the stores of the mel product as a rank-1 addend (the
    // same bits as the K = 1, beta = 1 product, which is a pass of its own over dDOUT; t2_set_gemm_fold(0) runs that)
    GemmDesc x = matmul_nn(dmel, z.M, c.w.proj_w, z.WO, c.S(BL.ddout), z.WO, BT, z.WO, z.M);
    if (get_gemm_fold()) { x.r1_m = dgate; x.r1_n = c.w.gate_w; }
    T2_TRY(gemm(x, c.s));
    if (!get_gemm_fold()) {
        GemmDesc y = matmul_nn(dgate, 1, c.w.gate_w, z.WO, c.S(BL.ddout), z.WO, BT, z.WO, 1);
        y.beta = 1.f;
        T2_TRY(gemm(y, c.s));
    }
    T2_TRY(gemm(matmul_tn(c, dmel, z.M, c.W(L.dout), z.WO, c.g.proj_w, z.WO, z.M, z.WO, BT), c.s));
    T2_TRY(gemm(matmul_tn(c, dgate, 1, c.W(L.dout), z.WO, c.g.gate_w, z.WO, 1, z.WO, BT), c.s));
    T2_TRY(colsum(dmel, z.M, BT, z.M, c.g.proj_b, nullptr, cws, c.s));
    return colsum(dgate, 1, BT, 1, c.g.gate_b, nullptr, cws, c.s);
}

// Decoder-LSTM weight gradients on stream `sb`.  They need nothing from chain A; where they are issued is the plan's
// (BwdPlan::dec_wgrads): in the step-range loop on chain B's stream, or with a deferred tail on the side stream.
// dec_wgrads_staged: the step-range loop has already filled the shared bf16 copy of dG.
int bwd_dec_lstm_wgrads(const Bwd& c, hipStream_t sb) {
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L;
    const int BT = z.B * z.T;
    const float* DG = c.S(c.BL.dgd);
    const Dg16 dg = c.dg16(c.p.scratch, 4 * z.Hd, c.p.dg_rows_d ? DG : nullptr);
    if (dg.on && !c.p.dec_wgrads_staged) T2_TRY(c.dg_cast(false, DG, dg, 0, BT, sb));
    // dW_ih = dG^T . DIN (bf16 steps: the forward pass left DIN's bf16 shadow) ; recurrent half: dW_hh = dG^T . dec_h(t-1)
    GemmDesc mih = dg.wgrad(matmul_tn(c, DG, 4 * z.Hd, c.W(L.din), z.WD, c.g.dec.w_ih, z.WD, 4 * z.Hd, z.WD, BT), 0);
    if (dg.on && c.p.use16) { mih.B16 = c.W16(L.din16); mih.ldb16 = z.WD; mih.b16_kmajor = 1; }
    T2_TRY(c.dg_gemm(c.p.dg_rows_d, mih, sb));
    // h(t-1) pairs with dG(t): drop the first step's rows of dG and the last step's rows of dec_h
    if (z.T > 1) T2_TRY(c.dg_gemm(c.p.dg_rows_d, dg.wgrad(matmul_tn(c, DG + (long)z.B * 4 * z.Hd, 4 * z.Hd, c.W(L.dout), z.WO, c.g.dec.w_hh, z.Hd, 4 * z.Hd, z.Hd, BT - z.B), z.B), sb));
    else T2_TRY(fill_f32(c.g.dec.w_hh, 0.f, (size_t)4 * z.Hd * z.Hd, sb));
    if (c.p.chain_b.on) {                                             // the chain summed dG over steps and rows: add the row tiles
        T2_TRY(batch_sum(c.cbb.st[0].dbias_part, (z.B + 31) / 32, 4 * z.Hd, c.g.dec.b_ih, sb));
        T2_CHECK_HIP(hipMemcpyAsync(c.g.dec.b_hh, c.g.dec.b_ih, (size_t)4 * z.Hd * sizeof(float), hipMemcpyDeviceToDevice, sb));
    } else T2_TRY(colsum(DG, 4 * z.Hd, BT, 4 * z.Hd, c.g.dec.b_ih, c.g.dec.b_hh, c.S(c.BL.colsum_ws), sb));
    return 0;
}

// Two reverse-time chains, overlapped in chunks of steps (see Side, c_api.hip):
//   B (side stream):     decoder-LSTM BPTT of a chunk, then dDIN rows of the chunk = dG . W_ih
//   A (caller's stream): attention-LSTM + attention BPTT of the chunk B finished
// Persistent chains (chain_bwd.hip): a persistent grid needs the whole device, and two of them must never be in flight
// together, so with the attention chain persistent everything runs on the caller's stream, one step range per chain.
int bwd_chains(Bwd& c) {
    const Sizes& z = c.z; const t2_decoder_bwd_layout& BL = c.BL; const BwdPlan& p = c.p;
    const std::vector<int>& bounds = p.bounds;
    if (p.chain_a.on) c.cab = chain_a_bwd_desc(c);
    if (p.chain_b.on) c.cbb = chain_b_bwd_desc(c);
    if (p.overlap) {
        T2_TRY(side_get(&c.side)); c.sd = c.side->s;
        T2_TRY(stream_edge(*c.side, c.ne++, c.s, c.side->s));           // fork: dDOUT is complete
    }
    const hipStream_t sb = p.overlap ? c.side->s : c.s;
    const float* DGd = c.S(BL.dgd);
    // bf16 mode: W_ih^T ([WD][4Hd], K contiguous) is staged once at the head of the scratch for all dDIN ranges; the shared
    // bf16 copy of dG behind it serves the dDIN product of each range and the two weight-gradient products
    __bf16* const wt16 = reinterpret_cast<__bf16*>(c.scratch(p.scratch.w_ih16.off));
    if (p.pre16) T2_TRY(stage_bf16(c.w.dec.w_ih, false, z.WD, wt16, z.WD, 4 * z.Hd, sb));
    const Dg16 dg = c.dg16(p.scratch, 4 * z.Hd, p.dg_rows_d ? DGd : nullptr);
    for (size_t ci = bounds.size() - 1; ci > 0; --ci) {
        const int t0 = bounds[ci - 1], t1 = bounds[ci];
        if (p.chain_b.on) {
            c.cbb.t0 = t0; c.cbb.t1 = t1;
            ProfScope ps(PK_CHAIN_B_BWD, sb);
            T2_TRY(chain_bwd(c.cbb, p.chain_b.plan, c.S(BL.chain), BL.chain_floats, sb));
        } else {
            for (int t = t1 - 1; t >= t0; --t) T2_TRY(dec_bwd_step(c, t));
        }
        GemmDesc dd = matmul_nn(DGd + c.R(t0) * 4 * z.Hd, 4 * z.Hd, c.w.dec.w_ih, z.WD, c.S(BL.ddin) + c.R(t0) * z.WD, z.WD,
                                (t1 - t0) * z.B, z.WD, 4 * z.Hd);
        dd = c.in(p.ddin_ws, dd);                                         // between fork and join the scratch is chain B's
        if (p.pre16) { dd.B16 = wt16; dd.ldb16 = 4 * z.Hd; }
        if (p.chunk_cast) {                                               // dG of the range cast in front of its dDIN product (or stored by the chain)
            T2_TRY(c.dg_cast(p.dg_rows_d, DGd, dg, c.R(t0), (t1 - t0) * z.B, sb));
            dd = dg.igrad(dd, c.R(t0));
        }
        T2_TRY(c.dg_gemm(p.dg_rows_d, dd, sb));
        if (p.overlap) T2_TRY(stream_edge(*c.side, c.ne++, sb, c.s));
        if (t0 == 0 && p.dec_wgrads == WGRADS_CHAIN_B) T2_TRY(bwd_dec_lstm_wgrads(c, sb));
        if (p.chain_a.on) {
            c.cab.t0 = t0; c.cab.t1 = t1;
            ProfScope ps(PK_CHAIN_A_BWD, c.s);
            T2_TRY(chain_bwd(c.cab, p.chain_a.plan, c.S(BL.chain), BL.chain_floats, c.s));
        } else {
            for (int t = t1 - 1; t >= t0; --t) T2_TRY(att_bwd_step(c, t));
        }
    }
    return 0;
}

// Leaf tail of stream s on stream `ts`: attention-LSTM weights, prenet, attention parameters
int bwd_stream_tail(const Bwd& c, int s, hipStream_t ts) {
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L;
    const StreamRef& r = c.st[s]; const BwdStreamRef& b = c.bst[s];
    const t2_lstm_grads& lg = *b.lg; const t2_attention_grads& ag = *b.ag;
    const int BT = z.B * z.T, hoff = r.hoff, coff = r.coff;
    float* cws = c.S(c.BL.colsum_ws);
    const float* DG = c.S(b.dg);
    const float* DIN = c.W(L.din);
    const float* P1 = c.W(r.p1); const float* P2 = c.W(r.p2);
    float* dP2 = c.S(b.dp2); float* dP1 = c.S(c.BL.dp1);
    const long ldw = z.P + z.E;
    // LSTM weights: W_ih = [prenet part | ctx part], W_hh, biases.  bf16 mode: the shared bf16 copy of dG ([BT][4Ha] at
    // the head of the scratch) is the k-major A operand of the three weight-gradient products (the shifted ones start
    // B rows in) and the K-contiguous A operand of the prenet's input gradient below; the ctx / h operands are read
    // from DIN's bf16 shadow where the forward pass left one
    const Dg16 dg = c.dg16(c.p.tail_scratch, 4 * z.Ha, c.p.dg_rows_a ? DG : nullptr);
    if (dg.on) T2_TRY(c.dg_cast(c.p.dg_rows_a, DG, dg, 0, BT, ts));
    const __bf16* DIN16 = dg.on && c.p.use16 ? c.W16(L.din16) : nullptr;
    auto dw_gemm = [&](const float* G, long row0, const float* X, const __bf16* X16, long ldx, float* Y, long ldy, int N, int K) -> int {
        GemmDesc m = dg.wgrad(matmul_tn(c, G, 4 * z.Ha, X, ldx, Y, ldy, 4 * z.Ha, N, K), row0);
        if (X16) { m.B16 = X16; m.ldb16 = ldx; m.b16_kmajor = 1; }
        return c.dg_gemm(c.p.dg_rows_a, m, ts);
    };
    T2_TRY(dw_gemm(DG, 0, P2, nullptr, z.P, lg.w_ih, ldw, z.P, BT));
    if (z.T > 1) {
        const float* DG1 = DG + (long)z.B * 4 * z.Ha;             // rows of steps 1..T-1 pair with ctx/h of steps 0..T-2
        T2_TRY(dw_gemm(DG1, z.B, DIN + coff, DIN16 ? DIN16 + coff : nullptr, z.WD, lg.w_ih + z.P, ldw, z.E, BT - z.B));
        T2_TRY(dw_gemm(DG1, z.B, DIN + hoff, DIN16 ? DIN16 + hoff : nullptr, z.WD, lg.w_hh, z.Ha, z.Ha, BT - z.B));
    } else {
        GemmDesc zc = matmul_tn(c, DG, 4 * z.Ha, DIN + coff, z.WD, lg.w_ih + z.P, ldw, 4 * z.Ha, z.E, BT);
        zc.alpha = 0.f;
        T2_TRY(gemm(zc, ts));
        T2_TRY(fill_f32(lg.w_hh, 0.f, (size_t)4 * z.Ha * z.Ha, ts));
    }
    if (c.p.chain_a.on) {
        T2_TRY(batch_sum(c.cab.st[s].dbias_part, (z.B + 31) / 32, 4 * z.Ha, lg.b_ih, ts));
        T2_CHECK_HIP(hipMemcpyAsync(lg.b_hh, lg.b_ih, (size_t)4 * z.Ha * sizeof(float), hipMemcpyDeviceToDevice, ts));
    } else T2_TRY(colsum(DG, 4 * z.Ha, BT, 4 * z.Ha, lg.b_ih, lg.b_hh, cws, ts));
    // prenet (model.py:13-24): dP2 = dG . W_ih[:, :P] ; through ReLU+dropout ; layer 2 ; layer 1
    const float scale = c.a.prenet_dropout ? 1.0f / (1.0f - c.d.p_prenet_dropout) : 1.0f;
    const GemmDesc gp = c.in(c.p.tail_scratch.whole(), matmul_nn(DG, 4 * z.Ha, r.lw->w_ih, ldw, dP2, z.P, BT, z.P, 4 * z.Ha));
    T2_TRY(c.dg_gemm(c.p.dg_rows_a, dg.igrad(gp, 0), ts));
    T2_TRY(relu_drop_bwd(dP2, P2, dP2, scale, (size_t)BT * z.P, ts));
    T2_TRY(gemm(matmul_tn(c, dP2, z.P, P1, z.P, b.prenet_w2, z.P, z.P, z.P, BT), ts));
    T2_TRY(gemm(matmul_nn(dP2, z.P, r.prenet_w2, z.P, dP1, z.P, BT, z.P, z.P), ts));
    T2_TRY(relu_drop_bwd(dP1, P1, dP1, scale, (size_t)BT * z.P, ts));
    T2_TRY(gemm(matmul_tn(c, dP1, z.P, c.W(L.x), z.M, b.prenet_w1, z.M, z.P, z.M, BT), ts));
    // attention parameters
    const bool lsa_chain = c.p.lsa_chain;                             // the persistent LSA backward: one partial per position split
    const int nsp = c.p.dq_parts;
    float* DQ = c.S(b.dq);
    if (nsp == 2) T2_TRY(fold_halves(DQ, BT, z.A, ts));               // dq row = partial 0 + partial 1
    T2_TRY(gemm(matmul_tn(c, DQ, 2 * z.A, DIN + hoff, z.WD, ag.wq, z.Ha, z.A, z.Ha, BT), ts));
    const bool dcak = c.d.attention_kind == T2_ATTN_DCA;
    const bool gmm = c.d.attention_kind == T2_ATTN_GMM || dcak;       // both: no processed-memory term
    if (dcak) {
        // W.weight went through the query-projection path above; W.bias = column sums of dq; the rest from the per-item
        // accumulators dv | dbT | dU | dT | dF | dV (attention_dca.hip)
        T2_REQUIRE(ag.mlp_b1 && ag.mlp_w2 && ag.loc_conv && ag.loc_dense && ag.dca_T && ag.dca_bT && ag.v, "t2_decoder_backward: DCA gradient buffers missing");
        T2_TRY(colsum(DQ, 2 * z.A, BT, z.A, ag.mlp_b1, nullptr, cws, ts));
        const size_t na = dca_acc_floats(z.A);
        float* full = reinterpret_cast<float*>(c.scratch(0));        // [na] floats of the split-K scratch (idle here)
        T2_REQUIRE(c.p.dca_acc_fits, "t2_decoder_backward: scratch too small");
        T2_TRY(batch_sum(c.S(b.dldense), z.B, (int)na, full, ts));
        auto cp = [&](float* dst, size_t off, size_t n) { return hipMemcpyAsync(dst, full + off, n * sizeof(float), hipMemcpyDeviceToDevice, ts); };
        size_t off = 0;
        T2_CHECK_HIP(cp(ag.v, off, z.A)); off += z.A;
        T2_CHECK_HIP(cp(ag.dca_bT, off, z.A)); off += z.A;
        T2_CHECK_HIP(cp(ag.loc_dense, off, (size_t)z.A * kDcaC)); off += (size_t)z.A * kDcaC;
        T2_CHECK_HIP(cp(ag.dca_T, off, (size_t)z.A * kDcaC)); off += (size_t)z.A * kDcaC;
        T2_CHECK_HIP(cp(ag.loc_conv, off, kDcaC * kDcaK)); off += kDcaC * kDcaK;
        T2_CHECK_HIP(cp(ag.mlp_w2, off, (size_t)kDcaC * kDcaK * z.A));
    } else if (gmm) {
        // mlp.0.weight was handled as the query projection above; mlp.0.bias = column sums of dq; second layer from
        // the per-item accumulators; memory_layer takes no part in the arithmetic (its gradient is None in the reference)
        T2_REQUIRE(ag.mlp_b1 && ag.mlp_w2 && ag.mlp_b2, "t2_decoder_backward: GMM needs mlp_b1 / mlp_w2 / mlp_b2 gradient buffers");
        T2_TRY(colsum(DQ, 2 * z.A, BT, z.A, ag.mlp_b1, nullptr, cws, ts));
        T2_TRY(batch_sum(c.S(b.dldense), z.B, 3 * kGmmK * z.A, ag.mlp_w2, ts));
        float* b2tmp = cws;                                          // 16 floats of scratch (slot 15 is padding)
        T2_TRY(batch_sum(c.S(b.dlconv), z.B, 16, b2tmp, ts));
        T2_CHECK_HIP(hipMemcpyAsync(ag.mlp_b2, b2tmp, 3 * kGmmK * sizeof(float), hipMemcpyDeviceToDevice, ts));
    } else {
        T2_TRY(batch_sum(c.S(b.dv), nsp * z.B, z.A, ag.v, ts));
    }
    if (c.d.attention_kind == T2_ATTN_LSA) {
        T2_REQUIRE(ag.loc_conv && ag.loc_dense, "t2_decoder_backward: LSA needs loc_conv / loc_dense gradient buffers");
        T2_TRY(batch_sum(c.S(b.dlconv), (lsa_chain ? 2 : 1) * z.B, c.d.loc_filters * 2 * c.d.loc_kernel, ag.loc_conv, ts));
        T2_TRY(batch_sum(c.S(b.dldense), (lsa_chain ? 2 : 1) * z.B, z.A * c.d.loc_filters, ag.loc_dense, ts));
    }
    if (!gmm) T2_TRY(gemm(matmul_tn(c, c.S(b.dpm), z.A, r.memory, z.E, ag.wm, z.E, z.A, z.E, z.B * r.Tin), ts));
    return 0;
}

// d(memory) of stream s = dPM . Wm  +  per item: align^T [Tin x T] . dctx [T x E], on the caller's stream: it feeds the
// encoders.  Neither descriptor carries scratch (nothing staged, no split-K), so these products may run beside a tail
// that works in the GEMM scratch on another stream.
int bwd_stream_dmemory(const Bwd& c, int s) {
    const Sizes& z = c.z;
    const StreamRef& r = c.st[s]; const BwdStreamRef& b = c.bst[s];
    const bool gmm = c.d.attention_kind == T2_ATTN_GMM || c.d.attention_kind == T2_ATTN_DCA;     // no processed-memory term
    if (!gmm) T2_TRY(gemm(matmul_nn(c.S(b.dpm), z.A, r.aw->wm, z.E, b.d_memory, z.E, z.B * r.Tin, z.E, z.A), c.s));
    GemmDesc dm = gemm_desc();
    dm.A = r.align; dm.sam = 1; dm.sak = r.Tin; dm.bsA = (long)z.T * r.Tin;
    dm.B = c.S(b.dctx); dm.sbk = (long)z.B * z.E; dm.sbn = 1; dm.bsB = z.E;     // dctx is [T,B,E]
    dm.C = b.d_memory; dm.ldc = z.E; dm.bsC = (long)r.Tin * z.E;
    dm.M = r.Tin; dm.N = z.E; dm.K = z.T; dm.batch = z.B; dm.beta = gmm ? 0.f : 1.f;
    return gemm(dm, c.s);
}

}  // namespace

extern "C" {

int t2_decoder_layout_query(const t2_dims* dims_in, int B, int T, int Tin, int Tsub, t2_decoder_layout* out) {
    T2_REQUIRE(dims_in && out, "null argument");
    t2_dims d; int max_pos = 0;
    T2_TRY(entry_dims(*dims_in, &d, &max_pos));
    T2_REQUIRE(B >= 1 && B <= 256 && T >= 1 && Tin >= 1 && Tsub >= 1, "bad shape B=%d T=%d Tin=%d Tsub=%d", B, T, Tin, Tsub);
    layout_of(d, sizes_of(d, B, T, Tin, Tsub), pass_env_here(nullptr, false), out);
    return 0;
}

int t2_decoder_forward(const t2_dims* dims_in, const t2_decoder_weights* w, const t2_decoder_fwd_args* a, void* stream) {
    T2_REQUIRE(dims_in && w && a, "null argument");
    t2_dims d; int max_pos = 0;
    T2_TRY(entry_dims(*dims_in, &d, &max_pos));
    T2_REQUIRE(a->B >= 1 && a->B <= 256 && a->T >= 1, "bad shape B=%d T=%d", a->B, a->T);
    T2_REQUIRE((long)a->B * a->T * 4 * d.att_rnn_dim < (1l << 32), "B*T too large for 32-bit RNG indices");
    T2_REQUIRE(a->phase >= 0 && a->phase <= 2, "t2_decoder_forward: phase must be 0, 1 or 2");
    const Sizes z = sizes_of(d, a->B, a->T, a->Tin, a->Tsub);
    PassEnv env = pass_env_here(nullptr, true);
    if (a->phase == 1) env.chain = false;                           // the prologue alone launches no chain: it asks for none (and for no claim)
    Dec c{d, *w, pass_plan_here(env, [&](const PassEnv& e) { return plan_decoder_fwd(d, z, e); }), a->ws, a->training != 0, a->prenet_dropout != 0,
          a->seed, (hipStream_t)stream, max_pos};
    stream_refs(d, *w, c.z, c.L, a->memory, a->memory_sub, a->mem_lengths, a->sub_lengths, a->align, a->align_sub, c.st);
    if (a->phase != 2) {
        T2_TRY(fwd_prologue(c, a->mels));
        if (a->phase == 1) return 0;
    }
    T2_TRY(processed_memory(c));                                    // model.py:258,261
    T2_TRY(fwd_chains(c));
    return fwd_outputs(c, a->mel_out, a->gate_out);
}

int t2_decoder_bwd_layout_query(const t2_dims* dims_in, int B, int T, int Tin, int Tsub, t2_decoder_bwd_layout* out) {
    T2_REQUIRE(dims_in && out, "null argument");
    t2_dims d; int max_pos = 0;
    T2_TRY(entry_dims(*dims_in, &d, &max_pos));
    T2_REQUIRE(B >= 1 && B <= 256 && T >= 1 && Tin >= 1 && Tsub >= 1, "bad shape B=%d T=%d Tin=%d Tsub=%d", B, T, Tin, Tsub);
    bwd_layout_of(d, sizes_of(d, B, T, Tin, Tsub), pass_env_here(nullptr, false), out);
    return 0;
}

int t2_decoder_backward(const t2_dims* dims_in, const t2_decoder_weights* w, const t2_decoder_grads* g,
                        const t2_decoder_bwd_args* a, void* stream) {
    T2_REQUIRE(dims_in && w && g && a, "null argument");
    t2_dims d; int max_pos = 0;
    T2_TRY(entry_dims(*dims_in, &d, &max_pos));
    const Sizes z = sizes_of(d, a->B, a->T, a->Tin, a->Tsub);
    Bwd c{d, *w, *g, *a, pass_plan_here(pass_env_here(a->ws, true), [&](const PassEnv& e) { return plan_decoder_bwd(d, z, e, a->defer_weight_grads != 0); }), (hipStream_t)stream};
    // (no lengths: the masks are in the saved alignments, which this pass only reads)
    stream_refs(d, *w, c.z, c.L, a->memory, a->memory_sub, nullptr, nullptr, const_cast<float*>(a->align), const_cast<float*>(a->align_sub), c.st);
    bwd_stream_refs(*g, *a, c.BL, c.bst);
    T2_TRY(bwd_projections(c));
    T2_TRY(bwd_chains(c));
    // ---- after the chains.  Only d(memory) feeds the caller's next backward nodes (the encoders); every weight gradient
    // is a leaf.  defer_weight_grads: the weight-gradient tail stays on the side stream, un-joined, underneath the
    // encoders' backward — the caller joins with t2_side_join() before it reads a gradient or releases a workspace.
    // The decoder-LSTM weight gradients are there too: queued by the launch path's chain B, or (WGRADS_TAIL: persistent
    // chains, no side stream until here) issued now, ahead of the tails, whose dG copy at the head of the scratch
    // overwrites theirs.  Otherwise: join here, one stream.
    hipStream_t ts = c.s;                                                // stream of the weight-gradient tail
    if (c.p.tail_on_side) {
        if (!c.side) T2_TRY(side_get(&c.side));
        T2_TRY(stream_edge(*c.side, c.ne++, c.s, c.side->s));           // chain A is complete: dG, dq, d(pm) of every step
        ts = c.side->s;
        if (c.p.dec_wgrads == WGRADS_TAIL) T2_TRY(bwd_dec_lstm_wgrads(c, ts));
    } else if (c.p.overlap) {
        T2_TRY(stream_edge(*c.side, c.ne++, c.side->s, c.s));           // join (split-K scratch and colsum scratch are shared)
    }
    for (int s = 0; s < c.z.NS; ++s) T2_TRY(bwd_stream_dmemory(c, s));
    for (int s = 0; s < c.z.NS; ++s) T2_TRY(bwd_stream_tail(c, s, ts));
    ++g_defer_counts[c.p.defer ? 0 : 1];
    return 0;
}

// The plan of a pass for an explicit environment, in the ABI's terms: pure, no device, no claim
static t2_pass_chain pass_chain_info(const ChainUse& u) {
    t2_pass_chain o{};
    o.asked = u.asked; o.on = u.on; o.reason = u.plan.refusal;
    o.reason_text = !u.asked ? "not asked for" : chain_refusal_text(u.plan.refusal);
    if (u.on) { o.instance = u.plan.instance; o.instance_name = chain_instance_name(u.plan.instance); o.grid = u.plan.grid; }
    return o;
}
static t2_scratch_carve carve_info(const ScratchCarve& c) {
    return t2_scratch_carve{c.w_ih16.off, c.w_ih16.bytes, c.dg16.off, c.dg16.bytes, c.rest.off, c.rest.bytes, c.total};
}
static int bounds_info(const std::vector<int>& b, t2_decoder_pass_plan_info* o) {
    T2_REQUIRE(b.size() <= T2_PASS_MAX_BOUNDS, "t2_decoder_pass_plan: %zu step-range bounds", b.size());
    o->nbounds = (int)b.size();
    std::copy(b.begin(), b.end(), o->bounds);
    return 0;
}
int t2_decoder_pass_plan(const t2_dims* dims_in, int pass, int B, int T, int Tin, int Tsub, const t2_pass_env* e, int defer_weight_grads,
                         int poll_every, t2_decoder_pass_plan_info* out) {
    T2_REQUIRE(dims_in && e && out && pass >= T2_PASS_FORWARD && pass <= T2_PASS_INFER, "t2_decoder_pass_plan: null argument or bad pass");
    t2_dims d; int max_pos = 0;
    T2_TRY(entry_dims(*dims_in, &d, &max_pos));
    T2_REQUIRE(B >= 1 && B <= 256 && T >= 1 && Tin >= 1 && Tsub >= 1, "bad shape B=%d T=%d Tin=%d Tsub=%d", B, T, Tin, Tsub);
    const PassEnv env{e->precision, e->split_steps != 0, e->chain != 0, e->chain_bwd != 0, e->overlap != 0,
                      ChainEnv{e->cus, e->claimed != 0, e->no_resident != 0}, e->saved_tiles != 0, e->dg_handoff != 0,
                      e->gemm_staging != 0, gemm_env_here().tiles256};
    const Sizes z = sizes_of(d, B, T, Tin, Tsub);
    t2_decoder_pass_plan_info o{};
    if (pass == T2_PASS_BACKWARD) {
        const BwdPlan p = plan_decoder_bwd(d, z, env, defer_weight_grads != 0);
        o.layout = p.L; o.bwd_layout = p.BL; o.use16 = p.use16; o.split = p.split; o.pre16 = p.pre16;
        o.scratch = carve_info(p.scratch); o.chain_a = pass_chain_info(p.chain_a); o.chain_b = pass_chain_info(p.chain_b);
        o.chained = p.chain_a.on || p.chain_b.on; o.overlap = p.overlap;
        T2_TRY(bounds_info(p.bounds, &o));
        o.defer = p.defer; o.share = p.share; o.chunk_cast = p.chunk_cast; o.ddin_ws_off = p.ddin_ws.off; o.ddin_ws_bytes = p.ddin_ws.bytes;
        o.dec_wgrads = p.dec_wgrads; o.dec_wgrads_staged = p.dec_wgrads_staged; o.tail_on_side = p.tail_on_side;
        o.tail_share = p.tail_share; o.tail_scratch = carve_info(p.tail_scratch);
        o.nsplit = p.nsplit; o.lsa_chain = p.lsa_chain; o.dq_parts = p.dq_parts;
        o.dg_rows_d = p.dg_rows_d; o.dg_rows_a = p.dg_rows_a;
    } else {
        const DecPlan p = pass == T2_PASS_FORWARD ? plan_decoder_fwd(d, z, env) : plan_decoder_infer(d, z, env, poll_every);
        o.layout = p.L; o.use16 = p.use16; o.split = p.split; o.pre16 = p.pre16;
        o.scratch = carve_info(p.scratch); o.chain_a = pass_chain_info(p.chain_a); o.chain_b = pass_chain_info(p.chain_b);
        o.chained = p.chained; o.clear = p.clear; o.saves_tiles = p.saves_tiles; o.overlap = p.overlap;
        T2_TRY(bounds_info(p.bounds, &o));
        o.poison_words = p.poison_words; o.poll = p.poll; o.shadow_floats = p.I.total_floats;
    }
    *out = o;
    return 0;
}

int t2_decoder_infer(const t2_dims* dims_in, const t2_decoder_weights* w, const t2_decoder_infer_args* a, void* stream) {
    T2_REQUIRE(dims_in && w && a && a->steps_run_host, "null argument");
    t2_dims d; int max_pos = 0;
    T2_TRY(entry_dims(*dims_in, &d, &max_pos));
    T2_REQUIRE(a->B >= 1 && a->B <= 256 && a->max_steps >= 1, "bad shape B=%d max_steps=%d", a->B, a->max_steps);
    const Sizes zs = sizes_of(d, a->B, a->max_steps, a->Tin, a->Tsub);
    Dec c{d, *w, pass_plan_here(pass_env_here(nullptr, true), [&](const PassEnv& e) { return plan_decoder_infer(d, zs, e, a->poll_every); }), a->ws, false,
          a->prenet_dropout != 0, a->seed, (hipStream_t)stream, max_pos};
    stream_refs(d, *w, c.z, c.L, a->memory, a->memory_sub, a->mem_lengths, a->sub_lengths, a->align, a->align_sub, c.st);
    const Sizes& z = c.z; const t2_decoder_layout& L = c.L;
    const int T = z.T, poll = c.p.poll;
    const bool chain = c.p.chained;

    hipLaunchKernelGGL(init_stop_kernel, dim3((z.B + 63) / 64), dim3(64), 0, c.s, a->stop_index, a->done_count, z.B);
    T2_LAUNCH_CHECK();
    T2_TRY(processed_memory(c));
    for (int s = 0; s < z.NS; ++s)                                   // W1 [P,M] -> [M,P]: coalesced thread-per-output reads
        T2_TRY(permute_rows(c.st[s].prenet_w1, c.P(L.w1t) + (size_t)s * z.M * z.P, z.P, z.M, 1, c.s));
    if (c.p.use16) {
        const long ldi = z.P + z.E;
        for (int s = 0; s < z.NS; ++s) {
            const t2_lstm_weights& lw = *c.st[s].lw;
            __bf16* f = c.P16(c.I.wa[s]);
            T2_TRY(cast_part(lw.w_hh, z.Ha, f, 0, c.I.Ka, 4 * z.Ha, z.Ha, false, false, c.s));
            T2_TRY(cast_part(lw.w_ih + z.P, ldi, f + z.Ha, 0, c.I.Ka, 4 * z.Ha, z.E, false, false, c.s));
            T2_TRY(cast_part(lw.w_ih, ldi, f + z.Ha + z.E, 0, c.I.Ka, 4 * z.Ha, z.P, false, false, c.s));
        }
        T2_TRY(cast_part(w->dec.w_ih, z.WD, c.P16(c.I.wd), 0, c.I.Kd, 4 * z.Hd, z.WD, false, false, c.s));
        T2_TRY(cast_part(w->dec.w_hh, z.Hd, c.P16(c.I.wd) + z.WD, 0, c.I.Kd, 4 * z.Hd, z.Hd, false, false, c.s));
        // zero recurrent state of step 0: h, ctx (attention rows) and dec_h (decoder rows)
        T2_CHECK_HIP(hipMemsetAsync(c.RowA(0, 0), 0, (size_t)2 * 2 * z.B * c.I.Ka * sizeof(__bf16), c.s));
        T2_CHECK_HIP(hipMemsetAsync(c.RowD(0), 0, (size_t)2 * z.B * c.I.Kd * sizeof(__bf16), c.s));
    }
    // one launch per step for projection + stop rule + the next step's prenets (infer.hip)
    auto tail = [&](int t, bool proj) -> int {
        StepTailDesc d{};
        d.B = z.B; d.M = z.M; d.P = z.P; d.WO = z.WO; d.NS = z.NS; d.t = t;
        d.do_proj = proj; d.do_prenet = proj ? (t + 1 < T) : 1;
        const int tn = proj ? t + 1 : 0;                             // the step whose prenet outputs are produced
        if (proj) {
            d.dout = c.P(L.dout) + c.R(t) * z.WO; d.lddout = z.WO;
            d.proj_w = w->proj_w; d.proj_b = w->proj_b; d.gate_w = w->gate_w; d.gate_b = w->gate_b;
            d.mel_out = a->mel_out + (long)t * z.M; d.ldmel = (long)T * z.M;
            d.gate_out = a->gate_out + t; d.ldgate = T;
            d.thr = a->gate_threshold; d.stop_index = a->stop_index; d.done = a->done_count;
        }
        for (int s = 0; s < z.NS; ++s) {
            const StreamRef& r = c.st[s];
            d.w1t[s] = c.P(L.w1t) + (size_t)s * z.M * z.P; d.w2[s] = r.prenet_w2;
            d.p1[s] = c.P(r.p1) + c.R(tn) * z.P; d.p2[s] = c.P(r.p2) + c.R(tn) * z.P;
            d.site1[s] = r.site_p1; d.site2[s] = r.site_p2;
        }
        d.ldp = z.P;
        if (c.p.use16) { for (int s = 0; s < z.NS; ++s) d.p2_16[s] = c.RowA(tn & 1, s) + z.Ha + z.E; d.ldp16 = c.I.Ka; }
        d.drop_p = c.prenet_dropout ? c.d.p_prenet_dropout : 0.f; d.seed = c.seed;
        d.drop_base = (uint32_t)(c.R(tn) * z.P); d.drop_mstride = (uint32_t)z.P;      // logical [T,B,P]
        return step_tail(d, c.s);
    };
    int steps = 0;
    StopPoll* pl = nullptr;
    T2_TRY(stop_poll_get(&pl));
    ChainDesc cdec{};
    if (chain) cdec = chain_dec_desc(c, *a);
    T2_TRY(chain_fwd_ws_clear(c.P(L.chain), L.chain_floats, c.p.clear, c.s));
    if (!chain) T2_TRY(tail(0, false));                              // prenet of the go frame (model.py:444-450)
    for (int t = 0; t < T; ++t) {
        if (chain) {
            if (t % poll == 0) {                                     // one persistent launch per polling interval
                cdec.t0 = t; cdec.t1 = std::min(T, t + poll);
                ProfScope ps(PK_CHAIN_DEC, c.s);
                T2_TRY(chain_fwd(cdec, c.p.chain_a.plan, c.P(L.chain), L.chain_floats, c.s));
            }
        } else {
            T2_TRY(att_lstm_step(c, t));
            T2_TRY(attention_step(c, t));
            T2_TRY(dec_lstm_step(c, t));
            T2_TRY(tail(t, true));                                   // mel_t, gate_t, stop rule, prenets of step t+1 (:470-471)
        }
        steps = t + 1;
        if (steps % poll == 0 && steps < T) {
            // Stop rule without draining the queue: the counter is copied to pinned memory behind an event; the host reads
            // the copy made TWO polls ago, so it blocks only when it is more than 2*poll steps ahead of the GPU and the
            // GPU always has work queued.  The loop overshoots the last stop by at most 3*poll steps (their frames are
            // past every item's stop index).
            const int k = steps / poll, slot = k & 3;
            T2_CHECK_HIP(hipMemcpyAsync(pl->host + slot, a->done_count, sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
            T2_CHECK_HIP(hipEventRecord(pl->ev[slot], c.s));
            if (k >= 3) {
                const int prev = (k - 2) & 3;
                T2_CHECK_HIP(hipEventSynchronize(pl->ev[prev]));
                if (pl->host[prev] >= z.B) break;
            }
        }
    }
    *a->steps_run_host = steps;
    return poison_if_aborted(c, a->mel_out, a->gate_out);
}

}  // extern "C"
