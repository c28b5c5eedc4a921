// What the persistent chain kernels (chain.hip, chain_bwd.hip, chain_enc.hip) and their host-side plan (chain_plan.hip) both
// derive from a shape: workgroup geometry, item sizes and the LDS carves.  Plain arithmetic on both sides, no device code.
#pragma once
#include "kernels.h"

namespace t2 {
namespace chain {

constexpr int NTH = 512, NWV = 8;
constexpr int PPR = 40;                    // LDS pitch of a 32-wide partial tile row (conflict-free fixed-order reads)
constexpr int NSH = kCntShards;            // shards of an arrival counter
constexpr int CNT_LINE = 32;               // unsigned words per 128-byte line
constexpr int CNT_STRIDE = NSH * CNT_LINE; // words per (sharded) arrival counter

// ---- forward chains and decode loop (chain.hip) ---------------------------------------------------------------------------
struct Geo {                                // derived on both sides from the descriptor
    int MT, NRG, NUG, nL, nA, KT; unsigned xs_bytes;
};
__host__ __device__ inline Geo geo_of(const ChainDesc& d, int UT, int RT) {
    Geo g;
    g.MT = (d.B + 31) / 32; g.NRG = (g.MT + RT - 1) / RT; g.NUG = d.H / (8 * UT);
    g.nL = d.NS * g.NUG * g.NRG; g.nA = d.kind == CHAIN_LSTM ? 0 : d.NS * d.B * d.CS;
    g.KT = (d.H + (d.kind == CHAIN_LSTM ? 0 : d.E) + (d.dec ? d.P : 0)) / 16;
    g.xs_bytes = (unsigned)g.KT * g.MT * 1024u;
    return g;
}

// LDS carve (floats).  Persistent part first, then a scratch area shared by the two phases.
struct Lds { int ab, v, ap, cum, q, e, an, cs, pm, mem, convw, dense, loc, wpad, pa, lsp, scratch, total; };
__host__ __device__ inline Lds lds_of(const ChainDesc& d, int UT, int RT, int Tin, int Jp, int Jm) {
    Lds m; int o = 0;
    auto take = [&](int n) { int r = o; o += (n + 3) & ~3; return r; };
    const int Tp = (Tin + 3) & ~3, EC = d.kind == CHAIN_LSTM ? 0 : d.E / d.CS;
    m.ab = take(4);
    if (d.kind != CHAIN_LSTM) {
        m.v = take(d.A + 4); m.ap = take(Tp + 4); m.cum = take(Tp + 4); m.q = take(d.A); m.e = take(Tp + 4); m.an = take(Tp + 4); m.cs = take(EC);
        m.pm = take(Jp * (d.kind == CHAIN_LSA ? d.A + 1 : d.A)); m.mem = take(Jm * EC / 2);    // (LSA reads pm position-major: odd pitch)
        // decode loop: the projection / prenet workgroups keep their weight fragments (64 KB) in this area instead of the
        // attention rows, however short the memories are
        if (d.dec && o - m.pm < 16384) take(16384 - (o - m.pm));
    } else { m.v = m.ap = m.cum = m.q = m.e = m.an = m.cs = m.pm = m.mem = o; }
    m.convw = m.dense = o;
    // location layer weights, resident, each as a bf16 hi/lo pair: conv taps [2][F][2 KP + 8] (KP = Kc rounded up to 8, zero taps
    // behind Kc), dense layer [2][A][F + 8]
    if (d.kind == CHAIN_LSA) { m.convw = take(d.F * (2 * ((d.Kc + 7) & ~7) + 8)); m.dense = take(d.A * (d.F + 8)); }
    const int lpart = NWV * 32 * PPR, lhs = RT * 32 * (UT * 8 + 4), lq = d.kind == CHAIN_LSTM ? 0 : RT * 32 * (d.A + 4);
    const int lphase = (lpart > lq ? lpart : lq) + lhs;
    int aphase = d.kind == CHAIN_LSTM ? 0 : 16 * d.A + NWV * EC;
    m.loc = m.wpad = m.pa = m.lsp = 0;
    if (d.kind == CHAIN_LSA) {                               // per-step location features behind the reduction buffers
        const int TwP = (Tin + d.Kc - 1 + 8 + 3) & ~3;
        m.loc = aphase;                                           // (the fp32 copy of the features is gone: the bf16 pair below is what is read)
        m.wpad = aphase; aphase += 2 * TwP;
        m.pa = aphase; aphase += (d.A / 32) * ((Tin + 3) & ~3);   // energy partials of the channel tiles [A/32][Tp]
        m.lsp = aphase; aphase += (Tin * (d.F + 8) + 3) & ~3;     // the features again as a bf16 hi/lo pair [2][Tin][F + 8]
    }
    m.scratch = take(lphase > aphase ? lphase : aphase);
    m.loc += m.scratch; m.wpad += m.scratch; m.pa += m.scratch; m.lsp += m.scratch;
    m.total = o;
    return m;
}

// ---- backward chains (chain_bwd.hip) ---------------------------------------------------------------------------------------
constexpr int GNC = 32;          // output columns of a G item
constexpr int GKP = 8;           // K parts
constexpr int PU = 16;           // hidden units of a P item
constexpr int ANC = 64;          // output columns of a G item (attention chain)
constexpr int AKP = 4;           // K parts = the four gate blocks

struct BwdLds { int ab, v, q, dctx, g, de, ps, ap, carry, dva, dqo, wq, pm, dpm, mem, cc, convw, dloc, wpad, ut, loc, red, TwP, scratch, total; };
__host__ __device__ inline BwdLds bwd_lds_of(int A, int E, int Tc, int MT, int kind = CHAIN_SMA, int F = 0, int Kc = 1) {
    BwdLds m; int o = 0;
    auto take = [&](int n) { int r = o; o += (n + 3) & ~3; return r; };
    const bool lsa = kind == CHAIN_LSA;
    const int pad = (Kc - 1) / 2;
    m.ab = take(4); m.v = take(A); m.q = take(A); m.dctx = take(E);
    m.g = take(Tc + 8); m.de = take(Tc + 8); m.ps = take(Tc + 8); m.ap = take(Tc + 8); m.carry = take(Tc + 8);
    m.dva = take(A); m.dqo = take(A);
    m.wq = take(PU * (A + 8));                                 // Wq slice of the P item as a bf16 hi/lo pair [2][PU][A + 8]
    m.pm = take(lsa ? 0 : Tc * A); m.dpm = take(Tc * A); m.mem = take((Tc + 1) * E / 2);
    // LSA: carried gradient on the cumulative weights, conv weights, dloc of the last step with `pad` halo rows on both
    // sides (pitch F + 1, column F stays zero), [w_prev; cum_prev] of two steps (ping-pong) with the same halos
    m.TwP = (Tc + 2 * pad + 8 + 3) & ~3;                    // (+8: the conv product's K is padded to a multiple of 16 with zero weights)
    m.cc = take(lsa ? Tc + 8 : 0); m.convw = take(lsa ? F * ((2 * Kc + 15) & ~15) : 0); m.dloc = take(lsa ? (Tc + 2 * pad) * (F + 1) : 0);
    m.wpad = take(lsa ? 4 * m.TwP : 0);
    // scratch shared by the phases; LSA's A phase: tanh / dpre tile [Tc][A + 4], location features [Tc][F + 1], reduction rows
    // (the tile's room first holds Q = dloc . Wc^T, [Tc + 2 pad][65], of the carried-gradient step)
    const int nut = Tc * (A + 4), nq = (Tc + 2 * pad) * 65;
    m.ut = 0; m.loc = ((nut > nq ? nut : nq) + 3) & ~3; m.red = m.loc + ((Tc * (F + 1) + 3) & ~3);
    const int sg = NWV * 32 * PPR, sp = 32 * (A + 4) + 4 * 32 * (PU + 4) + 4 * 32 * (PU + 1), sa = lsa ? m.red + 2 * NWV * A : 2 * 32 * A;
    m.scratch = take(sg > sp ? (sg > sa ? sg : sa) : (sp > sa ? sp : sa));
    m.total = o;
    return m;
}

// ---- encoder BiLSTM chains (chain_enc.hip) ---------------------------------------------------------------------------------
constexpr int EKW = 16;                    // K elements per lane: H = 16 * EKW = 256
constexpr int EH = 16 * EKW;
constexpr int EGKP = 4;                    // backward: K parts of the dx product = the four gate blocks
constexpr int EPU = 16;                    // backward: hidden units of a P item

}  // namespace chain
}  // namespace t2
