// The plans of the three decoder passes (decoder_plan.h): pure host arithmetic, pinned by tests/test_decoder_plan_cpu.py on
// the decisions recorded before this file existed (tests/golden/decoder_pass_plans.jsonl).  Every rule of a pass is stated
// here once; where two rules look alike and differ (the two pre16 conditions, the decode loop's use16), both are kept and named.
#include <algorithm>
#include <cstdint>

#include "decoder_plan.h"

namespace t2 {

namespace {

size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }
size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }
bool attends_by_content(const t2_dims& d) { return d.attention_kind == T2_ATTN_SMA || d.attention_kind == T2_ATTN_LSA; }   // the kinds the chains cover
int chain_kind(const t2_dims& d) { return d.attention_kind == T2_ATTN_SMA ? CHAIN_SMA : CHAIN_LSA; }

// bf16 copy of the decoder LSTM's W_ih (or its transpose): [4Hd][WD]
size_t w_ih16_bytes(const Sizes& z) { return al256((size_t)4 * z.Hd * z.WD * sizeof(__bf16)); }
// row-major bf16 copy of a dG buffer: [B*T][H4]
size_t dg16_bytes(const Sizes& z, int H4) { return al256((size_t)H4 * z.B * z.T * sizeof(__bf16)); }

ChainUse ask(bool asked, const ChainShape& shape, ChainPlan (*pure)(const ChainShape&, const ChainEnv&), const ChainEnv& env) {
    ChainUse u{};
    u.asked = asked; u.shape = shape;
    if (asked) { u.plan = pure(shape, env); u.on = u.plan.refusal == CHAIN_OK; }
    return u;
}

// Shapes of the chains of a pass: the fields their plans read (chain_plan.h), as the descriptors of the pass carry them
ChainShape att_chain_shape(const t2_dims& d, const Sizes& z, size_t ws_floats) {
    ChainShape s{};
    s.kind = chain_kind(d); s.NS = z.NS; s.B = z.B; s.H = z.Ha; s.E = z.E; s.A = z.A; s.F = d.loc_filters; s.Kc = d.loc_kernel;
    s.Tin[0] = z.Tin; s.Tin[1] = z.NS > 1 ? z.Tsub : 0; s.ws_bytes = ws_floats * sizeof(float);
    return s;
}
ChainShape lstm_chain_shape(const Sizes& z, size_t ws_floats) {
    ChainShape s{};
    s.kind = CHAIN_LSTM; s.NS = 1; s.B = z.B; s.H = z.Hd; s.ws_bytes = ws_floats * sizeof(float);
    return s;
}

// Does a product take the shared bf16 copy of dG ([rows][H4], row-major) as its A operand?  The descriptor is the one the drivers
// build (decoder.hip: bwd_chains, bwd_dec_lstm_wgrads, bwd_stream_tail), with stand-in addresses — plan_gemm reads their
// alignment only — and the scratch behind the copy; the answer is plan_gemm's, so the rule is stated there and nowhere else.
//   weight gradient dW[H4][N] = dG^T . X, K = rows: the copy is its k-major A operand; X[rows][ldx] fp32, or (x16) its bf16 shadow
//   input gradient  dX[rows][N] = dG . W, K = H4: the copy is its K-contiguous A operand; W fp32 [H4][ldx], or (x16) W^T as bf16 [N][H4]
bool takes_dg_copy(const PassEnv& env, bool wgrad, int rows, int H4, int N, long ldx, bool x16, const ScratchPart& ws) {
    if (rows <= 0) return true;                                       // (no such product)
    const float* at = reinterpret_cast<const float*>((uintptr_t)4096);
    GemmDesc m = gemm_desc();
    m.A = at; m.B = at; m.C = const_cast<float*>(at); m.ldc = N;
    m.A16 = reinterpret_cast<const __bf16*>(at); m.lda16 = H4; m.a16_kmajor = wgrad;
    m.sbn = 1; m.sbk = ldx; m.N = N;
    if (wgrad) { m.sam = 1; m.sak = H4; m.M = H4; m.K = rows; }
    else { m.sam = H4; m.sak = 1; m.M = rows; m.K = H4; }
    if (x16) { m.B16 = reinterpret_cast<const __bf16*>(at); m.ldb16 = wgrad ? ldx : H4; m.b16_kmajor = wgrad; }
    m.ws = const_cast<float*>(at); m.ws_bytes = ws.bytes;
    return plan_gemm(m, GemmEnv{env.precision, env.gemm_staging, env.gemm_tiles256, 0.0}).a.src == GemmSrc::caller;
}

}  // namespace

Sizes sizes_of(const t2_dims& d, int B, int T, int Tin, int Tsub) {
    Sizes z{};
    z.B = B; z.T = T; z.Tin = Tin; z.Tsub = Tsub;
    z.M = d.n_mel; z.P = d.prenet_dim; z.E = d.enc_dim; z.Ha = d.att_rnn_dim; z.Hd = d.dec_rnn_dim; z.A = d.att_dim;
    z.NS = d.n_streams == 1 ? 1 : 2;
    z.WD = z.NS * (z.Ha + z.E);
    z.WO = z.Hd + z.NS * z.E;
    return z;
}

InferShadows infer_shadows(const Sizes& z, size_t base) {
    InferShadows m{};
    m.Ka = z.Ha + z.E + z.P; m.Kd = z.WD + z.Hd;
    size_t off = base;
    auto take = [&](size_t elems) { size_t o = off; off += align4((elems + 1) / 2); return o; };
    m.wa[0] = take((size_t)4 * z.Ha * m.Ka); m.wa[1] = take((size_t)4 * z.Ha * m.Ka);
    m.wd = take((size_t)4 * z.Hd * m.Kd);
    m.rows_a = take((size_t)2 * 2 * z.B * m.Ka); m.rows_d = take((size_t)2 * z.B * m.Kd);
    m.total_floats = off - base;
    return m;
}

void layout_of(const t2_dims& d, const Sizes& z, const PassEnv& env, t2_decoder_layout* L) {
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += align4(n); return o; };
    const size_t BT = (size_t)z.B * z.T;
    L->x = take(BT * z.M);
    L->p1 = take(BT * z.P); L->p2 = take(BT * z.P); L->p1s = take(BT * z.P); L->p2s = take(BT * z.P);
    L->pm = take((size_t)z.B * z.Tin * z.A); L->pms = take((size_t)z.B * z.Tsub * z.A);
    L->prea = take(BT * 4 * z.Ha); L->preas = take(BT * 4 * z.Ha);
    L->ga = take(BT * 4 * z.Ha); L->gas = take(BT * 4 * z.Ha);
    L->cna = take(BT * z.Ha); L->cnas = take(BT * z.Ha); L->ca = take(BT * z.Ha); L->cas = take(BT * z.Ha);
    L->din = take(BT * z.WD);
    L->psel = take(BT * z.Tin); L->psels = take(BT * z.Tsub);
    L->wcum = take(BT * std::max(z.Tin, kGmmPad)); L->wcums = take(BT * std::max(z.Tsub, kGmmPad));   // LSA cumulative weights / GMM means
    L->pred = take(BT * 4 * z.Hd); L->gd = take(BT * 4 * z.Hd);
    L->cnd = take(BT * z.Hd); L->cd = take(BT * z.Hd);
    L->dout = take(BT * z.WO);
    L->qs = take(BT * z.A); L->qss = take(BT * z.A);
    L->qpart = take((size_t)2 * (z.Ha / 8) * z.B * z.A);
    L->w1t = take((size_t)2 * z.M * z.P);
    // bf16 shadow arena: teacher-forced passes keep [W_hh | W_ih[:,P:]] (+ transposes) per attention stream and W_hh of
    // the decoder LSTM; the decode loop keeps whole-cell shadows and ping-pong input rows (InferShadows) in the same space
    const size_t na = (size_t)4 * z.Ha * (z.Ha + z.E) / 2, nd = (size_t)4 * z.Hd * z.Hd / 2;      // bf16 pairs per float
    // split-bf16 steps (mode 2 with t2_set_split_steps on; decided by (mode, switch) alone, whatever the batch size): a lo
    // plane of the same size right behind each of the six shadows; the fields name the hi planes (split_lo_a / split_lo_d
    // give the lo plane)
    const size_t planes = env.precision == 2 && env.split_steps ? 2 : 1;
    const size_t train16 = planes * (4 * na + 2 * nd), infer16 = infer_shadows(z, 0).total_floats;
    const size_t arena = take(train16 > infer16 ? train16 : infer16);
    L->w16a = arena; L->w16as = L->w16a + planes * na; L->w16d = L->w16as + planes * na;
    L->wt16a = L->w16d + planes * nd; L->wt16as = L->wt16a + planes * na; L->wt16d = L->wt16as + planes * na;
    L->din16 = take(BT * z.WD / 2 + 4); L->dh16 = take(BT * z.Hd / 2 + 4);
    L->gemm_ws_floats = (size_t)16 << 20;                     // 64 MiB of split-K scratch
    // split-bf16 mode: the hoisted LSTM-input products stage both operands as three bf16 terms (6 bytes per element; the
    // decoder LSTM's takes up to all B*T rows when the chains are not overlapped), in front of the split-K partials
    if (env.precision == 2) {
        const size_t wd = std::max(z.WD, z.P), h4 = (size_t)4 * std::max(z.Ha, z.Hd);
        L->gemm_ws_floats += align4((6 * (BT + h4) * wd + 1024) / sizeof(float));
    }
    L->gemm_ws = take(L->gemm_ws_floats);
    // exchange space of the persistent chain kernels (chain.hip), the pass's status words at its head
    L->chain_floats = chain_fwd_ws_floats(z.NS, z.B, z.Ha, z.E, z.P, z.Hd, z.A);
    L->chain = take(L->chain_floats);
    // LSA: tanh tile and location features of every step, written by the forward chain for the backward chain (which then
    // repeats neither the location conv nor the tile: 1.3 GB + 0.33 GB per stream at B = 64, T = 400 — HBM is what this part has)
    const bool lsa = d.attention_kind == T2_ATTN_LSA;
    L->usave = take(lsa ? BT * align4(z.Tin) * z.A : 0); L->usaves = take(lsa && z.NS > 1 ? BT * align4(z.Tsub) * z.A : 0);   // [T][B][A][Tin rounded up to 4]
    L->locsave = take(lsa ? BT * z.Tin * d.loc_filters : 0); L->locsaves = take(lsa && z.NS > 1 ? BT * z.Tsub * d.loc_filters : 0);
    L->total_floats = off;
}

void bwd_layout_of(const t2_dims& d, const Sizes& z, const PassEnv& env, t2_decoder_bwd_layout* L) {
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += align4(n); return o; };
    const size_t BT = (size_t)z.B * z.T;
    const int ksd = lstm_bwd_ksplit(4 * z.Hd), ksa = lstm_bwd_ksplit(4 * z.Ha);
    L->ddout = take(BT * z.WO); L->ddin = take(BT * z.WD);
    L->dgd = take(BT * 4 * z.Hd); L->dga = take(BT * 4 * z.Ha); L->dgas = take(BT * 4 * z.Ha);
    L->dctx = take(BT * z.E); L->dctxs = take(BT * z.E);
    L->dq = take(BT * 2 * z.A); L->dqs = take(BT * 2 * z.A);              // rows [2][A]: one partial per position split
    L->dv = take((size_t)2 * z.B * z.A); L->dvs = take((size_t)2 * z.B * z.A);
    L->dpm = take((size_t)z.B * z.Tin * z.A); L->dpms = take((size_t)z.B * z.Tsub * z.A);
    L->carry = take((size_t)2 * z.B * z.Tin); L->carrys = take((size_t)2 * z.B * z.Tsub);   // ping-pong by step parity
    const bool lsa = d.attention_kind == T2_ATTN_LSA;          // LSA: cumulative-weight carry + per-item location-layer gradients
    const bool gmm = d.attention_kind == T2_ATTN_GMM;          // GMM: mean carry [B,8] + per-item db2 [B,16] / dW2 [B,3K*A]
    const bool dca = d.attention_kind == T2_ATTN_DCA;          // DCA: all per-item accumulators in one block (dldense)
    // (LSA: two rows per item — the persistent backward chain keeps one accumulator per position split)
    const size_t ncv = lsa ? (size_t)2 * z.B * d.loc_filters * 2 * d.loc_kernel : gmm ? (size_t)z.B * 16 : 0;
    const size_t nds = lsa ? (size_t)2 * z.B * z.A * d.loc_filters : gmm ? (size_t)z.B * 3 * kGmmK * z.A : dca ? (size_t)z.B * dca_acc_floats(z.A) : 0;
    L->carryc = take(lsa ? (size_t)z.B * z.Tin : gmm ? (size_t)z.B * kGmmPad : 0); L->carrycs = take(lsa ? (size_t)z.B * z.Tsub : gmm ? (size_t)z.B * kGmmPad : 0);
    L->dlconv = take(ncv); L->dlconvs = take(ncv); L->dldense = take(nds); L->dldenses = take(nds);
    L->dcd = take((size_t)z.B * z.Hd); L->dca = take((size_t)z.B * z.Ha); L->dcas = take((size_t)z.B * z.Ha);
    L->partd = take((size_t)ksd * z.B * z.Hd);
    L->parta = take((size_t)2 * ksa * z.B * (z.E + z.Ha));
    L->dp2 = take(BT * z.P); L->dp2s = take(BT * z.P); L->dp1 = take(BT * z.P);
    L->dmel_t = take(BT * z.M); L->dgate_t = take(BT);
    L->dg16a = take((size_t)2 * z.B * 4 * z.Ha / 2 + 4); L->dg16d = take((size_t)z.B * 4 * z.Hd / 2 + 4);
    L->colsum_ws = take((size_t)64 * 4 * (z.Ha > z.Hd ? z.Ha : z.Hd));
    L->gemm_ws_floats = (size_t)192 << 20;                    // 768 MiB: split-K partials + bf16 operand staging (gemm.hip)
    // split-bf16 mode: the largest weight-gradient product (dW_ih of an LSTM: K = B*T rows of dG [4H] and of its input
    // [WD]) stages 6 bytes per operand element; 256 MiB stay for its split-K partials
    if (env.precision == 2) {
        const size_t h4 = (size_t)4 * std::max(z.Ha, z.Hd), need = 6 * BT * (h4 + z.WD) + ((size_t)256 << 20);
        L->gemm_ws_floats = std::max(L->gemm_ws_floats, align4(need / sizeof(float)));
    }
    L->gemm_ws = take(L->gemm_ws_floats);
    // exchange space of the persistent backward chains (chain_bwd.hip); their status words are in the forward workspace
    L->chain_floats = chain_bwd_ws_floats(lsa ? CHAIN_LSA : CHAIN_SMA, z.NS, z.B, z.Ha, z.E, z.A, d.loc_filters, d.loc_kernel, z.Hd);
    L->chain = take(L->chain_floats);
    L->total_floats = off;
}

bool step_shapes_ok(const Sizes& z) {
    return z.B <= 128 && (z.Ha + z.E) % 256 == 0 && z.Hd % 256 == 0 && (4 * z.Ha) % 2048 == 0 && (4 * z.Hd) % 2048 == 0;
}
bool use_bf16_steps(const Sizes& z, const PassEnv& env) { return env.precision == 1 && step_shapes_ok(z); }
bool use_split_steps(const Sizes& z, const PassEnv& env) { return env.precision == 2 && env.split_steps && step_shapes_ok(z); }
StepMode teacher_step_mode(const Sizes& z, const PassEnv& env) { return StepMode{use_bf16_steps(z, env), use_split_steps(z, env)}; }
bool infer_use16(const Sizes& z, const InferShadows& I, const PassEnv& env) {
    return env.precision == 1 && z.B <= 128 && I.Ka % 256 == 0 && I.Kd % 256 == 0;
}

int attn_bwd_nsplit(const t2_dims& d, const Sizes& z) {
    return (d.attention_kind == T2_ATTN_SMA && z.B * z.NS <= 128 && std::min(z.Tin, z.NS == 2 ? z.Tsub : z.Tin) >= 16) ? 2 : 1;
}

std::vector<int> chunk_bounds(int T, bool overlap) {
    std::vector<int> b{0};
    if (!overlap) { b.push_back(T); return b; }
    const int CH = std::max(16, (T + 7) / 8);
    std::vector<int> tail;
    int rem = T;
    for (int s = 16; s < CH && rem - s >= CH; s *= 2) { tail.push_back(s); rem -= s; }
    const int n = std::max(1, rem / CH);
    for (int i = 1; i < n; ++i) {
        const int e = (int)((long)rem * i / n) & ~1;
        if (e > b.back()) b.push_back(e);
    }
    b.push_back(rem);
    for (auto it = tail.rbegin(); it != tail.rend(); ++it) b.push_back(b.back() + *it);
    return b;
}

// Two serial chains per teacher-forced forward pass: A (attention LSTMs + attention) and B (the decoder LSTM over the hoisted
// input half).  Persistent chains need the whole device each, so with one of them the chains run back to back on the caller's
// stream, one step range; otherwise B follows A range by range on the side stream.
DecPlan plan_decoder_fwd(const t2_dims& d, const Sizes& z, const PassEnv& env) {
    DecPlan p{};
    p.teacher = true; p.z = z;
    layout_of(d, z, env, &p.L);
    const StepMode m = teacher_step_mode(z, env);
    p.use16 = m.use16; p.split = m.split;
    // bf16 steps keep a bf16 shadow of every DIN row (din16): with one bf16 copy of W_ih at the head of the scratch the
    // decoder-LSTM input GEMMs of the chains read both operands as bf16 and stage nothing.  (The forward rule: the scratch
    // holds more than the copy.  The backward pass asks for more than twice its copy, plan_decoder_bwd.)
    const size_t total = p.L.gemm_ws_floats * sizeof(float), wb = w_ih16_bytes(z);
    p.pre16 = p.use16 && (4 * z.Hd) % 64 == 0 && z.WD % 64 == 0 && total > wb;
    p.scratch.total = total;
    p.scratch.w_ih16 = ScratchPart{0, p.pre16 ? wb : 0};
    p.scratch.dg16 = ScratchPart{p.scratch.w_ih16.bytes, 0};
    p.scratch.rest = ScratchPart{p.scratch.w_ih16.bytes, total - p.scratch.w_ih16.bytes};
    // the attention chain: bf16 steps, a content-based kind.  Its shape carries the pass's P and Hd (exchange-space layout)
    ChainShape sa = att_chain_shape(d, z, p.L.chain_floats);
    sa.P = z.P; sa.Hd = z.Hd;
    p.chain_a = ask(env.chain && p.use16 && attends_by_content(d), sa, plan_chain_fwd, env.chain_env);
    // (a pass whose attention-chain tiling has no kernel instance takes the per-step launches as a whole, the decoder LSTM
    //  included: its bits are then those of a pass with the chains off)
    ChainShape sb = lstm_chain_shape(z, p.L.chain_floats);
    sb.Tin[0] = 4;
    p.chain_b = ask(env.chain && p.use16 && !(p.chain_a.asked && p.chain_a.plan.refusal == CHAIN_REFUSE_NO_INSTANCE), sb, plan_chain_fwd, env.chain_env);
    p.chained = p.chain_a.on || p.chain_b.on;
    p.saves_tiles = p.chain_a.on && sa.kind == CHAIN_LSA;
    // status words always (0 = OK / not used); the tagged exchange buffers (zero state of step -1) when a chain runs
    p.clear = p.chained ? CHAIN_WS_TEACHER : CHAIN_WS_STATUS;
    p.overlap = env.overlap && z.T >= 32 && !p.chained;
    p.bounds = chunk_bounds(z.T, p.overlap);
    p.poison_words = p.chained ? CHAIN_STATUS_FWD_LSTM + 1 : 0;
    return p;
}

// The decode loop: per-step launches, or every phase of a step inside one persistent launch per polling interval
DecPlan plan_decoder_infer(const t2_dims& d, const Sizes& z, const PassEnv& env, int poll_every) {
    DecPlan p{};
    p.teacher = false; p.z = z;
    layout_of(d, z, env, &p.L);
    p.I = infer_shadows(z, p.L.w16a);
    p.use16 = infer_use16(z, p.I, env);
    p.scratch.total = p.L.gemm_ws_floats * sizeof(float);
    p.scratch.rest = p.scratch.whole();
    ChainShape s = att_chain_shape(d, z, p.L.chain_floats);
    s.dec = 1; s.P = z.P; s.M = z.M; s.Hd = z.Hd; s.Tin[1] = z.Tsub;
    p.chain_a = ask(env.chain && p.use16 && z.NS == 2 && attends_by_content(d), s, plan_chain_fwd, env.chain_env);
    p.chained = p.chain_a.on;
    // status words always; with the chain its whole exchange space (zero state of step -1: h, ctx, dec_h, go-frame prenet = 0)
    p.clear = p.chained ? CHAIN_WS_DECODE : CHAIN_WS_STATUS;
    p.bounds = chunk_bounds(z.T, false);
    p.poison_words = p.chained ? CHAIN_STATUS_FWD_ATT + 1 : 0;
    // one persistent launch per polling interval: 32 steps amortise its start-up
    p.poll = poll_every > 0 ? poll_every : p.chained ? 32 : 16;
    return p;
}

// Two reverse-time chains: B (decoder-LSTM BPTT of a step range, then the range's dDIN rows = dG . W_ih) and A (attention-LSTM
// and attention BPTT of the range B finished).  With the attention chain persistent everything runs on the caller's stream,
// one step range per chain; otherwise B runs ahead on the side stream.
BwdPlan plan_decoder_bwd(const t2_dims& d, const Sizes& z, const PassEnv& env, bool defer_weight_grads) {
    BwdPlan p{};
    p.z = z;
    layout_of(d, z, env, &p.L);
    bwd_layout_of(d, z, env, &p.BL);
    const StepMode m = teacher_step_mode(z, env);
    p.use16 = m.use16; p.split = m.split;
    p.defer = env.overlap && z.T >= 32 && defer_weight_grads;
    p.nsplit = attn_bwd_nsplit(d, z);
    // the attention chain: SMA where the launch path splits the positions in two as well, LSA after a forward chain (a
    // workspace filled by the per-step launches holds no tanh tile: the chain's plan refuses it)
    const bool lsa = d.attention_kind == T2_ATTN_LSA;
    ChainShape sa = att_chain_shape(d, z, p.BL.chain_floats);
    sa.saved_tiles = lsa && env.saved_tiles;
    p.chain_a = ask(env.chain && env.chain_bwd && p.use16 && (lsa || (d.attention_kind == T2_ATTN_SMA && p.nsplit == 2)), sa, plan_chain_bwd, env.chain_env);
    // (the missing tiles are looked at first, before the shape: whatever else the chain's plan would say, this is why it cannot run)
    if (p.chain_a.asked && lsa && !env.saved_tiles) { p.chain_a.on = false; p.chain_a.plan = ChainPlan{}; p.chain_a.plan.refusal = CHAIN_REFUSE_NO_SAVED_TILES; }
    p.overlap = env.overlap && z.T >= 32 && !p.chain_a.on;
    p.bounds = chunk_bounds(z.T, p.overlap);
    // (next to per-step launches of the attention chain a persistent decoder-LSTM grid only takes CUs away from them:
    //  measured 24.8 -> 26.3 ms; it runs when the attention chain is persistent too)
    p.chain_b = ask(p.chain_a.on, lstm_chain_shape(z, p.BL.chain_floats), plan_chain_bwd, env.chain_env);

    // ---- chain phase of the scratch.  bf16 mode: W_ih^T ([WD][4Hd], K contiguous) is staged once at its head for all dDIN
    // ranges.  (The backward rule: the scratch holds more than twice the copy; plan_decoder_fwd asks for more than once.)
    const size_t total = p.BL.gemm_ws_floats * sizeof(float), wb = w_ih16_bytes(z), BT = (size_t)z.B * z.T;
    p.pre16 = env.precision == 1 && (4 * z.Hd) % 64 == 0 && z.WD % 64 == 0 && total > 2 * wb;
    // the shared bf16 copy of dG ([BT][4Hd], behind W_ih^T) serves both of its consumers: the dDIN product of each range
    // and the two weight-gradient products; it must leave room for a staged copy of DIN behind it
    const size_t dg_off = p.pre16 ? wb : 0, dgb = dg16_bytes(z, 4 * z.Hd);
    p.share = env.precision == 1 && BT % 64 == 0 && z.B % 8 == 0 && (4 * z.Hd) % 128 == 0 && z.T > 1 &&
              total >= dg_off + dgb + ((size_t)z.WD * BT * sizeof(__bf16) + 256);
    p.chunk_cast = p.share && p.pre16;
    for (size_t ci = 1; ci < p.bounds.size(); ++ci) if (((p.bounds[ci] - p.bounds[ci - 1]) * z.B) % 64 != 0) p.chunk_cast = false;
    p.scratch.total = total;
    p.scratch.w_ih16 = ScratchPart{0, dg_off};
    p.scratch.dg16 = ScratchPart{dg_off, p.share ? dgb : 0};
    p.scratch.rest = ScratchPart{dg_off + p.scratch.dg16.bytes, total - dg_off - p.scratch.dg16.bytes};
    // a range's dDIN product reads the dG copy when the ranges are cast one by one; otherwise it works in everything behind
    // W_ih^T, and the copy is made there afterwards, in front of the weight gradients
    p.ddin_ws = p.chunk_cast ? p.scratch.rest : ScratchPart{dg_off, total - dg_off};
    // Decoder-LSTM weight gradients: on chain B's stream once its recurrence is done, underneath the rest of chain A (whose
    // launches leave most CUs idle); next to a persistent chain A there is nothing to run under, and with a deferred tail they
    // join it on the side stream (chain A writes nothing into the scratch, so the dG copy is still there)
    p.dec_wgrads = p.chain_a.on && p.defer ? WGRADS_TAIL : WGRADS_CHAIN_B;
    p.dec_wgrads_staged = p.chunk_cast;
    p.tail_on_side = p.defer;

    // ---- tail phase of the scratch: the shared bf16 copy of a stream's dG ([BT][4Ha]) at its head, room for as much behind
    const size_t dga = dg16_bytes(z, 4 * z.Ha);
    p.tail_share = env.precision == 1 && BT % 64 == 0 && z.B % 8 == 0 && (4 * z.Ha) % 128 == 0 && z.T > 1 && total >= 2 * dga;
    p.tail_scratch.total = total;
    p.tail_scratch.dg16 = ScratchPart{0, p.tail_share ? dga : 0};
    p.tail_scratch.rest = ScratchPart{p.tail_scratch.dg16.bytes, total - p.tail_scratch.dg16.bytes};
    p.lsa_chain = p.chain_a.on && lsa;                              // the persistent LSA backward: one partial per position split
    p.dq_parts = p.lsa_chain ? 2 : p.nsplit;
    p.dca_acc_fits = d.attention_kind != T2_ATTN_DCA || dca_acc_floats(z.A) * sizeof(float) <= total;
    // ---- dG hand-off: where a persistent chain produces dG and its only reader would be the cast into the shared copy (the
    // bias gradients are the chain's own), the chain stores the bf16 rows itself, at the head of the stream's fp32 dG region
    // (half of it: no product's scratch moves, so every product keeps its kernel, split-K factor and K chunks).  Not in the
    // carve: chain A runs while the decoder LSTM's copy is still needed, and the two tails share one carve.  Every other case
    // (no shared copy, a chain off or refused, per-step launches, fp32 and split-bf16 modes) keeps the fp32 rows and the casts
    // ... and only where no product is left that reads the fp32 rows: each must take the copy (a product that is no whole number
    // of tiles, or a shifted one whose K = BT - B is no multiple of 64, ignores it and converts the fp32 operand itself)
    const int H4d = 4 * z.Hd, H4a = 4 * z.Ha, shifted = (int)BT - z.B;
    bool all_d = true, all_a = true;
    for (size_t ci = 1; ci < p.bounds.size(); ++ci)                   // dDIN of each range, then dW_ih and dW_hh
        all_d = all_d && takes_dg_copy(env, false, (p.bounds[ci] - p.bounds[ci - 1]) * z.B, H4d, z.WD, z.WD, p.pre16, p.scratch.rest);
    all_d = all_d && takes_dg_copy(env, true, (int)BT, H4d, z.WD, z.WD, p.use16, p.scratch.rest) &&
            takes_dg_copy(env, true, shifted, H4d, z.Hd, z.WO, false, p.scratch.rest);
    all_a = takes_dg_copy(env, true, (int)BT, H4a, z.P, z.P, false, p.tail_scratch.rest) &&
            takes_dg_copy(env, true, shifted, H4a, z.E, z.WD, p.use16, p.tail_scratch.rest) &&
            takes_dg_copy(env, true, shifted, H4a, z.Ha, z.WD, p.use16, p.tail_scratch.rest) &&
            takes_dg_copy(env, false, (int)BT, H4a, z.P, z.P + z.E, false, p.tail_scratch.rest);
    p.dg_rows_d = env.dg_handoff && p.chain_b.on && p.chunk_cast && all_d;
    p.dg_rows_a = env.dg_handoff && p.chain_a.on && p.tail_share && all_a;
    return p;
}

}  // namespace t2
