// WaveGlow's host-side facts, each stated once: which tensor is which (WgTensors, waveglow.h) and how many elements it has, where
// the packed weights, the kept activations and every buffer of the three workspaces lie, what a weight-gradient launch looks like,
// and what the three plans refuse.  Pure host code: nothing here launches, asks a device or allocates on one, so the C ABI's plan
// entries run on a machine without a GPU and tests/test_waveglow_plan_cpu.py pins them.
//
// A size is the end of its carve: every layout is one walk that hands out offsets and the total is where the walk stops
// (packed_bytes, packed_bwd_bytes, saved_bytes, grad_floats, workspace_bytes).  The drivers place their buffers from the same struct.
#include <algorithm>

#include "waveglow.h"

namespace t2 {

// ---- what the launchers and the plans refuse
int wg_check_common(const char* who, int B, long L) {
    T2_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d outside 1..65535", who, B);
    T2_REQUIRE(L >= 1, "%s: L=%ld must be at least 1", who, L);
    T2_REQUIRE(L <= (long)INT32_MAX / 2, "%s: L=%ld exceeds the limit of %d columns per row", who, L, INT32_MAX / 2);
    return 0;
}
int wg_check_nc(const char* who, int nc) {
    T2_REQUIRE(nc >= 8 && nc <= 512 && nc % 8 == 0, "%s: n_channels=%d, must be a multiple of 8 from 8 to 512", who, nc);
    return 0;
}
int wg_check_group(const char* who, int G) {
    T2_REQUIRE(G >= 2 && G <= 8 && G % 2 == 0, "%s: n_group=%d is not even and from 2 to 8", who, G);
    return 0;
}
int wg_check_half(const char* who, int n_half) {
    T2_REQUIRE(n_half >= 1 && n_half <= 4, "%s: n_half=%d outside 1..4", who, n_half);
    return 0;
}
// a tail peels n_peel of its C channels off to z[:, zoff:] (G channels)
int wg_check_peel(const char* who, int n_peel, int C, int zoff, int G) {
    T2_REQUIRE(n_peel >= 0 && n_peel <= C && n_peel != C - 1, "%s: %d of %d channels peeled leave no whole flow", who, n_peel, C);
    T2_REQUIRE(zoff >= 0 && zoff + n_peel <= G && G <= 8, "%s: channels %d..%d of z lie outside its %d", who, zoff, zoff + n_peel, G);
    return 0;
}
int wg_gated_check(int B, int nc, int n_cond, long L, int d) {
    const char* who = "waveglow gated conv";
    T2_TRY_RC(wg_check_common(who, B, L));
    T2_TRY_RC(wg_check_nc(who, nc));
    T2_REQUIRE(n_cond >= 8 && n_cond % 8 == 0, "%s: %d conditioning channels (n_mel_channels * n_group), must be a positive multiple of 8", who, n_cond);
    T2_REQUIRE(d >= 1 && d <= kWgMaxD && (d & (d - 1)) == 0, "%s: dilation %d is not a power of two from 1 to %d", who, d, kWgMaxD);
    return 0;
}

// ---- the packs: floats of one packed operand (slab_gemm.h's order)
size_t wg_packed_floats(int kind, int rows, int k0, int k1) {
    if (kind == kWgGated) return slab_packed_floats(2, rows, k0, 3, k1);
    if (kind == kWgResSkip) return slab_packed_floats(1, rows, k0, 1, 0);
    return slab_packed_floats(1, rows * kWgUpStride, k0, kWgUpTaps, 0);
}
size_t wg_packed_t_floats(int rows, int k0, int taps, int k1) { return slab_packed_floats(1, rows, k0, taps, k1); }

static int rs_rows(const t2_waveglow_config& c, int i) { return i < c.n_layers - 1 ? 2 * c.n_channels : c.n_channels; }      // the last layer has no residual half

size_t wg_tensor_floats(const t2_waveglow_config& c, const WgLayout& lay, int t) {
    const size_t nc = c.n_channels, nl = c.n_layers, n_mel = c.n_mel_channels, n_cond = n_mel * c.n_group;
    const WgTensors& tt = lay.tt;
    if (t == tt.up_w()) return n_mel * n_mel * kWgUpK;
    if (t == tt.up_b()) return n_mel;
    const int k = (t - tt.start_w(0)) / tt.per_flow();
    const size_t ch = lay.flows[k].c;
    if (t == tt.start_w(k)) return nc * (ch / 2);
    if (t == tt.start_b(k)) return nc;
    if (t == tt.cond_w(k)) return 2 * nc * nl * n_cond;
    if (t == tt.cond_b(k)) return 2 * nc * nl;
    if (t < tt.rs_w(k, 0)) return (t - tt.in_w(k, 0)) % 2 == 0 ? 2 * nc * nc * 3 : 2 * nc;
    if (t < tt.end_w(k)) return rs_rows(c, (t - tt.rs_w(k, 0)) / 2) * ((t - tt.rs_w(k, 0)) % 2 == 0 ? nc : 1);
    return t == tt.end_w(k) ? ch * nc : (t == tt.end_b(k) ? ch : ch * ch);
}

int wg_layout(const t2_waveglow_config& c, WgLayout* out) {
    T2_REQUIRE(c.kernel_size == 3, "waveglow: kernel_size=%d, only 3 is implemented", c.kernel_size);
    T2_REQUIRE(c.n_layers >= 1 && c.n_layers <= T2_WAVEGLOW_MAX_LAYERS, "waveglow: n_layers=%d outside 1..%d", c.n_layers, T2_WAVEGLOW_MAX_LAYERS);
    T2_TRY_RC(wg_check_nc("waveglow", c.n_channels));
    T2_TRY_RC(wg_check_group("waveglow", c.n_group));
    T2_REQUIRE(c.n_early_size >= 0 && c.n_early_size % 2 == 0, "waveglow: n_early_size=%d is not even and non-negative", c.n_early_size);
    T2_REQUIRE(c.n_early_every >= 1, "waveglow: n_early_every=%d must be at least 1", c.n_early_every);
    T2_REQUIRE(c.n_flows >= 1 && c.n_flows <= 64, "waveglow: n_flows=%d outside 1..64", c.n_flows);
    T2_REQUIRE(c.n_mel_channels >= 1 && c.n_mel_channels <= 512, "waveglow: n_mel_channels=%d outside 1..512", c.n_mel_channels);
    const int n_cond = c.n_mel_channels * c.n_group, nc = c.n_channels;
    T2_REQUIRE(n_cond % 8 == 0, "waveglow: n_mel_channels * n_group = %d is not a multiple of 8", n_cond);
    WgLayout& L = *out;
    L.tt = WgTensors{c.n_layers, c.n_flows};
    L.flows.clear();
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += round4(n); return o; };
    auto tensor = [&](int t) { return take(wg_tensor_floats(c, L, t)); };          // the tensors that are copied as they are
    L.up_w = take(wg_packed_floats(kWgUpsample, c.n_mel_channels, c.n_mel_channels, 0));
    L.up_b = tensor(L.tt.up_b());
    int ch = c.n_group;
    L.n_planes = 1;
    for (int k = 0; k < c.n_flows; ++k) {
        const bool early = k % c.n_early_every == 0 && k > 0;
        if (early) { ch -= c.n_early_size; ++L.n_planes; }
        T2_REQUIRE(ch >= 2, "waveglow: flow %d is left with %d channels: n_early_size=%d is taken too often from n_group=%d", k, ch, c.n_early_size, c.n_group);
        L.flows.push_back(WgFlow{});
        WgFlow& f = L.flows.back();
        f.early = early; f.c = ch; f.n_half = ch / 2;
        f.start_w = tensor(L.tt.start_w(k)); f.start_b = tensor(L.tt.start_b(k));
        f.cond_b = tensor(L.tt.cond_b(k));
        for (int i = 0; i < c.n_layers; ++i) {
            f.gated[i] = take(wg_packed_floats(kWgGated, nc, nc, n_cond)); f.in_b[i] = tensor(L.tt.in_b(k, i));
            f.rs[i] = take(wg_packed_floats(kWgResSkip, rs_rows(c, i), nc, 0)); f.rs_b[i] = tensor(L.tt.rs_b(k, i));
        }
        f.end_w = tensor(L.tt.end_w(k)); f.end_b = tensor(L.tt.end_b(k)); f.winv = tensor(L.tt.mix(k));
    }
    L.n_remaining = ch; L.total = off;
    return 0;
}

void wg_bwd_layout(const t2_waveglow_config& c, const WgLayout& lay, WgBwdLayout* out) {
    const int nc = c.n_channels, n_cond = c.n_mel_channels * c.n_group, nl = c.n_layers;
    WgBwdLayout& L = *out;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += n; return o; };
    L.flows.assign(c.n_flows, WgBwdFlow{});
    for (WgBwdFlow& bf : L.flows)
        for (int i = 0; i < nl; ++i) {
            bf.conv_t[i] = take(wg_packed_t_floats(nc, 2 * nc, 3, 0));
            bf.cond_t[i] = take(wg_packed_t_floats(n_cond, 2 * nc, 1, 0));
            bf.rs_t[i] = take(wg_packed_t_floats(nc, nc, 1, i < nl - 1 ? nc : 0));
        }
    L.total = off;
    off = 0;                                       // the gradient arena: the tensors as torch lays them out, dense, in pack order
    L.grad.resize(lay.tt.count());
    for (int t = 0; t < lay.tt.count(); ++t) L.grad[t] = take(wg_tensor_floats(c, lay, t));
    L.grad_total = off;
}

WgSaved wg_saved(const t2_waveglow_config& c, const WgLayout& lay, int B, long L) {
    WgSaved sv;
    sv.per = round4((size_t)B * L); sv.nc = c.n_channels; sv.nl = c.n_layers; sv.n_cond = (size_t)c.n_mel_channels * c.n_group;
    size_t off = sv.per * sv.n_cond;
    for (const WgFlow& f : lay.flows) {
        sv.base.push_back(off); sv.ch.push_back(f.c);
        off += sv.per * ((size_t)f.c + sv.nc * (1 + 3 * sv.nl));
    }
    sv.total = off;
    return sv;
}

// ---- the workspaces.  n_sum_blocks: column blocks of the fp64 partial sums of s and z^2, 0 for infer, which has none
static WgFlowWs wg_carve_flow(const t2_waveglow_config& c, int B, long L, size_t n_sum_blocks) {
    const size_t per = round4((size_t)B * L), nc = c.n_channels, G = c.n_group, nf = c.n_flows;
    WgFlowWs w;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += n; return o; };
    auto take_doubles = [&](size_t n) { return take(2 * n); };      // the floats before them are a multiple of 4: 16-byte aligned
    w.spect = take(per * c.n_mel_channels * G); w.x = take(per * nc); w.out = take(per * nc); w.acts = take(per * nc);
    w.bufs[0] = take(per * G); w.bufs[1] = take(per * G);
    w.part_s = take_doubles(nf * B * n_sum_blocks); w.part_z = take_doubles(nf * B * n_sum_blocks);
    w.item = take_doubles(n_sum_blocks ? B : 0); w.sums = take_doubles(n_sum_blocks ? (size_t)B * (nf + 1) : 0);
    w.total = off;
    return w;
}

static WgBwdWs wg_carve_backward(const t2_waveglow_config& c, int B, long L, size_t n_slots) {
    const size_t per = round4((size_t)B * L), nc = c.n_channels, G = c.n_group;
    const size_t gpart = std::max(wg_grad_part_floats(wg_site_conv(c.n_channels, c.n_mel_channels * c.n_group), B, L),
                                  std::max(wg_grad_part_floats(wg_site_res_skip(c.n_channels), B, L), wg_grad_part_floats(wg_site_start(c.n_channels, c.n_group / 2), B, L)));
    WgBwdWs w;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += n; return o; };
    w.dx = take(per * nc); w.d_out = take(per * nc); w.du = take(per * 2 * nc); w.acts = take(per * nc); w.d_spect = take(per * c.n_mel_channels * G);
    w.dbuf[0] = take(per * G); w.dbuf[1] = take(per * G);
    w.gpart = take(gpart);                         // a multiple of 4 floats, so are those before it: the doubles are 16-byte aligned
    w.tpart = take(2 * n_slots * (G * nc + G + G * G));      // doubles: per slot flow 0's dW_end, db_end and a mix, the largest
    w.total = off;
    return w;
}

// ---- the weight gradient
// the shape of one launch: tiles, the columns' segments and the split of the reduction, from the sizes alone
static void wg_grad_shape(WgGrad* p, const WgGradSite& g, int B, long L) {
    int C[kWgGradMaxSeg], n = 0;                   // channels per segment: x at every tap, spect, the row of ones
    for (int j = 0; j < g.taps; ++j) C[n++] = g.x_ch;
    if (g.n_cond) C[n++] = g.n_cond;
    C[n++] = 1;
    p->M = g.M; p->nseg = n; p->B = B; p->L = L;
    p->mtiles = (g.M + kWgGradTile - 1) / kWgGradTile;
    int tiles = 0, col = 0;
    for (int s = 0; s < p->nseg; ++s) {
        p->seg[s].C = C[s]; p->seg[s].tile0 = tiles; p->seg[s].col0 = col;
        tiles += (C[s] + kWgGradTile - 1) / kWgGradTile; col += C[s];
    }
    p->ntiles = tiles; p->Ntot = col;
    p->nchunk = (int)((L + kWgGradTL - 1) / kWgGradTL);
    const long total = (long)B * p->nchunk;
    // at most 1024 workgroups, what 256 CUs hold at once at 4 per CU (34 816 bytes of LDS, 88 registers): one more would wait a whole round
    long nsplit = std::min<long>(std::min<long>(kWgGradMaxSplit, total), std::max<long>(1, 1024 / (p->mtiles * tiles)));
    p->per = (int)((total + nsplit - 1) / nsplit);
    p->nsplit = (int)((total + p->per - 1) / p->per);
}
size_t wg_grad_part_floats(const WgGradSite& g, int B, long L) {
    WgGrad p{};
    wg_grad_shape(&p, g, B, L);
    return round4((size_t)p.nsplit * p.M * p.Ntot);
}
WgGrad wg_grad_desc(const WgGradSite& g, const float* a, int a_rows, const float* x, int x_rows, int d, const float* spect, const WgGradOut& out, int B,
                    long L, float* part) {
    WgGrad p{};
    wg_grad_shape(&p, g, B, L);
    p.a = a; p.Mbuf = a_rows; p.part = part;
    for (int j = 0; j < g.taps; ++j) {
        p.seg[j].src = x; p.seg[j].Cbuf = x_rows; p.seg[j].shift = (j - g.taps / 2) * d;
        p.dst[j] = WgGradDst{out.dw_x + j, nullptr, (long)g.x_ch * g.taps, g.taps};
    }
    if (g.n_cond) { p.seg[g.taps].src = spect; p.seg[g.taps].Cbuf = g.n_cond; p.dst[g.taps] = WgGradDst{out.dw_spect, nullptr, g.n_cond, 1}; }
    p.dst[p.nseg - 1] = WgGradDst{out.db, out.db2, 1, 0};
    // 16-byte loads where L, the shift and the base address are multiples of four floats
    auto quads = [&](const float* q, int shift) { return L % 4 == 0 && shift % 4 == 0 && (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    p.avec = quads(p.a, 0);
    for (int i = 0; i < p.nseg; ++i) p.seg[i].vec = quads(p.seg[i].src, p.seg[i].shift);
    return p;
}

// ---- the three plans
int wg_plan(const t2_waveglow_config& c, const WgLayout& lay, int B, int T, WgInferPlan* out) {
    T2_REQUIRE(B >= 1 && B <= 65535, "waveglow: B=%d outside 1..65535", B);
    T2_REQUIRE(T >= 1, "waveglow: T=%d frames, must be at least 1", T);
    const long cols = (long)T * kWgUpStride / c.n_group;
    T2_REQUIRE(cols >= 1, "waveglow: T=%d frames give no whole group of %d samples", T, c.n_group);
    T2_REQUIRE(cols <= (long)INT32_MAX / 2, "waveglow: L=%ld exceeds the limit of %d columns per row", cols, INT32_MAX / 2);
    out->ws = wg_carve_flow(c, B, cols, 0);
    t2_waveglow_plan_info& info = out->info;
    info.L = cols; info.out_len = cols * c.n_group;
    info.n_remaining_channels = lay.n_remaining; info.n_noise_planes = lay.n_planes; info.n_tensors = lay.tt.count(); info.time_tile = kVocTT;
    info.workspace_bytes = out->ws.total * sizeof(float);
    info.packed_bytes = lay.total * sizeof(float);
    return 0;
}

int wg_forward_plan(const t2_waveglow_config& c, int B, int T, long N, WgForwardPlan* out) {
    WgLayout& lay = out->lay;
    T2_TRY_RC(wg_layout(c, &lay));
    T2_REQUIRE(B >= 1 && B <= 65535, "waveglow forward: B=%d outside 1..65535", B);
    T2_REQUIRE(T >= 1, "waveglow forward: T=%d frames, must be at least 1", T);
    T2_REQUIRE(N >= c.n_group, "waveglow forward: n_samples=%ld is shorter than one group of n_group=%d", N, c.n_group);
    const long have = ((long)T - 1) * kWgUpStride + kWgUpK;
    T2_REQUIRE(N <= have, "waveglow forward: n_samples=%ld, but the upsampled mel of T=%d frames has only %ld (glow.py:216)", N, T, have);
    const long cols = N / c.n_group;
    T2_REQUIRE(cols <= (long)INT32_MAX / 2, "waveglow forward: L=%ld exceeds the limit of %d columns per row", cols, INT32_MAX / 2);
    t2_waveglow_forward_info& info = out->info;
    info.L = cols; info.n_log_s_rows = 0; info.n_tensors = lay.tt.count();
    for (const WgFlow& f : lay.flows) info.n_log_s_rows += f.n_half;
    info.n_blocks = (cols + 255) / 256;
    info.n_partials = (size_t)2 * c.n_flows * B * info.n_blocks;
    out->ws = wg_carve_flow(c, B, cols, info.n_blocks);
    info.workspace_bytes = out->ws.total * sizeof(float);
    info.packed_bytes = lay.total * sizeof(float);
    return 0;
}

int wg_backward_plan(const t2_waveglow_config& c, int B, int T, long N, WgBackwardPlan* out) {
    WgForwardPlan fp;
    T2_TRY_RC(wg_forward_plan(c, B, T, N, &fp));
    out->lay = std::move(fp.lay);
    wg_bwd_layout(c, out->lay, &out->bl);
    t2_waveglow_backward_info& info = out->info;
    info.L = fp.info.L; info.n_tensors = out->lay.tt.count();
    info.n_slots = (size_t)B * fp.info.n_blocks * 4;
    out->sv = wg_saved(c, out->lay, B, info.L);
    out->ws = wg_carve_backward(c, B, info.L, info.n_slots);
    info.saved_bytes = out->sv.total * sizeof(float);
    info.grad_floats = out->bl.grad_total;
    info.packed_bwd_bytes = out->bl.total * sizeof(float);
    info.workspace_bytes = out->ws.total * sizeof(float);
    return 0;
}

}  // namespace t2
