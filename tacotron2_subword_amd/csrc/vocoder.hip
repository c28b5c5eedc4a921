// HiFi-GAN generator (Kong et al. 2020), inference: mel spectrogram -> waveform.  Replaces the reference's
// hifigan_infer/hifigan_model.py: Generator.forward (:100-116), ResBlock1.forward (:35-42), ResBlock2.forward (:63-68).
//
// Activations are [B][C][L] with time contiguous, as torch lays them out; nothing is transposed.  Arithmetic is exact fp32
// on the matrix cores (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain), whatever t2_set_precision says.
//
// One kernel serves the dilated Conv1d and the ConvTranspose1d.  Both are the GEMM  Y[co][q] = sum_{ci,j} W[co][ci,j] *
// act(X[ci][q + off_j])  with M = Cout, N = time and K = Cin * taps:
//   Conv1d (stride 1, "same" padding pad = (k*d - d)/2):   off_j = j*d - pad, one output per q;
//   ConvTranspose1d (stride u, kernel k = 2u, padding u/2), polyphase: output sample u*q + r reads only the taps
//     j = (r + pad) % u + m*u (m = 0, 1) at input q + (r + pad)/u - m, so phase r is a two-tap GEMM of its own whose
//     outputs land u apart.  No zero-stuffed input, no atomics: every output element is written once.
// The tiling, the slab staging (here with the leaky ReLU applied), the MFMA step, the epilogue's walk, the launcher and the weight
// pack are slab_gemm.h's.  This file adds the walk over chunks and taps, the polyphase term (phase from blockIdx.y, coff0 =
// (phase + pad)/u + 1, cstep = -1, output offset q*ostride + phase) and the epilogue: bias, optional residual, optional
// accumulate-into-destination, scale.  Cout = 8 wastes three quarters of its 32-channel tile: accepted.  The order of every sum
// is fixed: same bits from run to run and for an item alone or in a batch.  Element offsets are 64-bit throughout.
//
// Per-item lengths (a padded batch of mels of different lengths): with a `frames` pointer item b's rows at a stage hold
// clamp(frames[b], 0, T) * factor inputs, factor being the stage's cumulative upsampling.  That length bounds the slab staging
// (zeros from it on, as for a row that ends there), the epilogue's walk (so the residual and accumulate reads and the stores)
// and conv_post, which writes zeros behind it.  Grid, tiles and the order of every sum stay, so an item has the bits of its
// run alone; a workgroup whose tile lies behind its item's end returns before its first barrier.  The count is only read
// in the kernels, clamped: no value of it moves a load or a store out of a row.
#include <algorithm>
#include <vector>

#include "slab_gemm.h"
#include "vocoder.h"

namespace t2 {

struct VocGemm {
    const float* x; const float* wp; const float* bias; const float* res; float* y;
    int Cin, Cout, Lin;                           // outputs per phase = Lin; the output row has Lin * ostride elements
    int taps, d, pad, u, transposed;              // transposed: taps = 2, phases = ostride = u
    int halo_lo;                                  // slab column c holds input t0 + c - halo_lo
    int mtiles, nchunks, ostride;
    float slope, scale; int accumulate;
    const int32_t* frames; int T, factor;         // nullable: item b's rows hold clamp(frames[b], 0, T) * factor inputs, Lin = T * factor
};

// the inputs item b's rows hold; a count from the device is clamped, so that no value of it moves a load or a store out of the row
__device__ __forceinline__ int voc_row_len(const int32_t* frames, int b, int T, int factor, int full) {
    if (!frames) return full;
    const int f = frames[b];
    return (f < 0 ? 0 : (f > T ? T : f)) * factor;
}

template <int WM>
__global__ void __launch_bounds__(WM * 128) voc_gemm_kernel(VocGemm p) {
    __shared__ float slab[kSlabCK * kVocStride];
    const int wm = (threadIdx.x >> 6) % WM;
    const int mblocks = (p.mtiles + WM - 1) / WM;
    const int phase = blockIdx.y / mblocks, mt = (blockIdx.y % mblocks) * WM + wm;
    const bool active = mt < p.mtiles;             // uniform over the wave
    const int b = blockIdx.z;
    // slab column of tap j for output q = t0 + c: c + coff0 + j*cstep
    const int coff0 = p.transposed ? (phase + p.pad) / p.u + 1 : 0, cstep = p.transposed ? -1 : p.d;
    const f32x4* wp = reinterpret_cast<const f32x4*>(p.wp) + (size_t)(phase * p.mtiles + (active ? mt : 0)) * p.nchunks * p.taps * 128;
    const float* xb = p.x + (size_t)b * p.Cin * p.Lin;
    const int lane = threadIdx.x & 63, wt = (threadIdx.x >> 6) / WM, tc = wt * 64 + (lane & 31), hk = lane >> 5;
    const long t0 = (long)blockIdx.x * kVocTT;
    const int N = voc_row_len(p.frames, b, p.T, p.factor, p.Lin);
    if (t0 >= N) return;                           // the tile lies behind the item's end: uniform over the workgroup, before any barrier
    const float slope = p.slope;
    f32x16 acc[1][2] = {{f32x16{0}, f32x16{0}}};
    for (int c = 0; c < p.nchunks; ++c) {
        if (c) __syncthreads();                    // every wave is done reading the previous slab
        slab_stage_ld<kVocStride, WM * 2>(slab, xb, p.Cin, c * kSlabCK, p.Lin, N, t0, p.halo_lo, [slope](float v) { return v > 0.f ? v : v * slope; });
        __syncthreads();
        if (active)
            for (int j = 0; j < p.taps; ++j)
                slab_mfma_step<kVocStride, 1>(slab + hk * kVocStride + tc + coff0 + j * cstep, wp + ((size_t)c * p.taps + j) * 128 + lane, acc);
    }
    if (!active) return;
    const size_t lout = (size_t)p.Lin * p.ostride;
    slab_walk<WM, 1>(acc, mt, p.Cout, N, [=](int co, long q, const float (&a)[1]) {
        const size_t o = ((size_t)b * p.Cout + co) * lout + (size_t)q * p.ostride + phase;
        float v = a[0];
        if (p.bias) v += p.bias[co];
        if (p.res) v += p.res[o];
        if (p.accumulate) v = p.y[o] + v;
        p.y[o] = v * p.scale;
    });
}

// conv_post: y[b,0,t] = tanh(bias + sum_ci sum_j w[ci][j] * lrelu(x[b,ci,t+j-3])), ci then j ascending, one fused multiply-add
// per term.  Cout = 1 makes it a reduction: one thread per output sample, the weights in LDS, loads coalesced along time.
__global__ void __launch_bounds__(256) voc_post_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ audio, float* __restrict__ pre, int C, long L, float slope,
                                                      const int32_t* __restrict__ frames, int T, int factor, int32_t* __restrict__ sample_lengths) {
    extern __shared__ float ws[];
    const int b = blockIdx.y;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    // with per-item frame counts the row ends at N: tanh inside, exact zeros behind it, in audio and in pre alike
    const long N = voc_row_len(frames, b, T, factor, (int)L);
    if (sample_lengths && blockIdx.x == 0 && threadIdx.x == 0) sample_lengths[b] = (int32_t)N;
    if ((long)blockIdx.x * 256 < N) {              // uniform over the workgroup: a block wholly behind the end only writes zeros
        for (int i = threadIdx.x; i < C * kVocPostK; i += 256) ws[i] = w[i];
        __syncthreads();
    }
    if (t >= L) return;
    if (t >= N) {
        const size_t o = (size_t)b * L + t;
        if (pre) pre[o] = 0.f;
        audio[o] = 0.f;
        return;
    }
    const float* xb = x + (size_t)b * C * L;
    float acc = 0.f;
    for (int ci = 0; ci < C; ++ci) {
        const float* xr = xb + (size_t)ci * L;
#pragma unroll
        for (int j = 0; j < kVocPostK; ++j) {
            const long tt = t + j - kVocPostK / 2;
            float v = (tt >= 0 && tt < N) ? xr[tt] : 0.f;
            v = v > 0.f ? v : v * slope;
            acc = fmaf(ws[ci * kVocPostK + j], v, acc);
        }
    }
    acc += bias[0];
    const size_t o = (size_t)b * L + t;
    if (pre) pre[o] = acc;
    audio[o] = tanhf(acc);
}

// ------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------
int voc_shape_check(const char* who, int Cin, int Cout, int k, int d, int u) {
    T2_REQUIRE(Cin >= 8 && Cin <= 512 && Cin % 8 == 0, "%s: %d input channels, must be a multiple of 8 from 8 to 512", who, Cin);
    T2_REQUIRE(Cout >= 8 && Cout <= 512 && Cout % 8 == 0, "%s: %d output channels, must be a multiple of 8 from 8 to 512", who, Cout);
    if (u == 0) {
        T2_REQUIRE(k == 3 || k == 5 || k == 7 || k == 11, "%s: kernel size %d is not one of 3, 5, 7, 11", who, k);
        T2_REQUIRE(d == 1 || d == 2 || d == 3 || d == 5 || d == 6 || d == 12, "%s: dilation %d is not one of 1, 2, 3, 5, 6, 12", who, d);
        static_assert(5 * 12 <= kVocMaxPad, "the largest kernel at the largest dilation fits the slab");
    } else {
        T2_REQUIRE((k - u) % 2 == 0, "%s: kernel %d minus stride %d is odd: the padding (k - u)/2 would not give u outputs per input", who, k, u);
        T2_REQUIRE(u >= 2 && u <= 16 && k == 2 * u, "%s: kernel %d with stride %d is not implemented (kernel = 2 * stride, stride 2..16)", who, k, u);
    }
    return 0;
}

static size_t voc_packed_floats(int Cin, int Cout, int k, int u) {
    return u ? (size_t)u * slab_packed_floats(1, Cout, Cin, 2, 0) : slab_packed_floats(1, Cout, Cin, k, 0);
}

// packed[phase][mtile][chunk][tap]...: Conv1d [Cout][Cin][k] is one phase; ConvTranspose1d [Cin][Cout][k] one pack per phase r (taps (r + pad) % u + j*u)
static int voc_pack(const float* w, float* packed, int Cin, int Cout, int k, int u, hipStream_t s) {   // w in torch layout
    T2_TRY_RC(voc_shape_check("vocoder pack", Cin, Cout, k, 1, u));
    T2_REQUIRE(w && packed, "vocoder pack: null pointer");
    SlabPack p{};
    p.gates = 1; p.rows = Cout; p.split = 1; p.s0.w = w; p.s0.K = Cin; p.out = packed;
    if (!u) {
        p.s0.taps = k; p.s0.rhi = (long)Cin * k; p.s0.ks = k; p.s0.ts = 1;
        return slab_pack(p, s);
    }
    p.s0.taps = 2; p.s0.rhi = k; p.s0.ks = (long)Cout * k; p.s0.ts = u;
    for (int r = 0; r < u; ++r, p.out += slab_packed_floats(1, Cout, Cin, 2, 0)) {
        p.s0.base = (r + (k - u) / 2) % u;
        T2_TRY_RC(slab_pack(p, s));
    }
    return 0;
}

int voc_conv(const VocConv& a, hipStream_t s) {
    const char* who = a.u ? "vocoder conv_transpose1d" : "vocoder conv1d";
    T2_TRY_RC(voc_shape_check(who, a.Cin, a.Cout, a.k, a.u ? 1 : a.d, a.u));
    T2_REQUIRE(a.B >= 1 && a.B <= 65535, "%s: B=%d outside 1..65535", who, a.B);
    T2_REQUIRE(a.L >= 1, "%s: L=%ld must be at least 1", who, a.L);
    T2_REQUIRE(a.L <= (long)INT32_MAX / 2, "%s: L=%ld exceeds the limit of %d samples per row", who, a.L, INT32_MAX / 2);
    T2_REQUIRE(a.x && a.packed && a.y, "%s: null pointer", who);
    T2_REQUIRE(!(a.u && (a.res || a.accumulate)), "%s: residual / accumulate are Conv1d fusions", who);
    T2_REQUIRE(!a.frames || (a.factor >= 1 && a.T >= 1 && (long)a.T * a.factor == a.L), "%s: per-item counts of up to T=%d at factor %d do not span rows of L=%ld",
               who, a.T, a.factor, a.L);
    VocGemm p;
    p.x = a.x; p.wp = a.packed; p.bias = a.bias; p.res = a.res; p.y = a.y;
    p.Cin = a.Cin; p.Cout = a.Cout; p.Lin = (int)a.L;
    p.transposed = a.u != 0; p.u = a.u ? a.u : 1; p.ostride = p.u;
    p.taps = a.u ? 2 : a.k; p.d = a.u ? 1 : a.d; p.pad = a.u ? (a.k - a.u) / 2 : (a.k * a.d - a.d) / 2;
    p.halo_lo = a.u ? 1 : p.pad;
    p.mtiles = (a.Cout + 31) / 32; p.nchunks = slab_chunks(a.Cin);
    p.slope = a.slope; p.scale = a.scale; p.accumulate = a.accumulate;
    p.frames = a.frames; p.T = a.T; p.factor = a.factor;
    T2_REQUIRE(kVocTT + 2 * p.halo_lo <= kVocStride, "%s: halo %d does not fit the slab", who, p.halo_lo);
    return slab_launch(voc_gemm_kernel<4>, voc_gemm_kernel<2>, voc_gemm_kernel<1>, p, p.mtiles, a.L, p.u, a.B, s);
}

// ------------------------------------------------------------------------------------------------------------------
// the generator
// ------------------------------------------------------------------------------------------------------------------
int hifigan_layers(const t2_hifigan_config& c, std::vector<HifiganLayer>* out, size_t* packed_floats) {   // validates; no device
    T2_REQUIRE(c.resblock == 1 || c.resblock == 2, "hifigan: resblock \"%d\" is not \"1\" or \"2\"", c.resblock);
    T2_REQUIRE(c.n_mel == 80, "hifigan: %d mel channels, conv_pre takes 80", c.n_mel);
    T2_REQUIRE(c.num_upsamples >= 1 && c.num_upsamples <= T2_HIFIGAN_MAX_UPS, "hifigan: %d upsampling stages outside 1..%d", c.num_upsamples, T2_HIFIGAN_MAX_UPS);
    T2_REQUIRE(c.num_kernels >= 1 && c.num_kernels <= T2_HIFIGAN_MAX_KERNELS, "hifigan: %d resblock kernels outside 1..%d", c.num_kernels, T2_HIFIGAN_MAX_KERNELS);
    const int want_d = c.resblock == 1 ? 3 : 2;
    T2_REQUIRE(c.num_dilations == want_d, "hifigan: %d dilations per resblock, ResBlock%d takes %d", c.num_dilations, c.resblock, want_d);
    const int c0 = c.upsample_initial_channel;
    T2_REQUIRE(c0 >= 8 && c0 <= 512 && c0 % ((1 << c.num_upsamples) * 8) == 0,
               "hifigan: upsample_initial_channel=%d must be at most 512 and leave a multiple of 8 channels after %d halvings", c0, c.num_upsamples);
    std::vector<HifiganLayer> L;
    size_t off = 0;
    auto add = [&](int kind, int cin, int cout, int k, int d, int u) -> int {
        if (kind != 2) T2_TRY_RC(voc_shape_check("hifigan", cin, cout, k, d, u));
        HifiganLayer l{kind, cin, cout, k, d, u, 0, 0};
        l.w_off = off; off += kind == 2 ? round4((size_t)cin * k) : voc_packed_floats(cin, cout, k, u);
        l.b_off = off; off += round4(cout);
        L.push_back(l);
        return 0;
    };
    T2_TRY_RC(add(0, c.n_mel, c0, 7, 1, 0));
    for (int i = 0; i < c.num_upsamples; ++i) T2_TRY_RC(add(1, c0 >> i, c0 >> (i + 1), c.upsample_kernel_sizes[i], 1, c.upsample_rates[i]));
    for (int i = 0; i < c.num_upsamples; ++i) {
        const int ch = c0 >> (i + 1);
        for (int j = 0; j < c.num_kernels; ++j) {
            const int k = c.resblock_kernel_sizes[j];
            for (int m = 0; m < c.num_dilations; ++m) T2_TRY_RC(add(0, ch, ch, k, c.resblock_dilation_sizes[j][m], 0));
            if (c.resblock == 1) for (int m = 0; m < 3; ++m) T2_TRY_RC(add(0, ch, ch, k, 1, 0));
        }
    }
    T2_TRY_RC(add(2, c0 >> c.num_upsamples, 1, kVocPostK, 1, 0));
    if (out) *out = L;
    if (packed_floats) *packed_floats = off;
    return 0;
}

int hifigan_plan(const t2_hifigan_config& c, int B, int T, HifiganPlan* out) {
    T2_REQUIRE(out, "hifigan: null plan");
    std::vector<HifiganLayer> L;
    size_t packed = 0;
    T2_TRY_RC(hifigan_layers(c, &L, &packed));
    T2_REQUIRE(B >= 1 && B <= 65535, "hifigan: B=%d outside 1..65535", B);
    T2_REQUIRE(T >= 1, "hifigan: T=%d frames, must be at least 1", T);
    long len = T;
    size_t buf = (size_t)c.upsample_initial_channel * T;
    for (int i = 0; i < c.num_upsamples; ++i) {
        len *= c.upsample_rates[i];
        T2_REQUIRE(len <= (long)INT32_MAX / 2, "hifigan: %ld samples after stage %d exceed the limit of %d per row", len, i, INT32_MAX / 2);
        buf = std::max(buf, (size_t)(c.upsample_initial_channel >> (i + 1)) * len);
    }
    out->out_len = len;
    out->buf_floats = round4(buf * B);
    out->workspace_bytes = 5 * out->buf_floats * sizeof(float);      // XS, X, T, P, Q of the widest stage
    out->packed_bytes = packed * sizeof(float);
    out->n_layers = (int)L.size();
    return 0;
}

static int hifigan_pack(const t2_hifigan_config& c, const float* const* weights, const float* const* biases, int n_layers, float* packed, hipStream_t s) {
    std::vector<HifiganLayer> L;
    T2_TRY_RC(hifigan_layers(c, &L, nullptr));
    T2_REQUIRE(weights && biases && packed, "hifigan_pack: null pointer");
    T2_REQUIRE(n_layers == (int)L.size(), "hifigan_pack: %d layers given, the configuration has %d", n_layers, (int)L.size());
    for (int i = 0; i < n_layers; ++i) {
        const HifiganLayer& l = L[i];
        T2_REQUIRE(weights[i] && biases[i], "hifigan_pack: layer %d has a null weight or bias", i);
        if (l.kind == 2) T2_CHECK_HIP(hipMemcpyAsync(packed + l.w_off, weights[i], (size_t)l.cin * l.k * sizeof(float), hipMemcpyDeviceToDevice, s));
        else T2_TRY_RC(voc_pack(weights[i], packed + l.w_off, l.cin, l.cout, l.k, l.u, s));
        T2_CHECK_HIP(hipMemcpyAsync(packed + l.b_off, biases[i], (size_t)l.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

// frames (nullable, device [B]): per-item frame counts, clamped to [0, T] in the kernels; item b is then computed as if it were
// mel[b, :, :frames[b]] alone, audio and pre_tanh are zero behind frames[b] * prod(rates), which sample_lengths (nullable) receives
static int hifigan_forward(const t2_hifigan_config& c, const t2_hifigan_fwd_args& a, const int32_t* frames, int32_t* sample_lengths, hipStream_t s) {
    std::vector<HifiganLayer> L;
    HifiganPlan pl;
    T2_TRY_RC(hifigan_layers(c, &L, nullptr));
    T2_REQUIRE(a.n_mel == c.n_mel, "hifigan_forward: the mel has %d channels, the generator takes %d", a.n_mel, c.n_mel);
    T2_TRY_RC(hifigan_plan(c, a.B, a.T, &pl));
    T2_REQUIRE(a.packed && a.mel && a.workspace && a.audio, "hifigan_forward: null pointer");
    T2_REQUIRE(frames || !sample_lengths, "hifigan_forward: sample lengths asked for without frame counts");
    float* XS = a.workspace; float* X = XS + pl.buf_floats; float* Tb = X + pl.buf_floats; float* P = Tb + pl.buf_floats; float* Q = P + pl.buf_floats;
    const float kSlope = 0.1f;                                       // LRELU_SLOPE, hifigan_model.py:8
    auto run = [&](const HifiganLayer& l, const float* x, float* y, long len, float slope, const float* res, int accumulate, float scale) {
        return voc_conv(VocConv{a.B, l.cin, l.cout, len, l.k, l.d, l.u, x, a.packed + l.w_off, a.packed + l.b_off, res, y, slope, accumulate, scale,
                                frames, a.T, (int)(len / a.T)}, s);
    };
    size_t li = 0;
    long len = a.T;
    T2_TRY_RC(run(L[li++], a.mel, XS, len, 1.f, nullptr, 0, 1.f));                     // conv_pre: no activation in front
    size_t rb = 1 + c.num_upsamples;                                                   // first resblock layer
    for (int i = 0; i < c.num_upsamples; ++i) {
        T2_TRY_RC(run(L[li++], XS, X, len, kSlope, nullptr, 0, 1.f));                  // x = ups[i](leaky_relu(x))
        len *= c.upsample_rates[i];
        for (int j = 0; j < c.num_kernels; ++j) {
            // xs = r0; xs += r1; ...; x = xs / num_kernels: the last conv of block j adds into XS, the last block scales
            const int acc = j > 0;
            const float scale = j == c.num_kernels - 1 ? 1.f / (float)c.num_kernels : 1.f;
            const float* cur = X;
            float* pp[2] = {P, Q};
            for (int m = 0; m < c.num_dilations; ++m) {
                const bool last = m == c.num_dilations - 1;
                float* dst = last ? XS : pp[m & 1];
                if (c.resblock == 1) {
                    T2_TRY_RC(run(L[rb + m], cur, Tb, len, kSlope, nullptr, 0, 1.f));                                     // c1(leaky_relu(x))
                    T2_TRY_RC(run(L[rb + 3 + m], Tb, dst, len, kSlope, cur, last ? acc : 0, last ? scale : 1.f));        // c2(leaky_relu(xt)) + x
                } else {
                    T2_TRY_RC(run(L[rb + m], cur, dst, len, kSlope, cur, last ? acc : 0, last ? scale : 1.f));           // c(leaky_relu(x)) + x
                }
                cur = dst;
            }
            rb += c.resblock == 1 ? 6 : 2;
        }
    }
    const HifiganLayer& post = L.back();
    T2_REQUIRE(rb + 1 == L.size(), "hifigan_forward: layer table out of step");
    // F.leaky_relu(x) in front of conv_post is torch's default slope 0.01, not LRELU_SLOPE (hifigan_model.py:112)
    return voc_post(XS, a.packed + post.w_off, a.packed + post.b_off, a.audio, a.pre_tanh, a.B, post.cin, len, frames, a.T, (int)(len / a.T), sample_lengths, s);
}

int voc_post(const float* x, const float* w, const float* bias, float* audio, float* pre, int B, int C, long len, const int32_t* frames, int T, int factor,
             int32_t* sample_lengths, hipStream_t s) {
    dim3 grid((unsigned)((len + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(voc_post_kernel, grid, dim3(256), (size_t)C * kVocPostK * sizeof(float), s, x, w, bias, audio, pre, C, len, 0.01f, frames, T, factor,
                       sample_lengths);
    T2_LAUNCH_CHECK();
    return 0;
}

}  // namespace t2

// ---- C ABI (include/t2amd.h)
using namespace t2;
static_assert(T2_VOCODER_TIME_TILE == kVocTT, "t2amd.h mirrors the time tile");

extern "C" {

int t2_hifigan_plan(const t2_hifigan_config* cfg, int B, int T, t2_hifigan_plan_info* out) {
    T2_REQUIRE(cfg && out, "t2_hifigan_plan: null pointer");
    HifiganPlan p;
    T2_TRY_RC(hifigan_plan(*cfg, B, T, &p));
    out->out_len = p.out_len; out->workspace_bytes = p.workspace_bytes; out->packed_bytes = p.packed_bytes;
    out->n_layers = p.n_layers; out->time_tile = kVocTT;
    return 0;
}
int t2_hifigan_pack(const t2_hifigan_config* cfg, const float* const* weights_host, const float* const* biases_host, int n_layers,
                    float* packed, void* stream) {
    T2_REQUIRE(cfg, "t2_hifigan_pack: null configuration");
    return hifigan_pack(*cfg, weights_host, biases_host, n_layers, packed, (hipStream_t)stream);
}
int t2_hifigan_forward(const t2_hifigan_config* cfg, const t2_hifigan_fwd_args* a, void* stream) {
    T2_REQUIRE(cfg && a, "t2_hifigan_forward: null pointer");
    return hifigan_forward(*cfg, *a, nullptr, nullptr, (hipStream_t)stream);
}
int t2_hifigan_forward_ragged(const t2_hifigan_config* cfg, const t2_hifigan_ragged_args* a, void* stream) {
    T2_REQUIRE(cfg && a, "t2_hifigan_forward_ragged: null pointer");
    T2_REQUIRE(a->frames, "t2_hifigan_forward_ragged: null frame counts (t2_hifigan_forward is the call without them)");
    t2_hifigan_fwd_args f{};
    f.B = a->B; f.T = a->T; f.n_mel = a->n_mel;
    f.packed = a->packed; f.mel = a->mel; f.workspace = a->workspace; f.audio = a->audio; f.pre_tanh = a->pre_tanh;
    return hifigan_forward(*cfg, f, a->frames, a->sample_lengths, (hipStream_t)stream);
}
size_t t2_vocoder_packed_floats(int Cin, int Cout, int k, int u) { return voc_packed_floats(Cin, Cout, k, u); }
static int vocoder_layer(const t2_vocoder_conv_args* a, int u, const int32_t* lengths, void* stream) {
    T2_REQUIRE(a->w && a->packed_ws, "t2_vocoder: null weights or packing scratch");
    T2_TRY_RC(voc_pack(a->w, a->packed_ws, a->Cin, a->Cout, a->k, u, (hipStream_t)stream));
    return voc_conv(VocConv{a->B, a->Cin, a->Cout, (long)a->L, a->k, a->d, u, a->x, a->packed_ws, a->bias, u ? nullptr : a->residual, a->y,
                            a->slope, u ? 0 : a->accumulate, u ? 1.f : a->scale, lengths, lengths ? a->L : 0, lengths ? 1 : 0}, (hipStream_t)stream);
}
int t2_vocoder_conv_ragged(const t2_vocoder_conv_ragged_args* a, void* stream) {
    T2_REQUIRE(a, "t2_vocoder_conv_ragged: null arguments");
    T2_REQUIRE(a->lengths, "t2_vocoder_conv_ragged: null lengths (t2_vocoder_conv1d / t2_vocoder_conv_transpose1d are the calls without them)");
    T2_REQUIRE(a->conv.u >= 0, "t2_vocoder_conv_ragged: stride u=%d must not be negative", a->conv.u);
    return vocoder_layer(&a->conv, a->conv.u, a->lengths, stream);
}
int t2_vocoder_conv1d(const t2_vocoder_conv_args* a, void* stream) {
    T2_REQUIRE(a, "t2_vocoder_conv1d: null arguments");
    T2_REQUIRE(a->u == 0, "t2_vocoder_conv1d: stride u=%d given, a Conv1d has none", a->u);
    return vocoder_layer(a, 0, nullptr, stream);
}
int t2_vocoder_conv_transpose1d(const t2_vocoder_conv_args* a, void* stream) {
    T2_REQUIRE(a, "t2_vocoder_conv_transpose1d: null arguments");
    T2_REQUIRE(a->u >= 1, "t2_vocoder_conv_transpose1d: stride u=%d must be positive", a->u);
    return vocoder_layer(a, a->u, nullptr, stream);
}

}  // extern "C"
