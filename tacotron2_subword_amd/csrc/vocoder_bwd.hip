// HiFi-GAN generator, training: the forward that keeps every conv's pre-activation input (the tape) and the backward of
// hifigan_infer/hifigan_model.py: Generator.forward (:100-116), ResBlock1.forward (:35-42), ResBlock2.forward (:63-68), which the
// reference leaves to torch's autograd.  Exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32), whatever t2_set_precision
// says; no atomics, every sum in a fixed order, partial sums added ascending in fp64: the same bits from run to run.
//
// Four kernels, all on slab_gemm.h's pieces or on the shape of wg_wgrad_kernel (waveglow_kernels.hip):
//   voc_dgrad_kernel     dX[ci][t] = ((acc ? dX : 0) + (res + lrelu'(x[ci][t]) * sum_{co,j} W.. * dY..) * scale.  Conv1d: the forward
//                        GEMM with M = Cin, K = Cout and the taps flipped (padding is symmetric), on a pack of its own.
//                        ConvTranspose1d (k = 2u, stride u, pad u/2): u*q + j - pad = u*(q + s) + r makes it a three-tap stride-1
//                        convolution over the Cout*u de-interleaved rows (co, r); the slab loader reads a contiguous run of dY
//                        and scatters element p to row co*u + p % u, column p / u.  One launch per layer, no zero-stuffed tensor.
//   voc_wgrad_kernel     C[m][n] = sum_b sum_l A[b][m][l] * Bop[b][n][l], the reduction along time in chunks of 32 steps, 128 x 128
//                        tiles, split into runs that depend on the shape alone; voc_wgrad_reduce_kernel adds the partial planes
//                        ascending in fp64.  The vocoder's own kernel (not wg_wgrad_kernel generalised): it stages both operands
//                        through the leaky ReLU, walks (tap, channel) columns densely and reads dY at u*q + j - pad for the
//                        transposed form, where the bias gradient is a row of ones on the A side.
//   voc_post_bwd_kernel  conv_post (Cout = 1) and the tanh: d_pre = d_audio * (1 - audio^2), the data gradient (slope 0.01) per
//                        thread, dw[ci][j] and db as fp64 partial sums per workgroup, added ascending by voc_post_reduce_kernel.
//   voc_bwd_pack_kernel  the two data-gradient weight packs.
// The plan (hifigan_train_plan) is pure: the tape, the scratch and the launch list from the configuration, B and T alone.
#include <algorithm>
#include <vector>

#include "slab_gemm.h"
#include "vocoder.h"

namespace t2 {

// ------------------------------------------------------------------------------------------------------------------
// data gradient
// ------------------------------------------------------------------------------------------------------------------
struct VocDgrad {
    const float* dy; const float* wp; const float* x; const float* res; float* dx;
    int Cin, Cout, L;                              // dX [B][Cin][L]; dY [B][Cout][L] (u = 0) or [B][Cout][L*u]
    int u, taps, d, halo, mtiles, nchunks;
    float slope, scale; int accumulate;
};

template <int WM>
__global__ void __launch_bounds__(WM * 128) voc_dgrad_kernel(VocDgrad p) {
    __shared__ float slab[kSlabCK * kVocStride];
    const int wm = (threadIdx.x >> 6) % WM;
    const int mt = blockIdx.y * WM + wm;
    const bool active = mt < p.mtiles;             // uniform over the wave
    const int b = blockIdx.z;
    const int lane = threadIdx.x & 63, wt = (threadIdx.x >> 6) / WM, tc = wt * 64 + (lane & 31), hk = lane >> 5;
    const long t0 = (long)blockIdx.x * kVocTT;
    const long Lout = p.u ? (long)p.L * p.u : p.L;
    const float* dyb = p.dy + (size_t)b * p.Cout * Lout;
    const f32x4* wp = reinterpret_cast<const f32x4*>(p.wp) + (size_t)(active ? mt : 0) * p.nchunks * p.taps * 128;
    f32x16 acc[1][2] = {{f32x16{0}, f32x16{0}}};
    for (int c = 0; c < p.nchunks; ++c) {
        if (c) __syncthreads();                    // every wave is done reading the previous slab
        if (p.u) {
            // rows (co, r) = 16*c .. 16*c + 15 of the de-interleaved dY, columns q = t0 - 1 .. t0 + 128: a contiguous run of each
            // channel, element p to row co*u + p % u, column p / u.  Cout * u is a multiple of 16, so every row of the chunk is written
            const int u = p.u, co0 = c * kSlabCK / u, nco = (c * kSlabCK + kSlabCK - 1) / u - co0 + 1, run = u * (kVocTT + 2);
            const long p0 = (t0 - 1) * u;
            for (int idx = threadIdx.x; idx < nco * run; idx += WM * 128) {
                const int co = co0 + idx / run, pp = idx % run, row = co * u + pp % u - c * kSlabCK;
                const long q = p0 + pp;
                if (row >= 0 && row < kSlabCK) slab[row * kVocStride + pp / u] = (co < p.Cout && q >= 0 && q < Lout) ? dyb[(size_t)co * Lout + q] : 0.f;
            }
        } else {
            slab_stage<kVocStride, WM * 2>(slab, dyb, p.Cout, c * kSlabCK, p.L, t0, p.halo, [](float v) { return v; });
        }
        __syncthreads();
        if (active)
            for (int j = 0; j < p.taps; ++j)
                slab_mfma_step<kVocStride, 1>(slab + hk * kVocStride + tc + j * p.d, wp + ((size_t)c * p.taps + j) * 128 + lane, acc);
    }
    if (!active) return;
    slab_walk<WM, 1>(acc, mt, p.Cin, p.L, [=](int ci, long q, const float (&a)[1]) {
        const size_t o = ((size_t)b * p.Cin + ci) * p.L + q;
        float v = a[0];
        if (p.x) v *= p.x[o] > 0.f ? 1.f : p.slope;      // torch's convention at 0 (and -0): the slope side
        if (p.res) v += p.res[o];
        v *= p.scale;
        if (p.accumulate) v = p.dx[o] + v;
        p.dx[o] = v;
    });
}

// packed[mtile][chunk * taps + tap][pg][lane][i] (slab_gemm.h), rows = Cin.  Conv1d w [Cout][Cin][k]: element (ci, co, j) = w[co][ci][k-1-j].
// ConvTranspose1d w [Cin][Cout][2u]: element (ci, kk = co*u + r, tap s + 1) = w[ci][co][u*s + r + pad], zero where that tap does not exist
__global__ void __launch_bounds__(256) voc_bwd_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin, int Cout, int k, int u, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int taps = u ? 3 : k, nsteps = slab_chunks(u ? Cout * u : Cout) * taps;
    const int i = idx & 3, lane = (idx >> 2) & 63, pg = (idx >> 8) & 1;
    const size_t rest = idx >> 9;
    const int step = (int)(rest % nsteps), mt = (int)(rest / nsteps);
    const int ci = mt * 32 + (lane & 31), kk = (step / taps) * kSlabCK + 2 * (4 * pg + i) + (lane >> 5), j = step % taps;
    float v = 0.f;
    if (u) {
        const int co = kk / u, jj = u * (j - 1) + kk % u + (k - u) / 2;
        if (ci < Cin && co < Cout && jj >= 0 && jj < k) v = w[((size_t)ci * Cout + co) * k + jj];
    } else if (ci < Cin && kk < Cout) {
        v = w[((size_t)kk * Cin + ci) * k + (k - 1 - j)];
    }
    out[idx] = v;
}

size_t voc_dgrad_packed_floats(int Cin, int Cout, int k, int u) {
    return u ? slab_packed_floats(1, Cin, Cout * u, 3, 0) : slab_packed_floats(1, Cin, Cout, k, 0);
}

static int voc_dgrad_pack(const float* w, float* packed, int Cin, int Cout, int k, int u, hipStream_t s) {
    T2_TRY_RC(voc_shape_check("vocoder data-gradient pack", Cin, Cout, k, 1, u));
    T2_REQUIRE(w && packed, "vocoder data-gradient pack: null pointer");
    const size_t total = voc_dgrad_packed_floats(Cin, Cout, k, u);
    hipLaunchKernelGGL(voc_bwd_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, packed, Cin, Cout, k, u, total);
    T2_LAUNCH_CHECK();
    return 0;
}

// One layer's data gradient on its pack.  L is the layer's input length: dx, x, res [B][Cin][L]; dy [B][Cout][L] or [B][Cout][L*u]
struct VocDgradCall {
    int B, Cin, Cout; long L; int k, d, u;
    const float* dy; const float* packed; const float* x; const float* res; float* dx;
    float slope; int accumulate; float scale;
};

static bool voc_overlap(const float* a, size_t na, const float* b, size_t nb) {      // [a, a + na) meets [b, b + nb)
    return a && b && reinterpret_cast<uintptr_t>(a) < reinterpret_cast<uintptr_t>(b + nb) && reinterpret_cast<uintptr_t>(b) < reinterpret_cast<uintptr_t>(a + na);
}

// everything voc_dgrad refuses, so that a unit entry point can refuse before it packs
static int voc_dgrad_check(const VocDgradCall& a) {
    const char* who = a.u ? "vocoder conv_transpose1d data gradient" : "vocoder conv1d data gradient";
    T2_TRY_RC(voc_shape_check(who, a.Cin, a.Cout, a.k, a.u ? 1 : a.d, a.u));
    T2_REQUIRE(a.B >= 1 && a.B <= 65535, "%s: B=%d outside 1..65535", who, a.B);
    T2_REQUIRE(a.L >= 1 && a.L * (a.u ? a.u : 1) <= (long)INT32_MAX / 2, "%s: L=%ld outside 1..%d output samples per row", who, a.L, INT32_MAX / 2);
    T2_REQUIRE(a.dy && a.packed && a.dx, "%s: null pointer", who);
    const size_t nx = (size_t)a.B * a.Cin * a.L, ny = (size_t)a.B * a.Cout * a.L * (a.u ? a.u : 1);
    T2_REQUIRE(!voc_overlap(a.dx, nx, a.dy, ny) && !voc_overlap(a.dx, nx, a.res, nx),
               "%s: the destination must not overlap the upstream gradient or the residual (tiles read a halo of both)", who);
    T2_REQUIRE(!a.u || (a.Cout * a.u) % kSlabCK == 0, "%s: Cout * stride = %d is not a multiple of %d", who, a.Cout * a.u, kSlabCK);
    return 0;
}

static int voc_dgrad(const VocDgradCall& a, hipStream_t s) {
    const char* who = a.u ? "vocoder conv_transpose1d data gradient" : "vocoder conv1d data gradient";
    T2_TRY_RC(voc_dgrad_check(a));
    VocDgrad p;
    p.dy = a.dy; p.wp = a.packed; p.x = a.x; p.res = a.res; p.dx = a.dx;
    p.Cin = a.Cin; p.Cout = a.Cout; p.L = (int)a.L; p.u = a.u;
    p.taps = a.u ? 3 : a.k; p.d = a.u ? 1 : a.d; p.halo = a.u ? 1 : (a.k * a.d - a.d) / 2;
    p.mtiles = (a.Cin + 31) / 32; p.nchunks = slab_chunks(a.u ? a.Cout * a.u : a.Cout);
    p.slope = a.slope; p.scale = a.scale; p.accumulate = a.accumulate;
    T2_REQUIRE(kVocTT + 2 * p.halo <= kVocStride, "%s: halo %d does not fit the slab", who, p.halo);
    return slab_launch(voc_dgrad_kernel<4>, voc_dgrad_kernel<2>, voc_dgrad_kernel<1>, p, p.mtiles, a.L, 1, a.B, s);
}

// ------------------------------------------------------------------------------------------------------------------
// weight and bias gradient
// ------------------------------------------------------------------------------------------------------------------
constexpr int kVocWgTile = 128, kVocWgTL = 32, kVocWgStride = 34, kVocWgMaxSplit = 256;
static_assert(kVocWgStride % 4 == 2 && kVocWgStride >= kVocWgTL, "rows 0..31 x 2 k-halves on 64 distinct banks");

// C[m][n] = sum_b sum_{l < La} A[b][m][l] * Bop[b][n][l].  A: rows m < Ma are lrelu(a[b][m][l], slope_a), row Ma (if M = Ma + 1) is ones.
// Bop: column n = j*Cb + c (j < taps) is lrelu(bsrc[b][c][l*bstride + j*d - pad], slope_b), zero outside [0, Lb); column taps*Cb (if
// ones_col) is ones.  Conv1d: A = dY, Bop = x.  ConvTranspose1d: A = x with the row of ones, Bop = dY at stride u.
struct VocWgrad {
    const float* a; const float* bsrc; float* part; float* dw; float* db;
    int M, Ma, Cb, taps, Ntot, ones_col;
    long La, Lb;
    int bstride, d, pad;
    float slope_a, slope_b;
    int B, nchunk, per, nsplit, mtiles, ntiles;
    int transposed, cout, u;                        // for the reduce: where the bias gradient lies
};

__global__ void __launch_bounds__(256) voc_wgrad_kernel(VocWgrad p) {
    __shared__ float As[kVocWgTile * kVocWgStride], Bs[kVocWgTile * kVocWgStride];
    __shared__ int bch[kVocWgTile], bshift[kVocWgTile];     // per column of the tile: its channel (-1: the ones, -2: none) and its tap's shift
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hk = lane >> 5;
    const int mt = blockIdx.x % p.mtiles, nt = blockIdx.x / p.mtiles;
    const int m0 = mt * kVocWgTile, n0 = nt * kVocWgTile;
    const int total = p.B * p.nchunk, u0 = blockIdx.y * p.per, u1 = min(total, u0 + p.per);
    const int col = threadIdx.x & 31, row0 = threadIdx.x >> 5;
    const float sa = p.slope_a, sb = p.slope_b;
    // The waves' share of the tile follows the rows it holds (uniform over the workgroup): up to 32 rows (the 32-channel stage, the
    // transposed form's row of ones) every wave takes one 32 x 32 tile along the columns, up to 64 rows two, else 64 x 64 each.
    // An element's sum keeps its order (chunks, then time steps, ascending) whichever wave owns it
    const int rows_here = min(kVocWgTile, p.M - m0);
    const int ni = rows_here <= 32 ? 1 : 2, nj = rows_here <= 64 ? 1 : 2;
    const int rbase = nj == 1 ? 0 : (wave & 1) * 64, cbase = nj == 1 ? wave * 32 : (wave >> 1) * 64;
    const int arows = nj == 1 ? ni * 32 : kVocWgTile;
    if (threadIdx.x < kVocWgTile) {
        const int n = n0 + threadIdx.x;
        int c = -2, sh = 0;
        if (n < p.taps * p.Cb) { c = n % p.Cb; sh = (n / p.Cb) * p.d - p.pad; }
        else if (n < p.Ntot) c = -1;
        bch[threadIdx.x] = c; bshift[threadIdx.x] = sh;
    }
    __syncthreads();
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) { acc[i][0] = f32x16{0}; acc[i][1] = f32x16{0}; }
    for (int un = u0; un < u1; ++un) {
        const int b = un / p.nchunk;
        const long t = (long)(un % p.nchunk) * kVocWgTL + col;
        if (un > u0) __syncthreads();              // every wave is done reading the previous slabs
        for (int row = row0; row < arows; row += 8) {
            const int m = m0 + row;
            float v = 0.f;
            if (t < p.La) {
                if (m < p.Ma) { v = p.a[((size_t)b * p.Ma + m) * p.La + t]; v = v > 0.f ? v : v * sa; }
                else if (m < p.M) v = 1.f;
            }
            As[row * kVocWgStride + col] = v;
        }
        for (int row = row0; row < kVocWgTile; row += 8) {
            const int c = bch[row];
            float v = 0.f;
            if (t < p.La) {
                if (c >= 0) {
                    const long tb = t * p.bstride + bshift[row];
                    if (tb >= 0 && tb < p.Lb) { v = p.bsrc[((size_t)b * p.Cb + c) * p.Lb + tb]; v = v > 0.f ? v : v * sb; }
                } else if (c == -1) {
                    v = 1.f;
                }
            }
            Bs[row * kVocWgStride + col] = v;
        }
        __syncthreads();
        const float* ap = As + (rbase + (lane & 31)) * kVocWgStride + hk;
        const float* bp = Bs + (cbase + (lane & 31)) * kVocWgStride + hk;
#pragma unroll
        for (int kk = 0; kk < kVocWgTL / 2; ++kk) {
            const float a0 = ap[2 * kk], b0 = bp[2 * kk];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            if (ni > 1) {                          // uniform over the workgroup
                const float a1 = ap[32 * kVocWgStride + 2 * kk];
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                if (nj > 1) {
                    const float b1 = bp[32 * kVocWgStride + 2 * kk];
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
                }
            }
        }
    }
    // lane holds column (of C) lane & 31 and rows (e&3) + 8*(e>>2) + 4*hk of each 32x32 tile
    float* pp = p.part + (size_t)blockIdx.y * p.M * p.Ntot;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + cbase + j * 32 + (lane & 31);
            if (i >= ni || j >= nj || n >= p.Ntot) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + rbase + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hk;
                if (m < p.M) pp[(size_t)m * p.Ntot + n] = acc[i][j][e];
            }
        }
}

// dw[m][c][j] (torch's layout for both forms: Conv1d [Cout][Cin][k], ConvTranspose1d [Cin][Cout][k]) = the planes' sum at (m, j*Cb + c);
// db: Conv1d the column of ones; ConvTranspose1d the row of ones over the u taps j = pad .. pad + u - 1, which meet every output once
__global__ void __launch_bounds__(256) voc_wgrad_reduce_kernel(VocWgrad p) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, nw = (size_t)p.Ma * p.taps * p.Cb, plane = (size_t)p.M * p.Ntot;
    if (idx < nw) {
        const int m = (int)(idx / ((size_t)p.taps * p.Cb)), n = (int)(idx % ((size_t)p.taps * p.Cb)), j = n / p.Cb, c = n % p.Cb;
        double acc = 0.0;
        for (int y = 0; y < p.nsplit; ++y) acc += (double)p.part[(size_t)y * plane + (size_t)m * p.Ntot + n];
        p.dw[((size_t)m * p.Cb + c) * p.taps + j] = (float)acc;
    } else if (idx < nw + p.cout && p.db) {
        const int co = (int)(idx - nw);
        double acc = 0.0;
        if (p.transposed) {
            for (int j = p.pad; j < p.pad + p.u; ++j)
                for (int y = 0; y < p.nsplit; ++y) acc += (double)p.part[(size_t)y * plane + (size_t)p.Ma * p.Ntot + (size_t)j * p.Cb + co];
        } else {
            for (int y = 0; y < p.nsplit; ++y) acc += (double)p.part[(size_t)y * plane + (size_t)co * p.Ntot + (size_t)p.taps * p.Cb];
        }
        p.db[co] = (float)acc;
    }
}

// the shape of one launch from the sizes alone.  L: the layer's input length
static VocWgrad voc_wgrad_shape(int B, int Cin, int Cout, long L, int k, int d, int u) {
    VocWgrad p{};
    p.B = B; p.transposed = u != 0; p.cout = Cout; p.u = u;
    if (u) { p.Ma = Cin; p.M = Cin + 1; p.Cb = Cout; p.taps = k; p.ones_col = 0; p.La = L; p.Lb = L * u; p.bstride = u; p.d = 1; p.pad = (k - u) / 2; }
    else { p.Ma = p.M = Cout; p.Cb = Cin; p.taps = k; p.ones_col = 1; p.La = p.Lb = L; p.bstride = 1; p.d = d; p.pad = (k * d - d) / 2; }
    p.Ntot = p.taps * p.Cb + p.ones_col;
    p.mtiles = (p.M + kVocWgTile - 1) / kVocWgTile; p.ntiles = (p.Ntot + kVocWgTile - 1) / kVocWgTile;
    p.nchunk = (int)((L + kVocWgTL - 1) / kVocWgTL);
    const long total = (long)B * p.nchunk;
    // at most 1024 workgroups, what 256 CUs hold at once at 4 per CU (34 816 bytes of LDS): one more would wait a whole round
    const long nsplit = std::min<long>(std::min<long>(kVocWgMaxSplit, total), std::max<long>(1, 1024 / (p.mtiles * p.ntiles)));
    p.per = (int)((total + nsplit - 1) / nsplit);
    p.nsplit = (int)((total + p.per - 1) / p.per);
    return p;
}
size_t voc_wgrad_part_floats(int B, int Cin, int Cout, long L, int k, int d, int u) {
    const VocWgrad p = voc_wgrad_shape(B, Cin, Cout, L, k, d, u);
    return round4((size_t)p.nsplit * p.M * p.Ntot);
}

struct VocWgradCall {
    int B, Cin, Cout; long L; int k, d, u;
    const float* x; const float* dy; float* dw; float* db; float* part; float slope;
};

static int voc_wgrad(const VocWgradCall& a, hipStream_t s) {
    const char* who = a.u ? "vocoder conv_transpose1d weight gradient" : "vocoder conv1d weight gradient";
    T2_TRY_RC(voc_shape_check(who, a.Cin, a.Cout, a.k, a.u ? 1 : a.d, a.u));
    T2_REQUIRE(a.B >= 1 && a.B <= 65535, "%s: B=%d outside 1..65535", who, a.B);
    T2_REQUIRE(a.L >= 1 && a.L * (a.u ? a.u : 1) <= (long)INT32_MAX / 2, "%s: L=%ld outside 1..%d output samples per row", who, a.L, INT32_MAX / 2);
    T2_REQUIRE(a.x && a.dy && a.dw && a.part, "%s: null pointer", who);
    VocWgrad p = voc_wgrad_shape(a.B, a.Cin, a.Cout, a.L, a.k, a.d, a.u);
    p.part = a.part; p.dw = a.dw; p.db = a.db;
    if (a.u) { p.a = a.x; p.bsrc = a.dy; p.slope_a = a.slope; p.slope_b = 1.f; }
    else { p.a = a.dy; p.bsrc = a.x; p.slope_a = 1.f; p.slope_b = a.slope; }
    hipLaunchKernelGGL(voc_wgrad_kernel, dim3((unsigned)(p.mtiles * p.ntiles), (unsigned)p.nsplit), dim3(256), 0, s, p);
    T2_LAUNCH_CHECK();
    const size_t n = (size_t)p.Ma * p.taps * p.Cb + p.cout;
    hipLaunchKernelGGL(voc_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
    T2_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// conv_post and the tanh, backwards
// ------------------------------------------------------------------------------------------------------------------
constexpr int kVocPostMaxC = 512;

__device__ __forceinline__ double voc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One thread per sample t of item b.  d_pre[t] = d_audio[t] * (1 - audio[t]^2), staged with a halo of 3 in LDS.
// dx[ci][t] = lrelu'(x[ci][t]) * sum_j w[ci][j] * d_pre[t - j + 3] * scale;  the thread's share of dw[ci][j] is lrelu(x[ci][t]) *
// d_pre[t - j + 3] and of db d_pre[t]: summed over the workgroup in fp64 (wave by shuffles, the four waves ascending) to
// part[(b * gridDim.x + blockIdx.x) * (7C + 1) + ...]
__global__ void __launch_bounds__(256) voc_post_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ audio,
                                                          const float* __restrict__ d_audio, float* __restrict__ dx, double* __restrict__ part, int C, long L,
                                                          float slope, float scale) {
    __shared__ float dp[256 + kVocPostK - 1];
    __shared__ double wsum[4][kVocPostK + 1];
    extern __shared__ float wl[];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long tb = (long)blockIdx.x * 256, t = tb + threadIdx.x;
    for (int i = threadIdx.x; i < C * kVocPostK; i += 256) wl[i] = w[i];
    for (int i = threadIdx.x; i < 256 + kVocPostK - 1; i += 256) {
        const long tt = tb + i - kVocPostK / 2;
        float v = 0.f;
        if (tt >= 0 && tt < L) { const float y = audio[(size_t)b * L + tt]; v = d_audio[(size_t)b * L + tt] * (1.f - y * y); }
        dp[i] = v;
    }
    __syncthreads();
    const bool valid = t < L;
    float g[kVocPostK];                            // g[j] = d_pre[t - j + 3]
#pragma unroll
    for (int j = 0; j < kVocPostK; ++j) g[j] = dp[threadIdx.x + kVocPostK - 1 - j];
    double* pp = part + ((size_t)b * gridDim.x + blockIdx.x) * ((size_t)C * kVocPostK + 1);
    for (int ci = 0; ci <= C; ++ci) {              // ci = C: the bias, against a row of ones at tap 3
        float xv = 0.f, av = 0.f;
        if (valid && ci < C) { xv = x[((size_t)b * C + ci) * L + t]; av = xv > 0.f ? xv : xv * slope; }
        if (valid && ci == C) av = 1.f;
        if (ci < C && valid) {
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < kVocPostK; ++j) acc = fmaf(wl[ci * kVocPostK + j], g[j], acc);
            dx[((size_t)b * C + ci) * L + t] = acc * (xv > 0.f ? 1.f : slope) * scale;
        }
        if (ci) __syncthreads();                   // wsum of the previous channel has been read
#pragma unroll
        for (int j = 0; j < kVocPostK; ++j) {
            const double sv = voc_wave_sum((double)av * (double)g[j]);
            if (lane == 0) wsum[wave][j] = sv;
        }
        __syncthreads();
        if (threadIdx.x < kVocPostK) {
            const double sv = ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
            if (ci < C) pp[ci * kVocPostK + threadIdx.x] = sv;
            else if (threadIdx.x == kVocPostK / 2) pp[C * kVocPostK] = sv;
        }
    }
}

__global__ void __launch_bounds__(256) voc_post_reduce_kernel(const double* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, int C, int nparts) {
    const int idx = blockIdx.x * 256 + threadIdx.x, n = C * kVocPostK + 1;
    if (idx >= n) return;
    double acc = 0.0;
    for (int y = 0; y < nparts; ++y) acc += part[(size_t)y * n + idx];
    if (idx < n - 1) dw[idx] = (float)acc;
    else db[0] = (float)acc;
}

size_t voc_post_part_doubles(int B, int C, long L) { return (size_t)B * ((L + 255) / 256) * ((size_t)C * kVocPostK + 1); }

struct VocPostBwdCall {
    int B, C; long L;
    const float* x; const float* w; const float* audio; const float* d_audio; float* dx; float* dw; float* db; double* part; float scale;
};

static int voc_post_bwd(const VocPostBwdCall& a, hipStream_t s) {
    const char* who = "vocoder conv_post backward";
    T2_REQUIRE(a.C >= 1 && a.C <= kVocPostMaxC, "%s: %d channels outside 1..%d", who, a.C, kVocPostMaxC);
    T2_REQUIRE(a.B >= 1 && a.B <= 65535, "%s: B=%d outside 1..65535", who, a.B);
    T2_REQUIRE(a.L >= 1 && a.L <= (long)INT32_MAX / 2, "%s: L=%ld outside 1..%d", who, a.L, INT32_MAX / 2);
    T2_REQUIRE(a.x && a.w && a.audio && a.d_audio && a.dx && a.dw && a.db && a.part, "%s: null pointer", who);
    T2_REQUIRE((reinterpret_cast<uintptr_t>(a.part) & 7) == 0, "%s: the partial sums are doubles, the scratch must be 8-byte aligned", who);
    const unsigned nblk = (unsigned)((a.L + 255) / 256);
    hipLaunchKernelGGL(voc_post_bwd_kernel, dim3(nblk, (unsigned)a.B), dim3(256), (size_t)a.C * kVocPostK * sizeof(float), s, a.x, a.w, a.audio, a.d_audio, a.dx,
                       a.part, a.C, a.L, 0.01f, a.scale);
    T2_LAUNCH_CHECK();
    hipLaunchKernelGGL(voc_post_reduce_kernel, dim3((unsigned)((a.C * kVocPostK + 1 + 255) / 256)), dim3(256), 0, s, a.part, a.dw, a.db, a.C, (int)(nblk * a.B));
    T2_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// the plan: pure, no device
// ------------------------------------------------------------------------------------------------------------------
enum { kOpConv, kOpPost, kOpPostBwd, kOpWgrad, kOpDgrad, kOpCount };
static_assert(kOpCount == T2_HIFIGAN_TRAIN_OPS, "t2amd.h mirrors the kinds of launch");
enum { kSpNone, kSpTape, kSpWs, kSpMel, kSpAudio, kSpDAudio, kSpDMel };
struct VocRef { int sp; size_t off; };
// One entry of the launch list.  kOpConv: out = conv(lrelu(x)) (+ res); kOpPost: audio from x; kOpPostBwd: out = dX from x and the
// audio's gradient, with the layer's dw, db; kOpWgrad: the layer's dw, db from x and dy; kOpDgrad: out = dX from dy, masked by x
struct VocStep { int op, layer; long len; VocRef x, dy, res, out; float slope; int accumulate; float scale; };

struct HifiganTrainPlan {
    HifiganPlan base;
    std::vector<HifiganLayer> L;
    std::vector<size_t> bwd_off, gw_off, gb_off;   // per layer: the data-gradient pack; dw and db in the gradient arena (torch layouts)
    size_t packed_bwd_floats, grad_floats, tape_floats, ws_floats, part_floats, post_part_doubles;
    std::vector<VocStep> fwd, bwd;
};

static int hifigan_train_plan(const t2_hifigan_config& c, int B, int T, bool mel_grad, HifiganTrainPlan* out) {
    HifiganTrainPlan& P = *out;
    size_t packed = 0;
    T2_TRY_RC(hifigan_layers(c, &P.L, &packed));
    T2_TRY_RC(hifigan_plan(c, B, T, &P.base));
    const int nl = (int)P.L.size(), nk = c.num_kernels, nd = c.num_dilations, per_block = c.resblock == 1 ? 6 : 2;
    P.bwd_off.assign(nl, 0); P.gw_off.assign(nl, 0); P.gb_off.assign(nl, 0);
    size_t boff = 0, goff = 0;
    for (int i = 0; i < nl; ++i) {
        const HifiganLayer& l = P.L[i];
        P.bwd_off[i] = boff;
        if (l.kind != 2) boff += voc_dgrad_packed_floats(l.cin, l.cout, l.k, l.u);
        P.gw_off[i] = goff; goff += round4((size_t)l.cin * l.cout * l.k);
        P.gb_off[i] = goff; goff += round4(l.cout);
    }
    P.packed_bwd_floats = boff; P.grad_floats = goff;
    // ---- the tape: conv_pre's output; per stage X (ups' output), per block the r_m (m = 1 .. nd-1) and, ResBlock1, the t_m; XS
    size_t toff = 0;
    auto take = [&](size_t n) { const size_t o = toff; toff += round4(n); return o; };
    const size_t bf = P.base.buf_floats;
    const VocRef G{kSpWs, 0}, DX{kSpWs, bf}, DT{kSpWs, 2 * bf}, PP[2] = {{kSpWs, 3 * bf}, {kSpWs, 4 * bf}}, none{kSpNone, 0};
    const float kSlope = 0.1f, inv = 1.f / (float)nk;
    struct Stage { VocRef in, X, XS; long len_in, len; std::vector<VocRef> r, t; };   // r[j*nd + m], t[j*nd + m]
    std::vector<Stage> st(c.num_upsamples);
    P.part_floats = 0;
    auto part = [&](const HifiganLayer& l, long len) { P.part_floats = std::max(P.part_floats, voc_wgrad_part_floats(B, l.cin, l.cout, len, l.k, l.d, l.u)); };
    long len = T;
    VocRef cur{kSpTape, take((size_t)B * c.upsample_initial_channel * T)};
    P.fwd.push_back(VocStep{kOpConv, 0, len, {kSpMel, 0}, none, none, cur, 1.f, 0, 1.f});           // conv_pre: no activation in front
    part(P.L[0], len);
    int rb = 1 + c.num_upsamples;
    for (int i = 0; i < c.num_upsamples; ++i) {
        Stage& S = st[i];
        const int ch = c.upsample_initial_channel >> (i + 1);
        S.in = cur; S.len_in = len;
        part(P.L[1 + i], len);
        len *= c.upsample_rates[i];
        S.len = len;
        const size_t n = (size_t)B * ch * len;
        S.X = VocRef{kSpTape, take(n)};
        P.fwd.push_back(VocStep{kOpConv, 1 + i, S.len_in, S.in, none, none, S.X, kSlope, 0, 1.f});
        S.XS = VocRef{kSpTape, take(n)};
        S.r.assign((size_t)nk * nd, none); S.t.assign((size_t)nk * nd, none);
        for (int j = 0; j < nk; ++j) {
            VocRef x = S.X;
            for (int m = 0; m < nd; ++m) {
                const bool last = m == nd - 1;
                S.r[j * nd + m] = x;
                const VocRef dst = last ? S.XS : VocRef{kSpTape, take(n)};
                const int lbase = rb + j * per_block;
                if (c.resblock == 1) {
                    S.t[j * nd + m] = VocRef{kSpTape, take(n)};
                    P.fwd.push_back(VocStep{kOpConv, lbase + m, len, x, none, none, S.t[j * nd + m], kSlope, 0, 1.f});
                    P.fwd.push_back(VocStep{kOpConv, lbase + 3 + m, len, S.t[j * nd + m], none, x, dst, kSlope, last && j > 0, last && j == nk - 1 ? inv : 1.f});
                    part(P.L[lbase + 3 + m], len);
                } else {
                    P.fwd.push_back(VocStep{kOpConv, lbase + m, len, x, none, x, dst, kSlope, last && j > 0, last && j == nk - 1 ? inv : 1.f});
                }
                part(P.L[lbase + m], len);
                x = dst;
            }
        }
        rb += nk * per_block;
        cur = S.XS;
    }
    T2_REQUIRE(rb + 1 == nl, "hifigan train plan: layer table out of step");
    P.fwd.push_back(VocStep{kOpPost, nl - 1, len, cur, none, none, {kSpAudio, 0}, 0.01f, 0, 1.f});
    P.tape_floats = toff;
    // ---- backwards.  G holds the gradient on a stage's output already divided by num_kernels (x = xs / num_kernels), so every
    // block reads it as it is; DX gathers the blocks' gradients on the stage's X
    P.bwd.push_back(VocStep{kOpPostBwd, nl - 1, len, cur, {kSpDAudio, 0}, none, G, 0.01f, 0, inv});
    for (int i = c.num_upsamples - 1; i >= 0; --i) {
        const Stage& S = st[i];
        rb -= nk * per_block;
        for (int j = 0; j < nk; ++j) {
            VocRef d = G;
            const int lbase = rb + j * per_block;
            for (int m = nd - 1; m >= 0; --m) {
                const VocRef x = S.r[j * nd + m], dst = m == 0 ? DX : PP[m & 1];
                const int acc = m == 0 && j > 0;
                if (c.resblock == 1) {
                    const VocRef t = S.t[j * nd + m];
                    P.bwd.push_back(VocStep{kOpWgrad, lbase + 3 + m, S.len, t, d, none, none, kSlope, 0, 1.f});
                    P.bwd.push_back(VocStep{kOpDgrad, lbase + 3 + m, S.len, t, d, none, DT, kSlope, 0, 1.f});
                    P.bwd.push_back(VocStep{kOpWgrad, lbase + m, S.len, x, DT, none, none, kSlope, 0, 1.f});
                    P.bwd.push_back(VocStep{kOpDgrad, lbase + m, S.len, x, DT, d, dst, kSlope, acc, 1.f});
                } else {
                    P.bwd.push_back(VocStep{kOpWgrad, lbase + m, S.len, x, d, none, none, kSlope, 0, 1.f});
                    P.bwd.push_back(VocStep{kOpDgrad, lbase + m, S.len, x, d, d, dst, kSlope, acc, 1.f});
                }
                d = dst;
            }
        }
        P.bwd.push_back(VocStep{kOpWgrad, 1 + i, S.len_in, S.in, DX, none, none, kSlope, 0, 1.f});
        P.bwd.push_back(VocStep{kOpDgrad, 1 + i, S.len_in, S.in, DX, none, G, kSlope, 0, i > 0 ? inv : 1.f});
    }
    P.bwd.push_back(VocStep{kOpWgrad, 0, (long)T, {kSpMel, 0}, G, none, none, 1.f, 0, 1.f});
    if (mel_grad) P.bwd.push_back(VocStep{kOpDgrad, 0, (long)T, none, G, none, {kSpDMel, 0}, 1.f, 0, 1.f});
    P.post_part_doubles = voc_post_part_doubles(B, P.L.back().cin, len);
    // five gradient buffers of the widest stage, the weight gradients' partial planes, conv_post's fp64 partial sums
    P.ws_floats = 5 * bf + P.part_floats + round4(2 * P.post_part_doubles);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// the executors: they only walk the plan's lists
// ------------------------------------------------------------------------------------------------------------------
struct VocBases { float* tape; float* ws; const float* mel; float* audio; const float* d_audio; float* d_mel; };
static float* voc_at(const VocBases& b, const VocRef& r) {
    switch (r.sp) {
        case kSpTape: return b.tape + r.off;
        case kSpWs: return b.ws + r.off;
        case kSpMel: return const_cast<float*>(b.mel);
        case kSpAudio: return b.audio;
        case kSpDAudio: return const_cast<float*>(b.d_audio);
        case kSpDMel: return b.d_mel;
        default: return nullptr;
    }
}

static int hifigan_forward_train(const t2_hifigan_config& c, const t2_hifigan_train_fwd_args& a, hipStream_t s) {
    HifiganTrainPlan P;
    T2_REQUIRE(a.n_mel == c.n_mel, "hifigan_forward_train: the mel has %d channels, the generator takes %d", a.n_mel, c.n_mel);
    T2_TRY_RC(hifigan_train_plan(c, a.B, a.T, false, &P));
    T2_REQUIRE(a.packed && a.mel && a.tape && a.audio, "hifigan_forward_train: null pointer");
    const VocBases bs{a.tape, nullptr, a.mel, a.audio, nullptr, nullptr};
    for (const VocStep& st : P.fwd) {
        const HifiganLayer& l = P.L[st.layer];
        if (st.op == kOpConv)
            T2_TRY_RC(voc_conv(VocConv{a.B, l.cin, l.cout, st.len, l.k, l.d, l.u, voc_at(bs, st.x), a.packed + l.w_off, a.packed + l.b_off, voc_at(bs, st.res),
                                       voc_at(bs, st.out), st.slope, st.accumulate, st.scale}, s));
        else
            T2_TRY_RC(voc_post(voc_at(bs, st.x), a.packed + l.w_off, a.packed + l.b_off, a.audio, nullptr, a.B, l.cin, st.len, nullptr, 0, 0, nullptr, s));
    }
    return 0;
}

static int hifigan_pack_backward(const t2_hifigan_config& c, const float* const* weights, int n_layers, float* packed_bwd, hipStream_t s) {
    HifiganTrainPlan P;
    T2_TRY_RC(hifigan_train_plan(c, 1, 1, false, &P));
    T2_REQUIRE(weights && packed_bwd, "hifigan_pack_backward: null pointer");
    T2_REQUIRE(n_layers == (int)P.L.size(), "hifigan_pack_backward: %d layers given, the configuration has %d", n_layers, (int)P.L.size());
    for (int i = 0; i < n_layers; ++i) {
        const HifiganLayer& l = P.L[i];
        T2_REQUIRE(weights[i], "hifigan_pack_backward: layer %d has a null weight", i);
        if (l.kind != 2) T2_TRY_RC(voc_dgrad_pack(weights[i], packed_bwd + P.bwd_off[i], l.cin, l.cout, l.k, l.u, s));
    }
    return 0;
}

static int hifigan_backward(const t2_hifigan_config& c, const t2_hifigan_bwd_args& a, hipStream_t s) {
    HifiganTrainPlan P;
    T2_REQUIRE(a.n_mel == c.n_mel, "hifigan_backward: the mel has %d channels, the generator takes %d", a.n_mel, c.n_mel);
    T2_TRY_RC(hifigan_train_plan(c, a.B, a.T, a.d_mel != nullptr, &P));
    T2_REQUIRE(a.packed && a.packed_bwd && a.mel && a.tape && a.audio && a.d_audio && a.workspace, "hifigan_backward: null pointer");
    T2_REQUIRE(a.grads || a.d_mel, "hifigan_backward: neither the weights' nor the mel's gradient is asked for");
    const VocBases bs{const_cast<float*>(a.tape), a.workspace, a.mel, const_cast<float*>(a.audio), a.d_audio, a.d_mel};
    float* part = a.workspace + 5 * P.base.buf_floats;
    double* post_part = reinterpret_cast<double*>(part + P.part_floats);
    for (const VocStep& st : P.bwd) {
        const HifiganLayer& l = P.L[st.layer];
        // without an arena (only the mel's gradient is asked for) the weight gradients are not launched; conv_post's kernel
        // computes its dw and db along the way, they land in the partial planes' scratch, which is then unused
        if (!a.grads && st.op == kOpWgrad) continue;
        float* dw = a.grads ? a.grads + P.gw_off[st.layer] : part;
        float* db = a.grads ? a.grads + P.gb_off[st.layer] : part + round4((size_t)l.cin * l.k);
        if (st.op == kOpPostBwd)
            T2_TRY_RC(voc_post_bwd(VocPostBwdCall{a.B, l.cin, st.len, voc_at(bs, st.x), a.packed + l.w_off, a.audio, a.d_audio, voc_at(bs, st.out), dw, db, post_part,
                                                  st.scale}, s));
        else if (st.op == kOpWgrad)
            T2_TRY_RC(voc_wgrad(VocWgradCall{a.B, l.cin, l.cout, st.len, l.k, l.d, l.u, voc_at(bs, st.x), voc_at(bs, st.dy), dw, db, part, st.slope}, s));
        else
            T2_TRY_RC(voc_dgrad(VocDgradCall{a.B, l.cin, l.cout, st.len, l.k, l.d, l.u, voc_at(bs, st.dy), a.packed_bwd + P.bwd_off[st.layer], voc_at(bs, st.x),
                                             voc_at(bs, st.res), voc_at(bs, st.out), st.slope, st.accumulate, st.scale}, s));
    }
    return 0;
}

}  // namespace t2

// ---- C ABI (include/t2amd.h)
using namespace t2;

extern "C" {

int t2_hifigan_train_plan(const t2_hifigan_config* cfg, int B, int T, t2_hifigan_train_plan_info* out) {
    T2_REQUIRE(cfg && out, "t2_hifigan_train_plan: null pointer");
    HifiganTrainPlan P;
    T2_TRY_RC(hifigan_train_plan(*cfg, B, T, true, &P));
    out->out_len = P.base.out_len;
    out->tape_bytes = P.tape_floats * sizeof(float); out->workspace_bytes = P.ws_floats * sizeof(float);
    out->packed_bytes = P.base.packed_bytes; out->packed_bwd_bytes = P.packed_bwd_floats * sizeof(float);
    out->grad_floats = P.grad_floats; out->part_bytes = P.part_floats * sizeof(float);
    out->n_layers = (int)P.L.size();
    out->n_forward_launches = (int)P.fwd.size(); out->n_backward_launches = 0;
    for (int i = 0; i < kOpCount; ++i) out->launches[i] = 0;
    for (const VocStep& st : P.fwd) ++out->launches[st.op];
    for (const VocStep& st : P.bwd) {
        ++out->launches[st.op];
        out->n_backward_launches += st.op == kOpDgrad ? 1 : 2;      // the weight gradient and conv_post's backward end in a reduce
    }
    return 0;
}
int t2_hifigan_grad_offsets(const t2_hifigan_config* cfg, size_t* w_offsets, size_t* b_offsets, int n_layers) {
    T2_REQUIRE(cfg && w_offsets && b_offsets, "t2_hifigan_grad_offsets: null pointer");
    HifiganTrainPlan P;
    T2_TRY_RC(hifigan_train_plan(*cfg, 1, 1, false, &P));
    T2_REQUIRE(n_layers == (int)P.L.size(), "t2_hifigan_grad_offsets: %d layers given, the configuration has %d", n_layers, (int)P.L.size());
    for (int i = 0; i < n_layers; ++i) { w_offsets[i] = P.gw_off[i]; b_offsets[i] = P.gb_off[i]; }
    return 0;
}
int t2_hifigan_pack_backward(const t2_hifigan_config* cfg, const float* const* weights_host, int n_layers, float* packed_bwd, void* stream) {
    T2_REQUIRE(cfg, "t2_hifigan_pack_backward: null configuration");
    return hifigan_pack_backward(*cfg, weights_host, n_layers, packed_bwd, (hipStream_t)stream);
}
int t2_hifigan_forward_train(const t2_hifigan_config* cfg, const t2_hifigan_train_fwd_args* a, void* stream) {
    T2_REQUIRE(cfg && a, "t2_hifigan_forward_train: null pointer");
    return hifigan_forward_train(*cfg, *a, (hipStream_t)stream);
}
int t2_hifigan_backward(const t2_hifigan_config* cfg, const t2_hifigan_bwd_args* a, void* stream) {
    T2_REQUIRE(cfg && a, "t2_hifigan_backward: null pointer");
    return hifigan_backward(*cfg, *a, (hipStream_t)stream);
}

size_t t2_vocoder_dgrad_packed_floats(int Cin, int Cout, int k, int u) { return voc_dgrad_packed_floats(Cin, Cout, k, u); }
static int vocoder_dgrad(const t2_vocoder_dgrad_args* a, int u, void* stream) {
    T2_REQUIRE(a->w && a->packed_ws, "t2_vocoder data gradient: null weights or packing scratch");
    const VocDgradCall c{a->B, a->Cin, a->Cout, (long)a->L, a->k, a->d, u, a->dy, a->packed_ws, a->x, a->residual, a->dx, a->slope, a->accumulate, a->scale};
    T2_TRY_RC(voc_dgrad_check(c));                  // refuse before anything is written, the pack included
    T2_TRY_RC(voc_dgrad_pack(a->w, a->packed_ws, a->Cin, a->Cout, a->k, u, (hipStream_t)stream));
    return voc_dgrad(c, (hipStream_t)stream);
}
int t2_vocoder_conv1d_dgrad(const t2_vocoder_dgrad_args* a, void* stream) {
    T2_REQUIRE(a, "t2_vocoder_conv1d_dgrad: null arguments");
    T2_REQUIRE(a->u == 0, "t2_vocoder_conv1d_dgrad: stride u=%d given, a Conv1d has none", a->u);
    return vocoder_dgrad(a, 0, stream);
}
int t2_vocoder_conv_transpose1d_dgrad(const t2_vocoder_dgrad_args* a, void* stream) {
    T2_REQUIRE(a, "t2_vocoder_conv_transpose1d_dgrad: null arguments");
    T2_REQUIRE(a->u >= 1, "t2_vocoder_conv_transpose1d_dgrad: stride u=%d must be positive", a->u);
    return vocoder_dgrad(a, a->u, stream);
}
size_t t2_vocoder_wgrad_part_floats(int B, int Cin, int Cout, int L, int k, int d, int u) {
    return voc_wgrad_part_floats(B, Cin, Cout, L, k, u ? 1 : d, u);
}
int t2_vocoder_wgrad(const t2_vocoder_wgrad_args* a, void* stream) {
    T2_REQUIRE(a, "t2_vocoder_wgrad: null arguments");
    T2_REQUIRE(a->u >= 0, "t2_vocoder_wgrad: stride u=%d must not be negative", a->u);
    return voc_wgrad(VocWgradCall{a->B, a->Cin, a->Cout, (long)a->L, a->k, a->u ? 1 : a->d, a->u, a->x, a->dy, a->dw, a->db, a->part, a->slope}, (hipStream_t)stream);
}
size_t t2_vocoder_post_part_doubles(int B, int C, int L) { return voc_post_part_doubles(B, C, L); }
int t2_vocoder_post_backward(const t2_vocoder_post_bwd_args* a, void* stream) {
    T2_REQUIRE(a, "t2_vocoder_post_backward: null arguments");
    return voc_post_bwd(VocPostBwdCall{a->B, a->C, (long)a->L, a->x, a->w, a->audio, a->d_audio, a->dx, a->dw, a->db, a->part, a->scale}, (hipStream_t)stream);
}

}  // extern "C"
