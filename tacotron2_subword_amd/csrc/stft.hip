// STFT analysis and synthesis.  Replaces the reference's stft.py: STFT.transform (:77-105) and STFT.inverse (:107-136) with
// audio_processing.py: window_sumsquare (:7-56), and the element-wise middle of bias_remover.py: hifiganBiasRemover.forward
// (:31-36).
//
// Tensors keep torch's [B, C, frames] layout with time contiguous.  Arithmetic is exact fp32 on the matrix cores
// (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain), whatever t2_set_precision says.  Both kernels are GEMMs of one shape:
// one operand is a table packed once into the order the lanes consume it (four k-steps per 16-byte load, zero-padded to whole
// tiles), the other is staged per chunk of 32 k in an LDS slab whose loader does the element-wise work.  A wave owns one
// 32 x 32 accumulator; the waves of a workgroup share the slab.
//
// Analysis:  Y[c][f] = sum_k basis[c][k] * xpad[f*hop + k]  (M = 2*(N/2+1) basis rows, columns = frames, K = N).
//   The loader reads the waveform itself: xpad[i] = x[reflect(i - N/2)] is index arithmetic, there is no padded copy and no
//   frame matrix.  A 32-row tile holds 16 bins, real rows and imaginary rows interleaved in groups of 8, so that a lane's
//   accumulator holds re and im of the same (bin, frame) and the epilogue can write magnitude and phase too.
// Synthesis: overlap-add as a GEMM, no atomics.  With R = N/hop and output sample t = q*hop + r,
//   y[q*hop + r] = sum_{j<R} sum_c X[c][q-j] * inv[c][j*hop + r],  X zero outside [0, nf):
//   rows = q, columns = r, K = R * 2*(N/2+1).  Per chunk of 16 bins the slab holds (re, im) of frames q0-(R-1) .. q0+31 and
//   every overlap j reads it at a shifted column, so X is formed once per chunk: from (magnitude, phase) with sincosf, or from
//   (re, im) with the bias remover's gain  g = max(|z| - strength*bias, 0) / |z|.  The epilogue divides by the window
//   sum-square envelope where it exceeds FLT_MIN, scales by N/hop and writes only the samples the reference keeps.
// The order of every sum is fixed: same bits from run to run and for an item alone or in a batch.  Offsets are 64-bit.
// Per-item counts (padded batches): the analysis takes sample counts n_b (its own reflection, 1 + n_b/hop frames, none where
// n_b <= N/2), the synthesis frame counts nf_b (loads, envelope and hop*(nf_b - 1) samples bounded by it).  Strides and tiles
// stay those of the padded tensors, so an item has the bits of its run alone; behind an item's count the outputs are zeros,
// and a tile wholly behind it runs no chunk.  The counts are read in the kernels only and clamped to the row.
#include <cfloat>

#include "kernels.h"

namespace t2 {

constexpr int kStftKC = 32;                                   // k per slab
constexpr int kStftAnaStride = kStftTile + 1;                 // odd: the loader's lanes run along k, one bank each
constexpr int kStftSynStride = kStftTile + kStftMaxOverlap + 1;
static_assert(kStftSynStride >= kStftTile + kStftMaxOverlap - 1, "the slab holds the frames of every overlap");

struct StftAna {
    const float* x; const float* pf; float* re; float* im; float* mag; float* phase;
    long n; int nf, N, hop, cutoff, bin_tiles, kchunks;
    const int32_t* lens; int32_t* nf_out;                      // nullable: per-item sample counts (clamped to [0, n]) and the frame counts they give
};

__global__ void __launch_bounds__(256) stft_analysis_kernel(StftAna p) {
    __shared__ float slab[kStftKC * kStftAnaStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hk = lane >> 5;
    const int mt = blockIdx.y * 4 + wave;
    const bool active = mt < p.bin_tiles;                      // uniform over the wave
    const int b = blockIdx.z;
    const long f0 = (long)blockIdx.x * kStftTile;
    const float* xb = p.x + (size_t)b * p.n;
    const f32x4* pf = reinterpret_cast<const f32x4*>(p.pf) + (size_t)(active ? mt : 0) * p.kchunks * 256;
    const int half = p.N / 2;
    // the item's own samples and frames: rows keep the stride n and the planes the stride nf, the reflection and the frame bound
    // are the item's.  A row of <= N/2 samples, where the reflect pad is undefined, has no frames
    long n = p.n;
    int nf = p.nf;
    if (p.lens) {
        const int l = p.lens[b];
        n = l < 0 ? 0 : (l > p.n ? p.n : (long)l);
        nf = n > half ? 1 + (int)(n / p.hop) : 0;
        if (p.nf_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.nf_out[b] = nf;
    }
    f32x16 acc = {0};

    // a tile wholly behind the item's frames stages nothing and writes zeros: uniform over the workgroup
    for (int c = 0; c < (f0 < nf ? p.kchunks : 0); ++c) {
        if (c) __syncthreads();                                // every wave is done reading the previous slab
        const int kl = threadIdx.x & 31, k = c * kStftKC + kl;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int fl = (threadIdx.x >> 5) + 8 * i;
            const long f = f0 + fl;
            float v = 0.f;
            if (f < nf && k < p.N) {
                long t = f * p.hop + k - half;                 // reflect padding: n > N/2 keeps both mirrors inside [0, n)
                if (t < 0) t = -t;
                else if (t >= n) t = 2 * (n - 1) - t;
                v = xb[t];
            }
            slab[kl * kStftAnaStride + fl] = v;
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 a = pf[(size_t)c * 256 + g * 64 + lane];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], slab[(8 * g + 2 * i + hk) * kStftAnaStride + (lane & 31)], acc, 0, 0, 0);
            }
        }
    }
    if (!active) return;
    // lane holds frame lane & 31 and tile rows (e&3) + 8*(e>>2) + 4*hk; row r is part (r>>3)&1 of bin 8*(r>>4) + (r&7):
    // element e (bit 2 clear) is re, e + 4 is im of bin 8*(e>>3) + 4*hk + (e&3)
    const long f = f0 + (lane & 31);
    if (f >= p.nf) return;
    const bool inside = f < nf;                                // frames at or past the item's count read as exact zeros
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int bin = mt * 16 + 8 * h + 4 * hk + i;
            if (bin >= p.cutoff) continue;
            const size_t o = ((size_t)b * p.cutoff + bin) * p.nf + f;
            const float re = inside ? acc[8 * h + i] : 0.f, im = inside ? acc[8 * h + i + 4] : 0.f;
            if (p.re) p.re[o] = re;
            if (p.im) p.im[o] = im;
            if (p.mag) p.mag[o] = inside ? sqrtf(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im))) : 0.f;   // torch.sqrt(re**2 + im**2), no contraction
            if (p.phase) p.phase[o] = inside ? atan2f(im, re) : 0.f;
        }
    }
}

struct StftSyn {
    const float* a; const float* b; const float* bias; const float* pi; const double* wsq; float* y;
    int nf, N, hop, R, cutoff, nchunks, col_tiles, mode, windowed;
    long qbase, out_len;
    float strength, scale;
    const int32_t* nfs; int32_t* len_out;                      // nullable: per-item frame counts (clamped to [0, nf]) and the sample counts they give
    const int32_t* lens; long n, row; int pad;                 // RAW: nullable per-item sample counts (clamped to [0, n]), the stride n + 2*pad of y's rows
};

// RAW (the analysis' backward, stft_analysis_backward): a = d_re, b = d_im taken as they are (a null plane reads as zeros),
// the basis table is the forward one, and y is the gradient of the padded signal, dxpad[b][q*hop + r] for every sample that a
// frame of the item covers: no envelope, no scale, no trim.  The item's frames follow from its sample count.
template <int WN, bool RAW>
__global__ void __launch_bounds__(WN * 64) stft_synthesis_kernel(StftSyn p) {
    __shared__ float slab[kStftKC * kStftSynStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hk = lane >> 5;
    const int ct = blockIdx.y * WN + wave;
    const bool active = ct < p.col_tiles;                      // uniform over the wave
    const int bi = blockIdx.z;
    const long q0 = p.qbase + (long)blockIdx.x * kStftTile;
    const long fbase = q0 - (p.R - 1);                         // frame of slab column 0
    const int W = kStftTile + p.R - 1;
    const float* pa = p.a + (size_t)bi * p.cutoff * p.nf;
    const float* pb = p.b + (size_t)bi * p.cutoff * p.nf;
    const f32x4* pi = reinterpret_cast<const f32x4*>(p.pi) + (size_t)(active ? ct : 0) * p.nchunks * p.R * 256;
    // the item's own frames: the planes keep the stride nf and the output the stride out_len, the loads, the envelope and the
    // samples written are bounded by the item's count
    int nf = p.nf;
    long out_len = p.out_len;
    if constexpr (RAW) {
        long len = p.n;
        if (p.lens) {
            const int l = p.lens[bi];
            len = l < 0 ? 0 : (l > p.n ? p.n : (long)l);
        }
        nf = (int)mel_frames(len, p.N, p.hop, p.pad);
        out_len = nf >= 1 ? (long)p.hop * (nf - 1) + p.N : 0;  // padded samples under a frame
    } else if (p.nfs) {
        const int l = p.nfs[bi];
        nf = l < 0 ? 0 : (l > p.nf ? p.nf : l);
        out_len = nf >= 1 ? (long)p.hop * (nf - 1) : 0;
        if (p.len_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.len_out[bi] = (int32_t)out_len;
    }
    f32x16 acc = {0};

    // a tile whose first sample lies behind the item's end stages nothing and writes zeros: uniform over the workgroup
    for (int c = 0; c < (q0 * p.hop - (RAW ? 0 : p.N / 2) < out_len ? p.nchunks : 0); ++c) {
        if (c) __syncthreads();
        for (int item = threadIdx.x; item < 16 * W; item += WN * 64) {
            const int bl = item / W, col = item - bl * W;
            const int bin = c * 16 + bl;
            const long f = fbase + col;
            float xr = 0.f, xi = 0.f;
            if (bin < p.cutoff && f >= 0 && f < nf) {
                const size_t o = (size_t)bin * p.nf + f;
                const float u = RAW && !p.a ? 0.f : pa[o], v = RAW && !p.b ? 0.f : pb[o];
                if constexpr (RAW) {
                    xr = u; xi = v;
                } else if (p.mode == 0) {                             // polar: u = magnitude, v = phase
                    float sn, cs;
                    sincosf(v, &sn, &cs);
                    xr = u * cs; xi = u * sn;
                } else {                                       // denoise: u = re, v = im
                    const float m = sqrtf(__fadd_rn(__fmul_rn(u, u), __fmul_rn(v, v)));
                    const float d = fmaxf(__fsub_rn(m, __fmul_rn(p.bias[bin], p.strength)), 0.f);
                    const float g = m > 0.f ? d / m : 0.f;
                    xr = g * u; xi = g * v;
                }
            }
            slab[(2 * bl) * kStftSynStride + col] = xr;
            slab[(2 * bl + 1) * kStftSynStride + col] = xi;
        }
        __syncthreads();
        if (active) {
            for (int j = 0; j < p.R; ++j) {
                const f32x4* pj = pi + ((size_t)c * p.R + j) * 256 + lane;
                const float* sj = slab + hk * kStftSynStride + (lane & 31) + p.R - 1 - j;   // row q reads frame q - j
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 w = pj[g * 64];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sj[(8 * g + 2 * i) * kStftSynStride], w[i], acc, 0, 0, 0);
                }
            }
        }
    }
    if (!active) return;
    const int r = ct * 32 + (lane & 31);
    if (r >= p.hop) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const long q = q0 + (e & 3) + 8 * (e >> 2) + 4 * hk;
        if constexpr (RAW) {
            const long tp = q * p.hop + r;
            if (tp < out_len) p.y[(size_t)bi * p.row + tp] = acc[e];
            continue;
        }
        const long t = q * p.hop + r, o = t - p.N / 2;          // stft.py:133-134: N/2 samples dropped at each end
        if (o < 0 || o >= p.out_len) continue;
        float v = acc[e];
        if (o >= out_len) v = 0.f;                             // behind the item's own end
        else if (p.windowed) {
            // window_sumsquare: frames i*hop <= t < i*hop + N in ascending order, each "+=" a float64 add rounded to float32
            const long lo = q - (p.R - 1) > 0 ? q - (p.R - 1) : 0, hi = q < nf - 1 ? q : nf - 1;
            float env = 0.f;
            for (long i = lo; i <= hi; ++i) env = (float)((double)env + p.wsq[t - i * p.hop]);
            if (env > FLT_MIN) v = v / env;                    // tiny(window_sum), stft.py:123-128
            v *= p.scale;
        }
        p.y[(size_t)bi * p.out_len + o] = v;
    }
}

// forward:  [bin_tile][chunk][g][lane][i] = fwd[part*cutoff + bin][k],  row r = lane & 31: part = (r>>3)&1,
//           bin = 16*bin_tile + 8*(r>>4) + (r&7),  k = 32*chunk + 8*g + 2*i + (lane>>5)
__global__ void __launch_bounds__(256) stft_pack_fwd_kernel(const float* __restrict__ fwd, float* __restrict__ out, int N, int cutoff, int kchunks, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int i = idx & 3, lane = (idx >> 2) & 63, g = (idx >> 8) & 3;
    const size_t rest = idx >> 10;
    const int c = (int)(rest % kchunks), mt = (int)(rest / kchunks);
    const int r = lane & 31, part = (r >> 3) & 1, bin = mt * 16 + 8 * (r >> 4) + (r & 7);
    const int k = c * kStftKC + 8 * g + 2 * i + (lane >> 5);
    out[idx] = (bin < cutoff && k < N) ? fwd[((size_t)part * cutoff + bin) * N + k] : 0.f;
}

// inverse:  [col_tile][chunk][j][g][lane][i] = inv[part*cutoff + bin][j*hop + r],  kk = 8*g + 2*i + (lane>>5): bin = 16*chunk + kk/2,
//           part = kk & 1,  r = 32*col_tile + (lane & 31)
__global__ void __launch_bounds__(256) stft_pack_inv_kernel(const float* __restrict__ inv, float* __restrict__ out, int N, int hop, int cutoff, int nchunks, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int R = N / hop;
    const int i = idx & 3, lane = (idx >> 2) & 63, g = (idx >> 8) & 3;
    size_t rest = idx >> 10;
    const int j = (int)(rest % R); rest /= R;
    const int c = (int)(rest % nchunks), ct = (int)(rest / nchunks);
    const int kk = 8 * g + 2 * i + (lane >> 5), bin = c * 16 + (kk >> 1), part = kk & 1;
    const int r = ct * 32 + (lane & 31);
    out[idx] = (bin < cutoff && r < hop) ? inv[((size_t)part * cutoff + bin) * N + (size_t)j * hop + r] : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------
int stft_plan(int N, int hop, int nf, StftPlan* out) {
    T2_REQUIRE(out, "stft: null plan");
    T2_REQUIRE(N >= 2 && N <= kStftMaxN, "stft: filter_length=%d outside 2..%d", N, kStftMaxN);
    T2_REQUIRE(N % 2 == 0, "stft: filter_length=%d is odd: the reflect padding and the trim take N/2 samples per side", N);
    T2_REQUIRE(hop >= 1 && hop <= N, "stft: hop_length=%d outside 1..filter_length=%d", hop, N);
    T2_REQUIRE(N % hop == 0, "stft: filter_length=%d is not a multiple of hop_length=%d: the overlap-add GEMM needs whole overlaps", N, hop);
    T2_REQUIRE(N / hop <= kStftMaxOverlap, "stft: filter_length=%d over hop_length=%d is %d overlaps, at most %d", N, hop, N / hop, kStftMaxOverlap);
    T2_REQUIRE(nf >= 1 && nf <= INT32_MAX / 2 / hop, "stft: %d frames outside 1..%d at hop_length=%d", nf, INT32_MAX / 2 / hop, hop);
    StftPlan p;
    p.cutoff = N / 2 + 1;
    p.overlap = N / hop;
    p.bin_tiles = (p.cutoff + 15) / 16;
    p.kchunks = (N + kStftKC - 1) / kStftKC;
    p.col_tiles = (hop + 31) / 32;
    p.out_len = (long)hop * (nf - 1);
    p.fwd_floats = (size_t)p.bin_tiles * p.kchunks * 1024;
    p.inv_floats = (size_t)p.col_tiles * p.bin_tiles * p.overlap * 1024;
    p.wsq_floats = (size_t)(2 * N + 3) / 4 * 4;
    *out = p;
    return 0;
}

int stft_pack_forward(int N, const float* fwd, float* packed, hipStream_t s) {
    StftPlan pl;
    T2_TRY_RC(stft_plan(N, N, 1, &pl));                         // the forward table does not depend on the hop
    T2_REQUIRE(fwd && packed, "stft_pack_forward: null pointer");
    hipLaunchKernelGGL(stft_pack_fwd_kernel, dim3((unsigned)((pl.fwd_floats + 255) / 256)), dim3(256), 0, s, fwd, packed, N, pl.cutoff, pl.kchunks, pl.fwd_floats);
    T2_LAUNCH_CHECK();
    return 0;
}

int stft_pack_overlap(int N, int hop, const float* basis, float* packed, hipStream_t s) {
    StftPlan pl;
    T2_TRY_RC(stft_plan(N, hop, 1, &pl));
    T2_REQUIRE(basis && packed, "stft_pack_overlap: null pointer");
    hipLaunchKernelGGL(stft_pack_inv_kernel, dim3((unsigned)((pl.inv_floats + 255) / 256)), dim3(256), 0, s, basis, packed, N, hop, pl.cutoff, pl.bin_tiles,
                       pl.inv_floats);
    T2_LAUNCH_CHECK();
    return 0;
}

// fwd, inv: the windowed bases [2*(N/2+1)][N] (the module's buffers without their middle dimension); wsq: the squared,
// centre-padded window [N] in fp64, nullable (no window: synthesis must then run with windowed = 0)
static int stft_pack(int N, int hop, const float* fwd, const float* inv, const double* wsq, float* packed, hipStream_t s) {
    StftPlan pl;
    T2_TRY_RC(stft_plan(N, hop, 1, &pl));
    T2_REQUIRE(fwd && inv && packed, "stft_pack: null pointer");
    T2_TRY_RC(stft_pack_forward(N, fwd, packed, s));
    T2_TRY_RC(stft_pack_overlap(N, hop, inv, packed + pl.fwd_floats, s));
    float* w = packed + pl.fwd_floats + pl.inv_floats;
    if (wsq) T2_CHECK_HIP(hipMemcpyAsync(w, wsq, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, s));
    else T2_CHECK_HIP(hipMemsetAsync(w, 0, pl.wsq_floats * sizeof(float), s));
    return 0;
}

// x [B, n] -> re, im, mag, phase [B, N/2+1, 1 + n/hop], each nullable
// lengths (nullable, device [B]): per-item sample counts, clamped to [0, n] in the kernel.  Item b is then x[b, :lengths[b]] alone:
// its own reflection, 1 + lengths[b]/hop frames (none where lengths[b] <= N/2), zeros in the planes behind them; frame_lengths
// (nullable) receives the counts
static int stft_analysis(const t2_stft_analysis_args& a, const int32_t* lengths, int32_t* frame_lengths, hipStream_t s) {
    T2_REQUIRE(a.B >= 1 && a.B <= 65535, "stft analysis: B=%d outside 1..65535", a.B);
    T2_REQUIRE(lengths || !frame_lengths, "stft analysis: frame counts asked for without sample counts");
    T2_REQUIRE(a.N >= 2 && a.N % 2 == 0, "stft analysis: filter_length=%d must be even", a.N);
    T2_REQUIRE(a.n > a.N / 2, "stft analysis: Padding size should be less than the corresponding input dimension, but got: padding (%d, %d) at dimension 1 "
               "of a signal of %ld samples", a.N / 2, a.N / 2, a.n);
    T2_REQUIRE(a.hop >= 1 && a.n / a.hop < INT32_MAX / 2 / a.hop, "stft analysis: %ld samples at hop_length=%d exceed the limit of %d per row", a.n, a.hop, INT32_MAX / 2);
    const int nf = 1 + (int)(a.n / a.hop);
    StftPlan pl;
    T2_TRY_RC(stft_plan(a.N, a.hop, nf, &pl));
    T2_REQUIRE(a.x && a.packed, "stft analysis: null pointer");
    T2_REQUIRE(a.re || a.im || a.mag || a.phase, "stft analysis: no output requested");
    StftAna p;
    p.x = a.x; p.pf = a.packed; p.re = a.re; p.im = a.im; p.mag = a.mag; p.phase = a.phase;
    p.n = a.n; p.nf = nf; p.N = a.N; p.hop = a.hop; p.cutoff = pl.cutoff; p.bin_tiles = pl.bin_tiles; p.kchunks = pl.kchunks;
    p.lens = lengths; p.nf_out = frame_lengths;
    dim3 grid((unsigned)((nf + kStftTile - 1) / kStftTile), (unsigned)((pl.bin_tiles + 3) / 4), (unsigned)a.B);
    hipLaunchKernelGGL(stft_analysis_kernel, grid, dim3(256), 0, s, p);
    T2_LAUNCH_CHECK();
    return 0;
}

// a, b [B, N/2+1, nf] -> y [B, 1, hop*(nf-1)]; modes and windowed as t2amd.h states them.
// frame_lengths (nullable, device [B]): per-item frame counts, clamped to [0, nf] in the kernel.  Item b is then its first
// frame_lengths[b] frames alone; y is zero from hop*(frame_lengths[b]-1) on (from 0 for a count below 1), which sample_lengths
// (nullable) receives
static int stft_synthesis(const t2_stft_synthesis_args& a, const int32_t* frame_lengths, int32_t* sample_lengths, hipStream_t s) {
    T2_REQUIRE(a.B >= 1 && a.B <= 65535, "stft synthesis: B=%d outside 1..65535", a.B);
    StftPlan pl;
    T2_TRY_RC(stft_plan(a.N, a.hop, a.nf, &pl));
    T2_REQUIRE(a.mode == T2_STFT_POLAR || a.mode == T2_STFT_DENOISE, "stft synthesis: mode %d is neither polar (0) nor denoise (1)", a.mode);
    T2_REQUIRE(a.a && a.b && a.packed, "stft synthesis: null pointer");
    T2_REQUIRE(a.mode == T2_STFT_POLAR || a.bias, "stft synthesis: the denoise mode needs the bias spectrum");
    T2_REQUIRE(frame_lengths || !sample_lengths, "stft synthesis: sample counts asked for without frame counts");
    if (pl.out_len == 0) {                                     // a single frame: everything falls into the trimmed margins
        if (sample_lengths) T2_CHECK_HIP(hipMemsetAsync(sample_lengths, 0, (size_t)a.B * sizeof(int32_t), s));
        return 0;
    }
    T2_REQUIRE(a.y, "stft synthesis: null output");
    StftSyn p;
    p.a = a.a; p.b = a.b; p.bias = a.bias; p.pi = a.packed + pl.fwd_floats; p.y = a.y;
    p.wsq = reinterpret_cast<const double*>(a.packed + pl.fwd_floats + pl.inv_floats);
    p.nf = a.nf; p.N = a.N; p.hop = a.hop; p.R = pl.overlap; p.cutoff = pl.cutoff; p.nchunks = pl.bin_tiles; p.col_tiles = pl.col_tiles;
    p.mode = a.mode; p.windowed = a.windowed != 0;
    p.qbase = (a.N / 2) / a.hop; p.out_len = pl.out_len;
    p.strength = a.strength; p.scale = (float)a.N / (float)a.hop;
    p.nfs = frame_lengths; p.len_out = sample_lengths;
    p.lens = nullptr; p.n = 0; p.row = 0; p.pad = 0;
    const long qlast = (a.N / 2 + pl.out_len - 1) / a.hop;
    const int wn = pl.col_tiles >= 8 ? 8 : (pl.col_tiles >= 4 ? 4 : (pl.col_tiles >= 2 ? 2 : 1));
    dim3 grid((unsigned)((qlast - p.qbase) / kStftTile + 1), (unsigned)((pl.col_tiles + wn - 1) / wn), (unsigned)a.B);
    if (wn == 8) hipLaunchKernelGGL((stft_synthesis_kernel<8, false>), grid, dim3(512), 0, s, p);
    else if (wn == 4) hipLaunchKernelGGL((stft_synthesis_kernel<4, false>), grid, dim3(256), 0, s, p);
    else if (wn == 2) hipLaunchKernelGGL((stft_synthesis_kernel<2, false>), grid, dim3(128), 0, s, p);
    else hipLaunchKernelGGL((stft_synthesis_kernel<1, false>), grid, dim3(64), 0, s, p);
    T2_LAUNCH_CHECK();
    return 0;
}

// dx[b][i] = dxpad[pad + i] + [1 <= i <= pad] dxpad[pad - i] + [L-1-pad <= i <= L-2] dxpad[pad + 2(L-1) - i] for i < L = the item's
// length, three rounded adds in that order; zero from L on.  dxpad holds nothing behind the item's last frame: zero there.
struct StftFold { const float* dxpad; float* dx; const int32_t* lens; long n, row; int N, hop, pad; };

__global__ void __launch_bounds__(256) stft_fold_kernel(StftFold p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int b = blockIdx.y;
    long L = p.n;
    if (p.lens) {
        const int l = p.lens[b];
        L = l < 0 ? 0 : (l > p.n ? p.n : (long)l);
    }
    const long nf = mel_frames(L, p.N, p.hop, p.pad);
    const long covered = nf >= 1 ? (long)p.hop * (nf - 1) + p.N : 0;
    const float* src = p.dxpad + (size_t)b * p.row;
    auto at = [&](long t) { return t < covered ? src[t] : 0.f; };
    float v = 0.f;
    if (i < L && nf >= 1) {
#pragma clang fp contract(off)
        v = at(p.pad + i);
        if (i >= 1 && i <= p.pad) v = v + at(p.pad - i);
        if (i >= L - 1 - p.pad && i <= L - 2) v = v + at(p.pad + 2 * (L - 1) - i);
    }
    p.dx[(size_t)b * p.n + i] = v;
}

int stft_analysis_backward(const t2_stft_analysis_backward_args& a, int pad, hipStream_t s) {
    T2_REQUIRE(a.B >= 1 && a.B <= 65535, "stft analysis backward: B=%d outside 1..65535", a.B);
    T2_REQUIRE(a.hop >= 1 && a.N >= 2 && a.N % 2 == 0, "stft analysis backward: filter_length=%d must be even and hop_length=%d positive", a.N, a.hop);
    T2_REQUIRE(pad >= 0 && pad <= a.N / 2, "stft analysis backward: pad=%d outside 0..filter_length/2=%d", pad, a.N / 2);
    T2_REQUIRE(a.n > pad && a.n + 2L * pad >= a.N && a.n <= INT32_MAX / 2, "stft analysis backward: n=%ld samples with pad=%d per side outside what filter_length=%d takes",
               a.n, pad, a.N);
    const long nf = (a.n + 2L * pad - a.N) / a.hop + 1;
    T2_REQUIRE(nf <= INT32_MAX / 2 / a.hop, "stft analysis backward: %ld frames exceed the limit at hop_length=%d", nf, a.hop);
    StftPlan pl;
    T2_TRY_RC(stft_plan(a.N, a.hop, (int)nf, &pl));
    T2_REQUIRE((a.d_re || a.d_im) && a.basis_table && a.dxpad && a.dx, "stft analysis backward: null pointer");
    StftSyn p{};
    p.a = a.d_re; p.b = a.d_im; p.pi = a.basis_table; p.y = a.dxpad;
    p.nf = (int)nf; p.N = a.N; p.hop = a.hop; p.R = pl.overlap; p.cutoff = pl.cutoff; p.nchunks = pl.bin_tiles; p.col_tiles = pl.col_tiles;
    p.qbase = 0; p.out_len = 0;
    p.lens = a.lengths; p.n = a.n; p.row = a.n + 2L * pad; p.pad = pad;
    const int wn = stft_backward_wave_cols(pl.col_tiles);
    dim3 grid((unsigned)((nf - 1 + pl.overlap + kStftTile - 1) / kStftTile), (unsigned)((pl.col_tiles + wn - 1) / wn), (unsigned)a.B);
    if (wn == 8) hipLaunchKernelGGL((stft_synthesis_kernel<8, true>), grid, dim3(512), 0, s, p);
    else if (wn == 4) hipLaunchKernelGGL((stft_synthesis_kernel<4, true>), grid, dim3(256), 0, s, p);
    else if (wn == 2) hipLaunchKernelGGL((stft_synthesis_kernel<2, true>), grid, dim3(128), 0, s, p);
    else hipLaunchKernelGGL((stft_synthesis_kernel<1, true>), grid, dim3(64), 0, s, p);
    T2_LAUNCH_CHECK();
    StftFold f{a.dxpad, a.dx, a.lengths, a.n, p.row, a.N, a.hop, pad};
    hipLaunchKernelGGL(stft_fold_kernel, dim3((unsigned)((a.n + 255) / 256), (unsigned)a.B), dim3(256), 0, s, f);
    T2_LAUNCH_CHECK();
    return 0;
}

}  // namespace t2

// ---- C ABI (include/t2amd.h)
using namespace t2;
static_assert(T2_STFT_FRAME_TILE == kStftTile, "t2amd.h mirrors the STFT frame tile");

extern "C" {

int t2_stft_plan(int N, int hop, int nf, t2_stft_plan_info* out) {
    T2_REQUIRE(out, "t2_stft_plan: null pointer");
    StftPlan p;
    T2_TRY_RC(stft_plan(N, hop, nf, &p));
    out->bins = p.cutoff; out->overlap = p.overlap; out->frame_tile = kStftTile; out->bin_tile = 16; out->out_len = p.out_len;
    out->fwd_floats = p.fwd_floats; out->inv_floats = p.inv_floats; out->wsq_floats = p.wsq_floats;
    out->packed_bytes = (p.fwd_floats + p.inv_floats + p.wsq_floats) * sizeof(float);
    return 0;
}
int t2_stft_pack(int N, int hop, const float* forward_basis, const float* inverse_basis, const double* window_sq, float* packed, void* stream) {
    return stft_pack(N, hop, forward_basis, inverse_basis, window_sq, packed, (hipStream_t)stream);
}
int t2_stft_analysis(const t2_stft_analysis_args* a, void* stream) {
    T2_REQUIRE(a, "t2_stft_analysis: null arguments");
    return stft_analysis(*a, nullptr, nullptr, (hipStream_t)stream);
}
int t2_stft_analysis_ragged(const t2_stft_analysis_ragged_args* a, void* stream) {
    T2_REQUIRE(a, "t2_stft_analysis_ragged: null arguments");
    T2_REQUIRE(a->lengths, "t2_stft_analysis_ragged: null lengths (t2_stft_analysis is the call without them)");
    t2_stft_analysis_args p{};
    p.B = a->B; p.N = a->N; p.hop = a->hop; p.n = a->n; p.x = a->x; p.packed = a->packed;
    p.re = a->re; p.im = a->im; p.mag = a->mag; p.phase = a->phase;
    return stft_analysis(p, a->lengths, a->frame_lengths, (hipStream_t)stream);
}
int t2_stft_synthesis(const t2_stft_synthesis_args* a, void* stream) {
    T2_REQUIRE(a, "t2_stft_synthesis: null arguments");
    return stft_synthesis(*a, nullptr, nullptr, (hipStream_t)stream);
}
int t2_stft_synthesis_ragged(const t2_stft_synthesis_ragged_args* a, void* stream) {
    T2_REQUIRE(a, "t2_stft_synthesis_ragged: null arguments");
    T2_REQUIRE(a->frame_lengths, "t2_stft_synthesis_ragged: null frame counts (t2_stft_synthesis is the call without them)");
    t2_stft_synthesis_args p{};
    p.B = a->B; p.N = a->N; p.hop = a->hop; p.nf = a->nf; p.mode = a->mode; p.windowed = a->windowed;
    p.a = a->a; p.b = a->b; p.bias = a->bias; p.strength = a->strength; p.packed = a->packed; p.y = a->y;
    return stft_synthesis(p, a->frame_lengths, a->sample_lengths, (hipStream_t)stream);
}
int t2_stft_analysis_backward(const t2_stft_analysis_backward_args* a, void* stream) {
    T2_REQUIRE(a, "t2_stft_analysis_backward: null arguments");
    return stft_analysis_backward(*a, a->N / 2, (hipStream_t)stream);
}

}  // extern "C"
