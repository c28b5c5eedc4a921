// HiFi-GAN multi-period discriminator: forward and backward of hifigan_infer/hifigan_model.py: DiscriminatorP.forward (:141-160),
// which the reference runs as six Conv2d with (k, 1) kernels and leaves to torch's autograd.  Exact fp32 on the matrix cores
// (v_mfma_f32_32x32x2_f32), whatever t2_set_precision says; no atomics, every sum in a fixed order, partial sums added ascending
// in fp64: the same bits from run to run, and an item has the same bits alone or in a batch.  Element offsets are 64-bit.
//
// Activations keep torch's layout [B][C][H][p], so a feature map is returned as it is.  The p columns never mix: conv i is a 1-D
// convolution along H for every column, and as a GEMM it has M = Cout, K = Cin * taps and N = the H' * p flattened positions
// (h', w) of one item.  Output column n = h' * p + w reads the input's flat index (s * h' + j - lo) * p + w; the zero padding
// along H is exactly "outside [0, H * p)", so slab_stage serves with a wider row: the inputs of one 128-column tile for all taps
// are one contiguous run of at most s * (126 + p) + 5 * p floats.  A tile spans columns of different w: at 8192 samples the
// 1024-wide layers hold 10..51 rows per column but 102..110 positions per item.
//
//   disc_gemm_kernel        the four GEMM-shaped convs forward (bias, then leaky ReLU 0.1; the feature map is also the tape: its
//                           sign gives lrelu' in the backward, slope > 0, and at exactly 0 torch's rule x > 0 ? 1 : slope), and
//                           their data gradients dPre_l = lrelu'(fmap_l) * (g_fmap_l + W^T dPre_{l+1}).  Stride 1: the forward
//                           with M and K swapped and the taps flipped.  Stride 3, polyphase: input row h = 3 * q + phase
//                           receives only the taps j = h + 2 (mod 3), one or two per phase, at h' = q and q + 1, so every
//                           phase is a stride-1 GEMM of its own over a contiguous run of dPre_{l+1}; its outputs land three
//                           rows apart.  No zero-stuffed tensor, every element written once.
//   disc_first_kernel       conv 0 (1 -> 32 channels), bound by memory: one thread per position, the reflect padding as index
//                           arithmetic on the item's own T; no padded copy of the audio.
//   disc_first_bwd_kernel   its data gradient, a gather: sample t collects from its own position and from the padded position
//                           that mirrors onto it.
//   disc_post_kernel        conv_post (Cout = 1, three taps): a reduction, one thread per position.
//   disc_post_dgrad_kernel  its data gradient with the leaky ReLU of conv 4 folded in.
//   disc_wgrad_kernel       dW[co][ci][j] = sum_{b,n} dPre[co][n] * X[ci][in(n, j)] and db as a column of ones, for all six convs:
//                           the shape of voc_wgrad_kernel (vocoder_bwd.hip), 128 x 128 tiles, the reduction over (item, position)
//                           split into runs that depend on the shape alone; disc_wgrad_reduce_kernel adds the partial planes
//                           ascending in fp64.  Conv 0 reads the audio through the reflect index.
// The weight packs go through slab_pack.  The plan (mpd_plan) is pure: shapes, tiles, scratch and launches from (period, B, T).
#include <algorithm>

#include "slab_gemm.h"

namespace t2 {

constexpr int kDiscLayers = T2_HIFIGAN_MPD_LAYERS;             // five convs and conv_post
constexpr int kDiscK = 5, kDiscPostK = 3, kDiscStride3 = 3, kDiscMaxPeriod = 11;
constexpr int kDiscC[kDiscLayers + 1] = {1, 32, 128, 512, 1024, 1024, 1};
constexpr float kDiscSlope = 0.1f;
constexpr int kDiscFlush = 4;                      // chunks of 16 operand channels per MFMA chain before it joins the running sum
// slab row stride in floats: = 32 mod 64 banks, and the widest run a tile reads (stride 3, period 11, five taps)
constexpr int kDiscSlabStride = 480;
static_assert(kDiscSlabStride % 64 == 32 && kDiscSlabStride >= kDiscStride3 * (126 + kDiscMaxPeriod) + kDiscK * kDiscMaxPeriod + 1, "slab row stride");

static int disc_conv_stride(int i) { return i < 4 ? kDiscStride3 : 1; }
static int disc_conv_taps(int i) { return i < 5 ? kDiscK : kDiscPostK; }

// ------------------------------------------------------------------------------------------------------------------
// the GEMM-shaped convs and their data gradients
// ------------------------------------------------------------------------------------------------------------------
struct DiscGemm {
    const float* x; const float* wp; const float* bias; const float* g; const float* mask; float* y;
    int K, M, Nin;                                 // operand [B][K][Nin], output [B][M][Hout * p]
    int p, s, lo, halo;                            // column n = h*p + w reads operand (s*h + j - lo)*p + w at tap j
    int nphase, taps[3], Hq[3];                    // phase f owns output rows h = nphase*q + f, q < Hq[f]
    long phase_off[3];                             // its pack, in f32x4
    int Hout, mtiles, nchunks;
    float slope;
};

__device__ __forceinline__ void disc_mfma_step(const float* s0, const float* s1, const f32x4* wj, f32x16 (&acc)[1][2]) {
#pragma unroll
    for (int pg = 0; pg < 2; ++pg) {
        const f32x4 a = wj[pg * 64];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = (pg * 4 + i) * 2 * kDiscSlabStride;
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], s0[o], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], s1[o], acc[0][1], 0, 0, 0);
        }
    }
}

template <int WM>
__global__ void __launch_bounds__(WM * 128) disc_gemm_kernel(DiscGemm p) {
    __shared__ float slab[kSlabCK * kDiscSlabStride];
    const int wm = (threadIdx.x >> 6) % WM;
    const int mblocks = (p.mtiles + WM - 1) / WM;
    const int phase = blockIdx.y / mblocks, mt = (blockIdx.y % mblocks) * WM + wm;
    const bool active = mt < p.mtiles;             // uniform over the wave
    const int b = blockIdx.z;
    const int ntaps = p.taps[phase], Nq = p.Hq[phase] * p.p;
    const int n0 = blockIdx.x * kVocTT;
    if (n0 >= Nq) return;                          // this phase has fewer tiles: uniform over the workgroup, before any barrier
    const int lane = threadIdx.x & 63, wt = (threadIdx.x >> 6) / WM, tc = wt * 64 + (lane & 31), hk = lane >> 5;
    // n / p and n % p once per lane: the lane's two columns in the slab, whose column 0 holds operand index f0
    const int h0 = n0 / p.p;
    const long f0 = ((long)p.s * h0 - p.lo) * p.p;
    const int na = n0 + tc, nb = na + 32;
    const int off0 = p.s * (na / p.p - h0) * p.p + na % p.p, off1 = p.s * (nb / p.p - h0) * p.p + nb % p.p;
    const f32x4* wp = reinterpret_cast<const f32x4*>(p.wp) + p.phase_off[phase] + (size_t)(active ? mt : 0) * p.nchunks * ntaps * 128;
    const float* xb = p.x + (size_t)b * p.K * p.Nin;
    // two levels of summation: the MFMA chain runs over kDiscFlush chunks (at most 4 * 16 channels * 5 taps = 320 terms), then
    // joins `tot` by one fp32 add per element.  K reaches 5120 here; with one chain over all of it the tests' worst gradient err / bound was 1.43, with two levels 0.35.
    // The order stays fixed: chunks, taps, then pg and i of the step, ascending, and the groups of chunks ascending
    f32x16 acc[1][2] = {{f32x16{0}, f32x16{0}}}, tot[1][2] = {{f32x16{0}, f32x16{0}}};
    for (int c = 0; c < p.nchunks; ++c) {
        if (c) __syncthreads();                    // every wave is done reading the previous slab
        slab_stage<kDiscSlabStride, WM * 2>(slab, xb, p.K, c * kSlabCK, p.Nin, f0 + p.halo, p.halo, [](float v) { return v; });
        __syncthreads();
        if (active) {
            for (int j = 0; j < ntaps; ++j)
                disc_mfma_step(slab + hk * kDiscSlabStride + off0 + j * p.p, slab + hk * kDiscSlabStride + off1 + j * p.p,
                               wp + ((size_t)c * ntaps + j) * 128 + lane, acc);
            if (c % kDiscFlush == kDiscFlush - 1 || c == p.nchunks - 1) {
                tot[0][0] += acc[0][0]; tot[0][1] += acc[0][1];
                acc[0][0] = f32x16{0}; acc[0][1] = f32x16{0};
            }
        }
    }
    if (!active) return;
    const size_t lout = (size_t)p.Hout * p.p;
    slab_walk<WM, 1>(tot, mt, p.M, Nq, [=](int r, long q, const float (&a)[1]) {
        const int qi = (int)q;
        const size_t col = p.nphase == 1 ? (size_t)qi : (size_t)(qi / p.p * p.nphase + phase) * p.p + qi % p.p;
        const size_t o = ((size_t)b * p.M + r) * lout + col;
        float v = a[0];
        if (p.bias) {                              // forward: bias, then the leaky ReLU
            v += p.bias[r];
            v = v > 0.f ? v : v * p.slope;
        } else {                                   // data gradient: the upstream gradient on this feature map, then lrelu'
            if (p.g) v += p.g[o];
            v *= p.mask[o] > 0.f ? 1.f : p.slope;
        }
        p.y[o] = v;
    });
}

// conv 0: y[b][co][h'][w] = lrelu(bias[co] + sum_j w[co][j] * xpad[b][(3h' + j - 2) * p + w]), xpad the audio reflected on the right
__global__ void __launch_bounds__(256) disc_first_kernel(const float* __restrict__ audio, const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, int T, int p, int H0, int H1, float slope) {
    __shared__ float ws[kDiscC[1] * (kDiscK + 1)];
    for (int i = threadIdx.x; i < kDiscC[1] * kDiscK; i += 256) ws[i] = w[i];
    if (threadIdx.x < kDiscC[1]) ws[kDiscC[1] * kDiscK + threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.y, N1 = H1 * p;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N1) return;
    const int h = n / p, wc = n % p;
    float xv[kDiscK];
#pragma unroll
    for (int j = 0; j < kDiscK; ++j) {
        const int r = kDiscStride3 * h + j - 2;
        float v = 0.f;
        if (r >= 0 && r < H0) {
            long f = (long)r * p + wc;
            if (f >= T) f = 2L * T - 2 - f;        // F.pad(..., "reflect"): padded[T + i] = x[T - 2 - i]
            v = audio[(size_t)b * T + f];
        }
        xv[j] = v;
    }
    for (int co = 0; co < kDiscC[1]; ++co) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < kDiscK; ++j) acc = fmaf(ws[co * kDiscK + j], xv[j], acc);
        acc += ws[kDiscC[1] * kDiscK + co];
        y[((size_t)b * kDiscC[1] + co) * N1 + n] = acc > 0.f ? acc : acc * slope;
    }
}

// the gradient on padded position f of item b: sum over co, then over the taps j = r + 2 (mod 3) of row r = f / p, ascending
__device__ __forceinline__ float disc_first_dx(const float* __restrict__ dp, const float* ws, long f, int p, int H1) {
    const int r = (int)(f / p), wc = (int)(f % p), N1 = H1 * p;
    float acc = 0.f;
    for (int co = 0; co < kDiscC[1]; ++co)
        for (int j = (r + 2) % kDiscStride3; j < kDiscK; j += kDiscStride3) {
            const int h = (r + 2 - j) / kDiscStride3;     // r + 2 - j >= 0 wherever h < H1 can hold: j <= 4 and r + 2 - j = 3h
            if (r + 2 - j >= 0 && h < H1) acc = fmaf(ws[co * kDiscK + j], dp[(size_t)co * N1 + (size_t)h * p + wc], acc);
        }
    return acc;
}

__global__ void __launch_bounds__(256) disc_first_bwd_kernel(const float* __restrict__ dpre, const float* __restrict__ w, float* __restrict__ d_audio,
                                                            int T, int p, int H0, int H1) {
    __shared__ float ws[kDiscC[1] * kDiscK];
    for (int i = threadIdx.x; i < kDiscC[1] * kDiscK; i += 256) ws[i] = w[i];
    __syncthreads();
    const int b = blockIdx.y;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const float* dp = dpre + (size_t)b * kDiscC[1] * H1 * p;
    float v = disc_first_dx(dp, ws, t, p, H1);
    const long f = 2L * T - 2 - t;                 // the padded position that holds a copy of sample t, if the padding reaches it
    if (f >= T && f < (long)H0 * p) v += disc_first_dx(dp, ws, f, p, H1);
    d_audio[(size_t)b * T + t] = v;
}

// conv_post: y[b][h][w] = bias + sum_ci sum_j w[ci][j] * x[b][ci][h + j - 1][w], ci then j ascending, one fused multiply-add per term
__global__ void __launch_bounds__(256) disc_post_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ y, int C, int H, int p) {
    extern __shared__ float wl[];
    for (int i = threadIdx.x; i < C * kDiscPostK; i += 256) wl[i] = w[i];
    __syncthreads();
    const int b = blockIdx.y, N = H * p;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int h = n / p;
    const float* xb = x + (size_t)b * C * N;
    float acc = 0.f;
    for (int ci = 0; ci < C; ++ci) {
        const float* xr = xb + (size_t)ci * N + n;
#pragma unroll
        for (int j = 0; j < kDiscPostK; ++j) {
            const int r = h + j - 1;
            const float v = (r >= 0 && r < H) ? xr[(j - 1) * p] : 0.f;
            acc = fmaf(wl[ci * kDiscPostK + j], v, acc);
        }
    }
    y[(size_t)b * N + n] = acc + bias[0];
}

// dPre of conv 4 = lrelu'(fmap) * (g + sum_j w[ci][j] * d_post[h + 1 - j][w]), one thread per element
__global__ void __launch_bounds__(256) disc_post_dgrad_kernel(const float* __restrict__ dpost, const float* __restrict__ w, const float* __restrict__ g,
                                                             const float* __restrict__ fm, float* __restrict__ dpre, int C, int H, int p, float slope,
                                                             size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int N = H * p;
    const int n = (int)(idx % N), ci = (int)(idx / N % C);
    const size_t b = idx / N / C;
    const int h = n / p;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < kDiscPostK; ++j) {
        const int r = h + 1 - j;
        if (r >= 0 && r < H) acc = fmaf(w[ci * kDiscPostK + j], dpost[b * N + n + (1 - j) * p], acc);
    }
    if (g) acc += g[idx];
    dpre[idx] = acc * (fm[idx] > 0.f ? 1.f : slope);
}

// ------------------------------------------------------------------------------------------------------------------
// weight and bias gradient
// ------------------------------------------------------------------------------------------------------------------
constexpr int kDiscWgTile = 128, kDiscWgTL = 32, kDiscWgStride = 34, kDiscWgMaxSplit = 256;
static_assert(kDiscWgStride % 4 == 2 && kDiscWgStride >= kDiscWgTL, "rows 0..31 x 2 k-halves on 64 distinct banks");

// C[m][n] = sum_b sum_{l < La} A[b][m][l] * Bop[b][n][l].  A = dPre [B][M][La], La = H' * p.  Bop: column n = j*Cb + c (j < taps) is
// X[b][c] at flat index (s*h' + j - lo)*p + w for l = h'*p + w, zero where that row lies outside [0, H), mirrored at T (the reflect
// padding of the audio; elsewhere T = Lb = H*p and nothing mirrors); column taps*Cb is ones: the bias gradient.
struct DiscWgrad {
    const float* a; const float* bsrc; float* part; float* dw; float* db;
    int M, Cb, taps, Ntot, La, Lb;
    int p, s, lo, H, T;
    int B, nchunk, per, nsplit, mtiles, ntiles;
};

__global__ void __launch_bounds__(256) disc_wgrad_kernel(DiscWgrad p) {
    __shared__ float As[kDiscWgTile * kDiscWgStride], Bs[kDiscWgTile * kDiscWgStride];
    __shared__ int bch[kDiscWgTile], btap[kDiscWgTile];      // per column of the tile: its channel (-1: the ones, -2: none) and its tap
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hk = lane >> 5;
    const int mt = blockIdx.x % p.mtiles, nt = blockIdx.x / p.mtiles;
    const int m0 = mt * kDiscWgTile, n0 = nt * kDiscWgTile;
    const int total = p.B * p.nchunk, u0 = blockIdx.y * p.per, u1 = min(total, u0 + p.per);
    const int col = threadIdx.x & 31, row0 = threadIdx.x >> 5;
    // the waves' share of the tile follows the rows it holds (uniform over the workgroup), as in voc_wgrad_kernel: up to 32 rows
    // (conv 0, conv_post) every wave takes one 32 x 32 tile along the columns, up to 64 rows two, else 64 x 64 each
    const int rows_here = min(kDiscWgTile, p.M - m0);
    const int ni = rows_here <= 32 ? 1 : 2, nj = rows_here <= 64 ? 1 : 2;
    const int rbase = nj == 1 ? 0 : (wave & 1) * 64, cbase = nj == 1 ? wave * 32 : (wave >> 1) * 64;
    const int arows = nj == 1 ? ni * 32 : kDiscWgTile;
    if (threadIdx.x < kDiscWgTile) {
        const int n = n0 + threadIdx.x;
        int c = -2, j = 0;
        if (n < p.taps * p.Cb) { c = n % p.Cb; j = n / p.Cb; }
        else if (n < p.Ntot) c = -1;
        bch[threadIdx.x] = c; btap[threadIdx.x] = j;
    }
    __syncthreads();
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) { acc[i][0] = f32x16{0}; acc[i][1] = f32x16{0}; }
    for (int un = u0; un < u1; ++un) {
        const int b = un / p.nchunk;
        const int t = (un % p.nchunk) * kDiscWgTL + col;
        const int hq = t / p.p, wc = t - hq * p.p, r0 = p.s * hq - p.lo;
        if (un > u0) __syncthreads();              // every wave is done reading the previous slabs
        for (int row = row0; row < arows; row += 8) {
            const int m = m0 + row;
            As[row * kDiscWgStride + col] = (t < p.La && m < p.M) ? p.a[((size_t)b * p.M + m) * p.La + t] : 0.f;
        }
        for (int row = row0; row < kDiscWgTile; row += 8) {
            const int c = bch[row];
            float v = 0.f;
            if (t < p.La) {
                if (c >= 0) {
                    const int r = r0 + btap[row];
                    if (r >= 0 && r < p.H) {
                        long f = (long)r * p.p + wc;
                        if (f >= p.T) f = 2L * p.T - 2 - f;
                        v = p.bsrc[((size_t)b * p.Cb + c) * p.Lb + f];
                    }
                } else if (c == -1) {
                    v = 1.f;
                }
            }
            Bs[row * kDiscWgStride + col] = v;
        }
        __syncthreads();
        const float* ap = As + (rbase + (lane & 31)) * kDiscWgStride + hk;
        const float* bp = Bs + (cbase + (lane & 31)) * kDiscWgStride + hk;
#pragma unroll
        for (int kk = 0; kk < kDiscWgTL / 2; ++kk) {
            const float a0 = ap[2 * kk], b0 = bp[2 * kk];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            if (ni > 1) {                          // uniform over the workgroup
                const float a1 = ap[32 * kDiscWgStride + 2 * kk];
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                if (nj > 1) {
                    const float b1 = bp[32 * kDiscWgStride + 2 * kk];
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

// dw[m][c][j] (torch's [Cout][Cin][k][1]) = the planes' sum at (m, j*Cb + c); db[m] the column of ones
__global__ void __launch_bounds__(256) disc_wgrad_reduce_kernel(DiscWgrad p) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, row = (size_t)p.taps * p.Cb, nw = (size_t)p.M * row, plane = (size_t)p.M * p.Ntot;
    if (idx >= nw + p.M) return;
    const int m = idx < nw ? (int)(idx / row) : (int)(idx - nw), n = idx < nw ? (int)(idx % row) : (int)row;
    double acc = 0.0;
    for (int y = 0; y < p.nsplit; ++y) acc += (double)p.part[(size_t)y * plane + (size_t)m * p.Ntot + n];
    if (idx < nw) p.dw[((size_t)m * p.Cb + n % p.Cb) * p.taps + n / p.Cb] = (float)acc;
    else p.db[m] = (float)acc;
}

// the shape of one launch from the sizes alone
static DiscWgrad disc_wgrad_shape(int B, int Cin, int Cout, int taps, int s, int p, int Hin, int Hout, int T) {
    DiscWgrad q{};
    q.B = B; q.M = Cout; q.Cb = Cin; q.taps = taps; q.Ntot = taps * Cin + 1; q.La = Hout * p;
    q.p = p; q.s = s; q.lo = (taps - 1) / 2; q.H = Hin; q.Lb = T ? T : Hin * p; q.T = q.Lb;
    q.mtiles = (q.M + kDiscWgTile - 1) / kDiscWgTile; q.ntiles = (q.Ntot + kDiscWgTile - 1) / kDiscWgTile;
    q.nchunk = (q.La + kDiscWgTL - 1) / kDiscWgTL;
    const long total = (long)B * q.nchunk;
    // at most 1024 workgroups, what 256 CUs hold at once at 4 per CU (35 840 bytes of LDS): one more would wait a whole round
    const long nsplit = std::min<long>(std::min<long>(kDiscWgMaxSplit, total), std::max<long>(1, 1024 / (q.mtiles * q.ntiles)));
    q.per = (int)((total + nsplit - 1) / nsplit);
    q.nsplit = (int)((total + q.per - 1) / q.per);
    return q;
}

static int disc_wgrad(DiscWgrad q, const float* a, const float* bsrc, float* dw, float* db, float* part, hipStream_t s) {
    q.a = a; q.bsrc = bsrc; q.dw = dw; q.db = db; q.part = part;
    hipLaunchKernelGGL(disc_wgrad_kernel, dim3((unsigned)(q.mtiles * q.ntiles), (unsigned)q.nsplit), dim3(256), 0, s, q);
    T2_LAUNCH_CHECK();
    const size_t n = (size_t)q.M * q.taps * q.Cb + q.M;
    hipLaunchKernelGGL(disc_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q);
    T2_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// the plan: pure, no device
// ------------------------------------------------------------------------------------------------------------------
struct MpdPlan {
    int period, B, T, pad;
    int H[kDiscLayers + 1];                        // H[0]: rows of the padded audio; H[i + 1]: rows of feature map i
    size_t fmap_floats[kDiscLayers], max_fmap;
    size_t w_off[kDiscLayers], b_off[kDiscLayers], packed_floats;      // forward pack: conv 0 and conv_post as torch has them, the rest slab packs
    size_t bwd_off[kDiscLayers][3], packed_bwd_floats;                  // data-gradient packs of convs 1..4, per phase
    size_t gw_off[kDiscLayers], gb_off[kDiscLayers], grad_floats;      // the gradient arena, torch layouts
    DiscWgrad wg[kDiscLayers];
    size_t part_floats, ws_floats;
    int tiles[kDiscLayers];
};
// polyphase taps of a stride-3 data gradient: phase f takes forward taps kPhaseTap0[f] and (two-tap phases) kPhaseTap0[f] - 3
constexpr int kPhaseTaps[3] = {1, 2, 2}, kPhaseTap0[3] = {2, 3, 4};

static int mpd_plan(int period, int B, int T, MpdPlan* out) {
    const char* who = "hifigan multi-period discriminator";
    T2_REQUIRE(out, "%s: null plan", who);
    T2_REQUIRE(period >= 2 && period <= kDiscMaxPeriod, "%s: period %d outside 2..%d", who, period, kDiscMaxPeriod);
    T2_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d outside 1..65535 (real and generated items together)", who, B);
    T2_REQUIRE(T >= 1 && T <= (1 << 28), "%s: T=%d outside 1..%d samples", who, T, 1 << 28);
    MpdPlan& P = *out;
    P = MpdPlan{};
    P.period = period; P.B = B; P.T = T;
    P.pad = (period - T % period) % period;
    T2_REQUIRE(P.pad <= T - 1, "%s: T=%d is too short for period %d: the reflect padding of %d needs at least %d samples", who, T, period, P.pad, P.pad + 1);
    P.H[0] = (T + P.pad) / period;
    for (int i = 0; i < kDiscLayers; ++i) P.H[i + 1] = disc_conv_stride(i) == 1 ? P.H[i] : (P.H[i] - 1) / kDiscStride3 + 1;
    size_t off = 0, boff = 0, goff = 0;
    P.part_floats = 0; P.max_fmap = 0;
    for (int i = 0; i < kDiscLayers; ++i) {
        const int cin = kDiscC[i], cout = kDiscC[i + 1], k = disc_conv_taps(i), s = disc_conv_stride(i);
        const bool gemm = i >= 1 && i <= 4;
        P.fmap_floats[i] = (size_t)B * cout * P.H[i + 1] * period;
        P.max_fmap = std::max(P.max_fmap, round4(P.fmap_floats[i]));
        P.tiles[i] = gemm ? (P.H[i + 1] * period + kVocTT - 1) / kVocTT : 0;
        P.w_off[i] = off; off += gemm ? slab_packed_floats(1, cout, cin, k, 0) : round4((size_t)cout * cin * k);
        P.b_off[i] = off; off += round4(cout);
        for (int f = 0; f < 3; ++f) {
            P.bwd_off[i][f] = boff;
            if (gemm && s == 1 && f == 0) boff += slab_packed_floats(1, cin, cout, k, 0);
            if (gemm && s != 1) boff += slab_packed_floats(1, cin, cout, kPhaseTaps[f], 0);
        }
        P.gw_off[i] = goff; goff += round4((size_t)cout * cin * k);
        P.gb_off[i] = goff; goff += round4(cout);
        P.wg[i] = disc_wgrad_shape(B, cin, cout, k, s, period, P.H[i], P.H[i + 1], i == 0 ? T : 0);
        P.part_floats = std::max(P.part_floats, round4((size_t)P.wg[i].nsplit * P.wg[i].M * P.wg[i].Ntot));
    }
    P.packed_floats = off; P.packed_bwd_floats = boff; P.grad_floats = goff;
    P.ws_floats = 2 * P.max_fmap + P.part_floats;  // two buffers for the chain of dPre, the weight gradients' partial planes
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// packs and executors
// ------------------------------------------------------------------------------------------------------------------
static int mpd_pack(const float* const* weights, const float* const* biases, float* packed, hipStream_t s) {
    MpdPlan P;
    T2_TRY_RC(mpd_plan(2, 1, 2, &P));
    T2_REQUIRE(weights && biases && packed, "hifigan_mpd_pack: null pointer");
    for (int i = 0; i < kDiscLayers; ++i) {
        const int cin = kDiscC[i], cout = kDiscC[i + 1], k = disc_conv_taps(i);
        T2_REQUIRE(weights[i] && biases[i], "hifigan_mpd_pack: conv %d has a null weight or bias", i);
        if (i >= 1 && i <= 4) {
            SlabPack q{};
            q.gates = 1; q.rows = cout; q.split = 1; q.out = packed + P.w_off[i];
            q.s0.w = weights[i]; q.s0.K = cin; q.s0.taps = k; q.s0.rhi = (long)cin * k; q.s0.ks = k; q.s0.ts = 1;
            T2_TRY_RC(slab_pack(q, s));
        } else {
            T2_CHECK_HIP(hipMemcpyAsync(packed + P.w_off[i], weights[i], sizeof(float) * cout * cin * k, hipMemcpyDeviceToDevice, s));
        }
        T2_CHECK_HIP(hipMemcpyAsync(packed + P.b_off[i], biases[i], sizeof(float) * cout, hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

// rows = Cin, K = Cout: element (ci, co, tap t) = w[co][ci][tap0 + t * tstep]
static int mpd_pack_backward(const float* const* weights, float* packed_bwd, hipStream_t s) {
    MpdPlan P;
    T2_TRY_RC(mpd_plan(2, 1, 2, &P));
    T2_REQUIRE(weights && packed_bwd, "hifigan_mpd_pack_backward: null pointer");
    for (int i = 1; i <= 4; ++i) {
        const int cin = kDiscC[i], cout = kDiscC[i + 1];
        T2_REQUIRE(weights[i], "hifigan_mpd_pack_backward: conv %d has a null weight", i);
        SlabPack q{};
        q.gates = 1; q.rows = cin; q.split = 1;
        q.s0.w = weights[i]; q.s0.K = cout; q.s0.rhi = kDiscK; q.s0.ks = (long)cin * kDiscK;
        if (disc_conv_stride(i) == 1) {            // the taps flipped: the padding is symmetric
            q.out = packed_bwd + P.bwd_off[i][0]; q.s0.taps = kDiscK; q.s0.base = kDiscK - 1; q.s0.ts = -1;
            T2_TRY_RC(slab_pack(q, s));
            continue;
        }
        for (int f = 0; f < 3; ++f) {
            q.out = packed_bwd + P.bwd_off[i][f]; q.s0.taps = kPhaseTaps[f]; q.s0.base = kPhaseTap0[f]; q.s0.ts = -kDiscStride3;
            T2_TRY_RC(slab_pack(q, s));
        }
    }
    return 0;
}

static int disc_gemm_launch(DiscGemm q, int B, hipStream_t s) {
    int tmax = 0, ncols = 0;
    for (int f = 0; f < q.nphase; ++f) { tmax = std::max(tmax, q.taps[f]); ncols = std::max(ncols, q.Hq[f] * q.p); }
    const int W = q.s * (126 + q.p) + tmax * q.p;  // the run of the operand one tile reads, all taps
    q.halo = (W - kVocTT + 1) / 2;
    T2_REQUIRE(q.halo >= 0 && kVocTT + 2 * q.halo <= kDiscSlabStride, "hifigan discriminator conv: a run of %d columns does not fit the slab", W);
    q.mtiles = (q.M + 31) / 32; q.nchunks = slab_chunks(q.K);
    q.slope = kDiscSlope;
    if (ncols == 0) return 0;
    return slab_launch(disc_gemm_kernel<4>, disc_gemm_kernel<2>, disc_gemm_kernel<1>, q, q.mtiles, (long)ncols, q.nphase, B, s);
}

static int mpd_forward(const t2_hifigan_mpd_fwd_args& a, hipStream_t s) {
    MpdPlan P;
    T2_TRY_RC(mpd_plan(a.period, a.B, a.T, &P));
    T2_REQUIRE(a.packed && a.audio, "hifigan_mpd_forward: null pointer");
    for (int i = 0; i < kDiscLayers; ++i) T2_REQUIRE(a.fmap[i], "hifigan_mpd_forward: feature map %d is null", i);
    const int p = P.period;
    hipLaunchKernelGGL(disc_first_kernel, dim3((unsigned)((P.H[1] * p + 255) / 256), (unsigned)a.B), dim3(256), 0, s, a.audio, a.packed + P.w_off[0],
                       a.packed + P.b_off[0], a.fmap[0], a.T, p, P.H[0], P.H[1], kDiscSlope);
    T2_LAUNCH_CHECK();
    for (int i = 1; i <= 4; ++i) {
        DiscGemm q{};
        q.x = a.fmap[i - 1]; q.wp = a.packed + P.w_off[i]; q.bias = a.packed + P.b_off[i]; q.y = a.fmap[i];
        q.K = kDiscC[i]; q.M = kDiscC[i + 1]; q.Nin = P.H[i] * p;
        q.p = p; q.s = disc_conv_stride(i); q.lo = 2;
        q.nphase = 1; q.taps[0] = kDiscK; q.Hq[0] = P.H[i + 1]; q.Hout = P.H[i + 1];
        T2_TRY_RC(disc_gemm_launch(q, a.B, s));
    }
    hipLaunchKernelGGL(disc_post_kernel, dim3((unsigned)((P.H[6] * p + 255) / 256), (unsigned)a.B), dim3(256), sizeof(float) * kDiscC[5] * kDiscPostK, s,
                       a.fmap[4], a.packed + P.w_off[5], a.packed + P.b_off[5], a.fmap[5], kDiscC[5], P.H[5], p);
    T2_LAUNCH_CHECK();
    return 0;
}

static int mpd_backward(const t2_hifigan_mpd_bwd_args& a, hipStream_t s) {
    MpdPlan P;
    T2_TRY_RC(mpd_plan(a.period, a.B, a.T, &P));
    T2_REQUIRE(a.packed && a.packed_bwd && a.audio && a.workspace, "hifigan_mpd_backward: null pointer");
    for (int i = 0; i < kDiscLayers; ++i) T2_REQUIRE(a.fmap[i], "hifigan_mpd_backward: feature map %d is null", i);
    T2_REQUIRE(a.g_fmap[5], "hifigan_mpd_backward: the gradient on conv_post's output (the score) must be given");
    T2_REQUIRE(a.grads || a.d_audio, "hifigan_mpd_backward: neither the weights' nor the audio's gradient is asked for");
    const int p = P.period;
    float* buf[2] = {a.workspace, a.workspace + P.max_fmap};
    float* part = a.workspace + 2 * P.max_fmap;
    auto wgrad = [&](int i, const float* dpre, const float* x) -> int {
        if (!a.grads) return 0;                    // without an arena no weight gradient is launched
        return disc_wgrad(P.wg[i], dpre, x, a.grads + P.gw_off[i], a.grads + P.gb_off[i], part, s);
    };
    T2_TRY_RC(wgrad(5, a.g_fmap[5], a.fmap[4]));
    int cur = 0;
    hipLaunchKernelGGL(disc_post_dgrad_kernel, dim3((unsigned)((P.fmap_floats[4] + 255) / 256)), dim3(256), 0, s, a.g_fmap[5], a.packed + P.w_off[5], a.g_fmap[4],
                       a.fmap[4], buf[cur], kDiscC[5], P.H[5], p, kDiscSlope, P.fmap_floats[4]);
    T2_LAUNCH_CHECK();
    for (int i = 4; i >= 1; --i) {                 // buf[cur] holds dPre of conv i
        T2_TRY_RC(wgrad(i, buf[cur], a.fmap[i - 1]));
        DiscGemm q{};
        q.x = buf[cur]; q.g = a.g_fmap[i - 1]; q.mask = a.fmap[i - 1]; q.y = buf[cur ^ 1];
        q.K = kDiscC[i + 1]; q.M = kDiscC[i]; q.Nin = P.H[i + 1] * p;
        q.p = p; q.s = 1; q.Hout = P.H[i];
        if (disc_conv_stride(i) == 1) {
            q.wp = a.packed_bwd + P.bwd_off[i][0]; q.lo = 2; q.nphase = 1; q.taps[0] = kDiscK; q.Hq[0] = P.H[i];
        } else {
            q.wp = a.packed_bwd + P.bwd_off[i][0]; q.lo = 0; q.nphase = 3;
            for (int f = 0; f < 3; ++f) {
                q.taps[f] = kPhaseTaps[f]; q.Hq[f] = (P.H[i] - f + 2) / 3;
                q.phase_off[f] = (long)((P.bwd_off[i][f] - P.bwd_off[i][0]) / 4);
            }
        }
        T2_TRY_RC(disc_gemm_launch(q, a.B, s));
        cur ^= 1;
    }
    T2_TRY_RC(wgrad(0, buf[cur], a.audio));
    if (a.d_audio) {
        hipLaunchKernelGGL(disc_first_bwd_kernel, dim3((unsigned)((a.T + 255) / 256), (unsigned)a.B), dim3(256), 0, s, buf[cur], a.packed + P.w_off[0], a.d_audio,
                           a.T, p, P.H[0], P.H[1]);
        T2_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace t2

// ---- C ABI (include/t2amd.h)
using namespace t2;

extern "C" {

int t2_hifigan_mpd_plan(int period, int B, int T, t2_hifigan_mpd_plan_info* out) {
    T2_REQUIRE(out, "t2_hifigan_mpd_plan: null pointer");
    MpdPlan P;
    T2_TRY_RC(mpd_plan(period, B, T, &P));
    out->period = P.period; out->B = P.B; out->T = P.T; out->pad = P.pad;
    for (int i = 0; i <= kDiscLayers; ++i) { out->H[i] = P.H[i]; out->C[i] = kDiscC[i]; }
    for (int i = 0; i < kDiscLayers; ++i) {
        out->tiles[i] = P.tiles[i]; out->splits[i] = P.wg[i].nsplit;
        out->fmap_floats[i] = P.fmap_floats[i]; out->w_offsets[i] = P.gw_off[i]; out->b_offsets[i] = P.gb_off[i];
    }
    out->packed_bytes = P.packed_floats * sizeof(float); out->packed_bwd_bytes = P.packed_bwd_floats * sizeof(float);
    out->workspace_bytes = P.ws_floats * sizeof(float); out->part_bytes = P.part_floats * sizeof(float);
    out->grad_floats = P.grad_floats;
    out->n_forward_launches = kDiscLayers;
    out->n_backward_launches = 2 * kDiscLayers + 1 + 4 + 1;   // weight gradients with their reduces, conv_post's and the four GEMM data gradients, the audio's
    return 0;
}
int t2_hifigan_mpd_pack(const float* const* weights_host, const float* const* biases_host, float* packed, void* stream) {
    return mpd_pack(weights_host, biases_host, packed, (hipStream_t)stream);
}
int t2_hifigan_mpd_pack_backward(const float* const* weights_host, float* packed_bwd, void* stream) {
    return mpd_pack_backward(weights_host, packed_bwd, (hipStream_t)stream);
}
int t2_hifigan_mpd_forward(const t2_hifigan_mpd_fwd_args* a, void* stream) {
    T2_REQUIRE(a, "t2_hifigan_mpd_forward: null arguments");
    return mpd_forward(*a, (hipStream_t)stream);
}
int t2_hifigan_mpd_backward(const t2_hifigan_mpd_bwd_args* a, void* stream) {
    T2_REQUIRE(a, "t2_hifigan_mpd_backward: null arguments");
    return mpd_backward(*a, (hipStream_t)stream);
}

}  // extern "C"
