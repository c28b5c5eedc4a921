// WaveGlow's kernels and, for each, the host function that launches it once: no driver, no plan, no timer (waveglow.hip drives
// them, waveglow_plan.hip says where their operands lie).
//
// Activations are [B][C][L] with time contiguous, L = T*256/n_group; arithmetic is exact fp32 on the matrix cores
// (v_mfma_f32_32x32x2_f32), whatever t2_set_precision says.  Three of the five kernels of the WN are one GEMM kernel on the pieces
// that slab_gemm.h holds for this file and vocoder.hip (staging, MFMA step, epilogue walk, launcher, pack): here no transform while
// staging, two operand segments, two accumulator pairs for the gate, and three epilogues:
//   gated conv   Y = tanh(U[:nc]) * sigmoid(U[nc:]),  U = in_layers[i](x) + cond_layer(spect)[2nc*i : 2nc*(i+1)] as ONE GEMM with
//                K = 3*nc (the taps read x at -d, 0, +d from the slab) + n_mel*G (spect at the same column).  Tanh row c and
//                sigmoid row c + nc are two accumulators of the same wave: same lane, same element, same column, so the gate is
//                applied in registers and only [B, nc, L] is written.  The conditioning tensor [B, 2*nc*n_layers, L] never exists.
//   res_skip     the 1x1 conv; its epilogue does x += rs[:nc] and out += rs[nc:] in place (acts is a buffer of its own).
//   upsample     ConvTranspose1d(n_mel, n_mel, 1024, stride 256) as a polyphase GEMM: output sample 256q + r reads taps r + 256m
//                (m = 0..3) of frames q - m, so rows = (channel, phase r), columns = frames q, K = n_mel * 4; the epilogue writes
//                spect[b, ch*G + g, l] at 256q + r = l*G + g.  Each element once.  Inference never computes the 768 trailing
//                samples; the forward direction, whose audio may reach into them, asks for up to three more columns q.
// `start` (K <= 4) and the coupling (end: <= 8 rows reduced over nc with lanes along time, then (a1 - b)/exp(s), the c x c inverse
// mix and the early-noise prepend in one pass) are plain VALU.  The forward direction adds a head kernel (regroup + W_0), one tail
// kernel per flow and two small kernels that finish the sums in a fixed order; log |det W_k| comes from an fp64 LU.  The backward's
// data gradients are the same GEMM kernel on transposed packs with two more epilogues (gate backward: W_rs^T [dx; d_out] times the
// gate's derivative from the kept halves; accumulate: dx += conv^T(du), d_spect += W_cond^T du); its weight gradients are a second
// GEMM, wg_wgrad_kernel, whose reduction runs along time and is split over (item, time chunk) into partial planes added in a fixed
// order; the tail, start, head and upsample backward are VALU.  No atomics, every sum in a fixed order, 64-bit element offsets.
#include <algorithm>

#include "slab_gemm.h"
#include "waveglow.h"

namespace t2 {

constexpr int kWgStride = 416;                    // slab row stride in floats: = 32 mod 64 banks, >= kVocTT + 2*kWgMaxD
static_assert(kWgStride % 64 == 32 && kWgStride >= kVocTT + 2 * kWgMaxD, "slab row stride");
constexpr int kWgGradStride = 34;                 // row stride of the weight gradient's slabs
// Y[row][q] = sum over segment 0 (C0 channels x taps, tap j at slab column q + coff0 + j*cstep) and segment 1 (C1 channels, one
// tap at q) of packed weight x operand.  N = columns (row length of both operands and, but for the upsample, of the output).
struct WgGemm {
    const float* x0; const float* x1; const float* wp; const float* bias0; const float* bias1;
    float* y0; float* y1;
    int C0, C1, N;
    int taps, coff0, cstep, halo;
    int rows, mtiles, nch0, nch1;
    int first, last, raw, G; long Lg;             // res_skip: first, last; gated: raw; upsample: G, Lg = columns of spect
    int Nq;                                       // output columns: N, but for an upsample that keeps trailing samples (up to N + 3)
    const float* res;                             // res_skip: the x that rs[:nc] is added to (y0 receives the sum; the same buffer unless x_i is kept)
    float* s0; float* s1;                         // gated: nullable, receive tanh(u_a) and sigmoid(u_b) [B, nc, L]; gate backward: read as such
};

template <int WM, int MODE>
__global__ void __launch_bounds__(WM * 128) wg_gemm_kernel(WgGemm p) {
    constexpr int GATES = MODE == kWgGated ? 2 : 1;
    __shared__ float slab[kSlabCK * kWgStride];
    const int mt = blockIdx.y * WM + (threadIdx.x >> 6) % WM;
    const bool active = mt < p.mtiles;            // uniform over the wave
    const int b = blockIdx.z;
    const f32x4* wp = reinterpret_cast<const f32x4*>(p.wp) + (size_t)(active ? mt : 0) * (p.nch0 * p.taps + p.nch1) * GATES * 128;
    const int lane = threadIdx.x & 63, wt = (threadIdx.x >> 6) / WM, tc = wt * 64 + (lane & 31), hk = lane >> 5;
    const long t0 = (long)blockIdx.x * kVocTT;
    f32x16 acc[GATES][2];
#pragma unroll
    for (int g = 0; g < GATES; ++g) { acc[g][0] = f32x16{0}; acc[g][1] = f32x16{0}; }
    for (int c = 0; c < p.nch0 + p.nch1; ++c) {
        const bool seg0 = c < p.nch0;
        const int C = seg0 ? p.C0 : p.C1, ci0 = (seg0 ? c : c - p.nch0) * kSlabCK;
        const int halo = seg0 ? p.halo : 0;
        const float* xb = (seg0 ? p.x0 : p.x1) + (size_t)b * C * p.N;
        if (c) __syncthreads();                    // every wave is done reading the previous slab
        slab_stage<kWgStride, WM * 2>(slab, xb, C, ci0, p.N, t0, halo, [](float v) { return v; });
        __syncthreads();
        if (active) {
            const int taps = seg0 ? p.taps : 1;
            const size_t step0 = seg0 ? (size_t)c * p.taps : (size_t)p.nch0 * p.taps + (c - p.nch0);
            for (int j = 0; j < taps; ++j)
                slab_mfma_step<kWgStride, GATES>(slab + hk * kWgStride + tc + (seg0 ? p.coff0 + j * p.cstep : 0), wp + (step0 + j) * GATES * 128 + lane, acc);
        }
    }
    if (!active) return;
    slab_walk<WM, GATES>(acc, mt, p.rows, p.Nq, [=](int r, long q, const float (&a)[GATES]) {
        if constexpr (MODE == kWgGated) {
            const float ua = (a[0] + p.bias0[r]) + p.bias1[r];
            const float ub = (a[1] + p.bias0[r + p.rows]) + p.bias1[r + p.rows];
            if (p.raw) {
                p.y0[((size_t)b * 2 * p.rows + r) * p.N + q] = ua;
                p.y0[((size_t)b * 2 * p.rows + p.rows + r) * p.N + q] = ub;
            } else {
                const float tv = tanhf(ua), gv = 1.f / (1.f + expf(-ub));
                const size_t o = ((size_t)b * p.rows + r) * p.N + q;
                if (p.s0) { p.s0[o] = tv; p.s1[o] = gv; }
                p.y0[o] = tv * gv;
            }
        } else if constexpr (MODE == kWgResSkip) {
            const float v = a[0] + p.bias0[r];
            const int nc = p.C0;
            if (!p.last && r < nc) {
                const size_t o = ((size_t)b * nc + r) * p.N + q;
                p.y0[o] = p.res[o] + v;
            } else {
                const size_t o = ((size_t)b * nc + (p.last ? r : r - nc)) * p.N + q;
                p.y1[o] = p.first ? v : p.y1[o] + v;
            }
        } else if constexpr (MODE == kWgGateBwd) {
            // d_acts = a[0]; du = [d_acts * g * (1 - t^2); d_acts * t * g * (1 - g)] [B, 2*rows, L], acts = t * g recomputed
            const size_t o = ((size_t)b * p.rows + r) * p.N + q, o2 = ((size_t)b * 2 * p.rows + r) * p.N + q;
            const float tv = p.s0[o], gv = p.s1[o], da = a[0];
            p.y0[o2] = da * gv * (1.f - tv * tv);
            p.y0[o2 + (size_t)p.rows * p.N] = da * tv * gv * (1.f - gv);
            p.y1[o] = tv * gv;
        } else if constexpr (MODE == kWgAccum) {
            const size_t o = ((size_t)b * p.rows + r) * p.N + q;
            p.y0[o] = p.first ? a[0] : p.y0[o] + a[0];
        } else {
            const int ch = r / kWgUpStride;
            const long t = q * kWgUpStride + (r % kWgUpStride), l = t / p.G;
            if (l < p.Lg) p.y0[(((size_t)b * p.C0 + ch) * p.G + (int)(t % p.G)) * p.Lg + l] = a[0] + p.bias0[ch];
        }
    });
}

// x[b, c, t] = bias[c] + sum_h w[c][h] * (scale * audio[b, h, t]), h ascending; 32 channels per workgroup row
__global__ void __launch_bounds__(256) wg_start_kernel(const float* __restrict__ audio, int ctot, int n_half, float scale, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ x, int nc, long L) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= L) return;
    const int b = blockIdx.z;
    float a[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) a[h] = h < n_half ? audio[((size_t)b * ctot + h) * L + t] * scale : 0.f;
    const int c1 = min(nc, (int)(blockIdx.y + 1) * 32);
    for (int c = blockIdx.y * 32; c < c1; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int h = 0; h < 4; ++h)
            if (h < n_half) acc = fmaf(w[c * n_half + h], a[h], acc);
        x[((size_t)b * nc + c) * L + t] = acc + bias[c];
    }
}

// ---- what the coupling and the tail backward open with (the forward tail measured 1 % slower on them and keeps its own text; the
// `end` reduction stays a loop in each kernel, a shared one cost 3 %): w_end [C][nc], b_end [C], a mix [Cm][Cm] to LDS (256 threads)
__device__ __forceinline__ void wg_load_end(float* we, float* be, float* wi, const float* w_end, const float* b_end, const float* mix, int C, int nc,
                                            int Cm) {
    for (int i = threadIdx.x; i < C * nc; i += 256) we[i] = w_end[i];
    if (threadIdx.x < C) be[threadIdx.x] = b_end[threadIdx.x];
    if (threadIdx.x < Cm * Cm) wi[threadIdx.x] = mix[threadIdx.x];
    __syncthreads();
}
// a[h] and a[nh + h] without a dynamic register index: read, read with be[.] added (be: 8 floats), write
__device__ __forceinline__ void wg_get_pair(const float (&a)[8], int h, int nh, float& lo, float& hi) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        lo = r == h ? a[r] : lo;
        hi = r == nh + h ? a[r] : hi;
    }
}
__device__ __forceinline__ void wg_get_pair_plus(const float (&a)[8], const float* be, int h, int nh, float& lo, float& hi) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float t = a[r] + be[r];
        lo = r == h ? t : lo;
        hi = r == nh + h ? t : hi;
    }
}
__device__ __forceinline__ void wg_put_pair(float (&a)[8], int h, int nh, float lo, float hi) {
#pragma unroll
    for (int r = 0; r < 8; ++r) a[r] = r == h ? lo : (r == nh + h ? hi : a[r]);
}
// sum over the 256 threads, thread j's term at red[j]: a tree in LDS, in every run the same order
__device__ __forceinline__ double wg_tree_sum(double* red, double v) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// one thread per (item, column): end as <= 8 fmaf chains over nc (ascending), the affine inverse, the c x c mix (ascending)
__global__ void __launch_bounds__(256) wg_couple_kernel(WgCouple p) {
    __shared__ float we[8 * 512], be[8], wi[64];
    const int nh = p.n_half, C = 2 * nh;
    wg_load_end(we, be, wi, p.w_end, p.b_end, p.winv, C, p.nc, C);
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.L) return;
    const int b = blockIdx.y;
    float o[8], v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { o[r] = 0.f; v[r] = 0.f; }
    const float* ob = p.out + (size_t)b * p.nc * p.L + t;
    for (int c = 0; c < p.nc; ++c) {
        const float x = ob[(size_t)c * p.L];
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (r < C) o[r] = fmaf(we[r * p.nc + c], x, o[r]);
    }
    const float* ib = p.in + (size_t)b * C * p.L + t;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        if (h < nh) {
            const float a0 = ib[(size_t)h * p.L] * p.in_scale, a1 = ib[(size_t)(nh + h) * p.L] * p.in_scale;
            float bb = 0.f, s = 0.f;
            wg_get_pair_plus(o, be, h, nh, bb, s);
            wg_put_pair(v, h, nh, a0, (a1 - bb) / expf(s));
        }
    }
    const int Cn = C + p.n_early;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if (r < C) {
            float y = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c < C) y = fmaf(wi[r * C + c], v[c], y);
            if (p.dst) p.dst[((size_t)b * Cn + p.n_early + r) * p.L + t] = y;
            if (p.inter) p.inter[((size_t)b * p.L + t) * C + r] = y;
        }
    }
    if (p.dst)
        for (int j = 0; j < p.n_early; ++j) p.dst[((size_t)b * Cn + j) * p.L + t] = p.sigma * p.z[((size_t)b * p.n_early + j) * p.L + t];
}

// ---- the forward direction (audio -> z, glow.py:207-249): the kernels around the WN, which is the one above
// fixed-order sum of one double per lane over the wave, in every lane
__device__ __forceinline__ double wg_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// dst[b, r, l] = sum_g w[r][g] * audio[b, l*G + g] (g ascending): the regroup of glow.py:223 and flow 0's mix; one thread per (b, l)
__global__ void __launch_bounds__(256) wg_head_kernel(const float* __restrict__ audio, const float* __restrict__ w, float* __restrict__ dst, int G, long N,
                                                     long L) {
    __shared__ float wi[64];
    if (threadIdx.x < G * G) wi[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    const long l = (long)blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    const int b = blockIdx.y;
    const float* ab = audio + (size_t)b * N + (size_t)l * G;
    float v[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) v[g] = g < G ? ab[g] : 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if (r < G) {
            float y = 0.f;
#pragma unroll
            for (int g = 0; g < 8; ++g)
                if (g < G) y = fmaf(wi[r * G + g], v[g], y);
            dst[((size_t)b * G + r) * L + l] = y;
        }
    }
}

// One flow's tail, one thread per (item, column): (b, s) = end(out) as <= 8 fmaf chains over nc (ascending), a1' = exp(s) * a1 + b,
// v = cat(a0, a1').  v[:n_peel] goes to z[:, zoff:] (the next flow's early output; on the last flow all of v), the rest is mixed by
// the next flow's W (ascending) into dst.  part_s / part_z [item][column block] receive the workgroup's sums of s and of the z^2 it
// wrote, added in fp64 from the first term: per thread in channel order, then a xor tree over the wave, then the waves in order.
__global__ void __launch_bounds__(256) wg_tail_kernel(WgTail p) {
    __shared__ __align__(8) float we[8 * 512];
    __shared__ float be[8], wi[64];
    const int nh = p.n_half, C = 2 * nh, Cn = C - p.n_peel;
    for (int i = threadIdx.x; i < C * p.nc; i += 256) we[i] = p.w_end[i];
    if (threadIdx.x < C) be[threadIdx.x] = p.b_end[threadIdx.x];
    if (threadIdx.x < Cn * Cn) wi[threadIdx.x] = p.wnext[threadIdx.x];
    __syncthreads();
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = t < p.L;
    const int b = blockIdx.y;
    double sum_s = 0.0, sum_z = 0.0;
    if (valid) {
        float o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) o[r] = 0.f;
        const float* ob = p.out + (size_t)b * p.nc * p.L + t;
        for (int c = 0; c < p.nc; ++c) {
            const float x = ob[(size_t)c * p.L];
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (r < C) o[r] = fmaf(we[r * p.nc + c], x, o[r]);
        }
        float v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = 0.f;
        const float* ib = p.in + (size_t)b * C * p.L + t;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            if (h < nh) {
                const float a0 = ib[(size_t)h * p.L], a1 = ib[(size_t)(nh + h) * p.L];
                float bb = 0.f, s = 0.f;
#pragma unroll
                for (int r = 0; r < 8; ++r) {       // o[h] and o[nh + h] without a dynamic register index
                    if (r == h) bb = o[r] + be[r];
                    if (r == nh + h) s = o[r] + be[r];
                }
                const float y1 = fmaf(expf(s), a1, bb);
                if (p.log_s) p.log_s[((size_t)b * nh + h) * p.L + t] = s;
                sum_s += (double)s;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    if (r == h) v[r] = a0;
                    if (r == nh + h) v[r] = y1;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (r < p.n_peel) {
                if (p.z) p.z[((size_t)b * p.G + p.zoff + r) * p.L + t] = v[r];
                sum_z += (double)v[r] * (double)v[r];
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (r < Cn) {
                float y = 0.f;
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c >= p.n_peel && c < C) y = fmaf(wi[r * Cn + c - p.n_peel], v[c], y);
                p.dst[((size_t)b * Cn + r) * p.L + t] = y;
            }
        }
    }
    if (!p.part_s) return;                         // uniform
    sum_s = wg_wave_sum(sum_s);
    sum_z = wg_wave_sum(sum_z);
    __syncthreads();                               // every thread is done with `we`: its first 64 bytes carry the waves' sums
    double* red = reinterpret_cast<double*>(we);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = sum_s; red[4 + (threadIdx.x >> 6)] = sum_z; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t slot = (size_t)b * gridDim.x + blockIdx.x;
        p.part_s[slot] = ((red[0] + red[1]) + red[2]) + red[3];
        p.part_z[slot] = ((red[4] + red[5]) + red[6]) + red[7];
    }
}

// Per item (one wave each): sums[b][k] = sum of flow k's partials (lane j takes blocks j, j + 64, .. ascending, then the xor tree),
// sums[b][n_flows] = sum z^2 (flows ascending), item[b] = (sum z^2 / (2 sigma^2) - sum_k sums[b][k] - L * sum_k logdet W_k) / (G * L).
__global__ void __launch_bounds__(64) wg_nll_item_kernel(const double* __restrict__ part_s, const double* __restrict__ part_z, int n_flows, int B, int nblk,
                                                        long L, int G, float sigma, const float* __restrict__ logdet_w, double* __restrict__ sums,
                                                        double* __restrict__ item, float* __restrict__ nll_item) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double z2 = 0.0, stot = 0.0, ld = 0.0;
    for (int k = 0; k < n_flows; ++k) {
        const size_t base = ((size_t)k * B + b) * nblk;
        double ps = 0.0, pz = 0.0;
        for (int j = lane; j < nblk; j += 64) { ps += part_s[base + j]; pz += part_z[base + j]; }
        ps = wg_wave_sum(ps);
        pz = wg_wave_sum(pz);
        if (lane == 0) sums[(size_t)b * (n_flows + 1) + k] = ps;
        stot += ps; z2 += pz; ld += (double)logdet_w[k];
    }
    if (lane != 0) return;
    sums[(size_t)b * (n_flows + 1) + n_flows] = z2;
    const double nll = (z2 / (2.0 * (double)sigma * (double)sigma) - stot - (double)L * ld) / ((double)G * (double)L);
    item[b] = nll;
    if (nll_item) nll_item[b] = (float)nll;
}

// logdet[k] = B * L * logdet W_k (glow.py:100), and loss = mean over the items of item[b] (thread j takes items j, j + 256, ..
// ascending, then a tree in LDS): WaveGlowLoss (glow.py:48-59) from the sums above.
__global__ void __launch_bounds__(256) wg_nll_loss_kernel(const double* __restrict__ item, int B, long L, int n_flows, const float* __restrict__ logdet_w,
                                                         float* __restrict__ logdet, float* __restrict__ loss) {
    __shared__ double red[256];
    if (logdet && threadIdx.x < n_flows) logdet[threadIdx.x] = (float)((double)B * (double)L * (double)logdet_w[threadIdx.x]);
    if (!loss) return;                             // uniform
    double acc = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) acc += item[b];
    const double sum = wg_tree_sum(red, acc);
    if (threadIdx.x == 0) loss[0] = (float)(sum / (double)B);
}

// out[m] = log |det w[m]| of n matrices [c][c], c <= 8: LU with partial pivoting in fp64, sum of log |u_ii| rounded to fp32; NaN
// for a negative determinant and -inf for a singular matrix, as torch.logdet gives.  One workgroup per matrix, the matrix in LDS.
__global__ void __launch_bounds__(64) wg_logdet_kernel(const float* __restrict__ w, int c, float* __restrict__ out) {
    __shared__ double m[64];
    if ((int)threadIdx.x < c * c) m[threadIdx.x] = (double)w[(size_t)blockIdx.x * c * c + threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double acc = 0.0;
    bool negative = false, singular = false;
    for (int i = 0; i < c && !singular; ++i) {
        int piv = i;                                // `>` is false for a NaN: one off the diagonal is never chosen here, it spreads
        for (int r = i + 1; r < c; ++r)             // through the elimination below and is met as a pivot (or in the sum) later
            if (fabs(m[r * c + i]) > fabs(m[piv * c + i])) piv = r;
        if (piv != i) {
            for (int j = 0; j < c; ++j) { const double tmp = m[i * c + j]; m[i * c + j] = m[piv * c + j]; m[piv * c + j] = tmp; }
            negative = !negative;
        }
        const double u = m[i * c + i];
        if (u != u) { negative = true; break; }     // a NaN in the matrix gives NaN
        if (u == 0.0) { singular = true; break; }
        if (u < 0.0) negative = !negative;
        acc += log(fabs(u));
        for (int r = i + 1; r < c; ++r) {
            const double f = m[r * c + i] / u;
            for (int j = i + 1; j < c; ++j) m[r * c + j] -= f * m[i * c + j];
        }
    }
    const double inf = __builtin_inf();
    out[blockIdx.x] = singular ? (float)-inf : (negative ? __builtin_nanf("") : (float)acc);
}

// the torch layouts of the forward's packs: gated Conv1d [2nc][nc][3] + the layer's rows of cond [2nc][n_cond], two gates rows
// apart; res_skip Conv1d [rows][nc][1]; upsample ConvTranspose1d [Cin][Cout][1024], row = channel * 256 + phase, tap j at phase + 256 j
int wg_pack(int kind, const float* w0, const float* w1, float* out, int rows, int k0, int k1, hipStream_t s) {
    T2_REQUIRE(w0 && out && (kind != kWgGated || w1), "waveglow pack: null pointer");
    SlabPack p{};
    p.out = out; p.gates = 1; p.rows = rows; p.split = 1; p.s0.w = w0; p.s0.K = k0; p.s0.taps = 1;
    if (kind == kWgGated) {
        p.gates = 2; p.s0.taps = 3; p.s0.gs = (long)rows * k0 * 3; p.s0.rhi = (long)k0 * 3; p.s0.ks = 3; p.s0.ts = 1;
        p.s1.w = w1; p.s1.K = k1; p.s1.gs = (long)rows * k1; p.s1.rhi = k1; p.s1.ks = 1;
    } else if (kind == kWgResSkip) {
        p.s0.rhi = k0; p.s0.ks = 1;
    } else {
        p.rows = rows * kWgUpStride; p.split = kWgUpStride; p.s0.taps = kWgUpTaps;
        p.s0.rhi = kWgUpK; p.s0.rlo = 1; p.s0.ks = (long)k0 * kWgUpK; p.s0.ts = kWgUpStride;
    }
    return slab_pack(p, s);
}

template <int MODE>
static int wg_launch(const WgGemm& p, int B, hipStream_t s) {
    return slab_launch(wg_gemm_kernel<4, MODE>, wg_gemm_kernel<2, MODE>, wg_gemm_kernel<1, MODE>, p, p.mtiles, p.Nq, 1, B, s);
}

int wg_gated(int B, int nc, int n_cond, long L, int d, int raw, const float* x, const float* spect, const float* packed, const float* b_in,
                    const float* b_cond, float* y, hipStream_t s, float* keep_t, float* keep_g) {
    T2_TRY_RC(wg_gated_check(B, nc, n_cond, L, d));
    T2_REQUIRE(x && spect && packed && b_in && b_cond && y, "waveglow gated conv: null pointer");
    WgGemm p{};
    p.x0 = x; p.x1 = spect; p.wp = packed; p.bias0 = b_in; p.bias1 = b_cond; p.y0 = y;
    p.C0 = nc; p.C1 = n_cond; p.N = p.Nq = (int)L; p.taps = 3; p.coff0 = 0; p.cstep = d; p.halo = d;
    p.rows = nc; p.mtiles = (nc + 31) / 32; p.nch0 = slab_chunks(nc); p.nch1 = slab_chunks(n_cond); p.raw = raw; p.s0 = keep_t; p.s1 = keep_g;
    return wg_launch<kWgGated>(p, B, s);
}

int wg_res_skip(int B, int nc, long L, int first, int last, const float* acts, const float* packed, const float* bias, float* x, float* out,
                       hipStream_t s, const float* x_from) {
    const char* who = "waveglow res_skip";
    T2_TRY_RC(wg_check_common(who, B, L));
    T2_TRY_RC(wg_check_nc(who, nc));
    T2_REQUIRE(acts && packed && bias && out && (last || x), "%s: null pointer", who);
    WgGemm p{};
    p.x0 = acts; p.wp = packed; p.bias0 = bias; p.y0 = x; p.y1 = out; p.res = x_from ? x_from : x;
    p.C0 = nc; p.N = p.Nq = (int)L; p.taps = 1;
    p.rows = last ? nc : 2 * nc; p.mtiles = (p.rows + 31) / 32; p.nch0 = slab_chunks(nc); p.first = first; p.last = last;
    return wg_launch<kWgResSkip>(p, B, s);
}

// n_samples: the samples of the transposed conv that are regrouped, T*256 for inference; up to T*256 + 768 (the trailing ones,
// frames q = T .. T+2 whose taps reach back into the mel) for the forward direction.  The loader zero-fills past the row.
int wg_upsample(int B, int n_mel, int T, int G, long n_samples, const float* mel, const float* packed, const float* bias, float* spect, hipStream_t s) {
    const char* who = "waveglow upsample";
    T2_TRY_RC(wg_check_common(who, B, T));
    T2_REQUIRE(n_mel >= 1 && n_mel <= 512, "%s: n_mel_channels=%d outside 1..512", who, n_mel);
    T2_TRY_RC(wg_check_group(who, G));
    T2_REQUIRE(n_samples / G >= 1, "%s: %ld samples give no whole group of %d", who, n_samples, G);
    T2_REQUIRE(n_samples <= (long)T * kWgUpStride + kWgUpK - kWgUpStride, "%s: %ld samples, %d frames give %ld", who, n_samples, T,
               (long)T * kWgUpStride + kWgUpK - kWgUpStride);
    T2_REQUIRE(mel && packed && bias && spect, "%s: null pointer", who);
    WgGemm p{};
    p.x0 = mel; p.wp = packed; p.bias0 = bias; p.y0 = spect;
    p.C0 = n_mel; p.N = T; p.taps = kWgUpTaps; p.coff0 = kWgUpTaps - 1; p.cstep = -1; p.halo = kWgUpTaps - 1;
    p.rows = n_mel * kWgUpStride; p.mtiles = p.rows / 32; p.nch0 = slab_chunks(n_mel); p.G = G; p.Lg = n_samples / G;
    p.Nq = (int)std::max((long)T, (p.Lg * G + kWgUpStride - 1) / kWgUpStride);
    return wg_launch<kWgUpsample>(p, B, s);
}

int wg_start(int B, int nc, int ctot, int n_half, long L, float scale, const float* audio, const float* w, const float* bias, float* x, hipStream_t s) {
    hipLaunchKernelGGL(wg_start_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)((nc + 31) / 32), (unsigned)B), dim3(256), 0, s, audio, ctot, n_half,
                       scale, w, bias, x, nc, L);
    T2_LAUNCH_CHECK();
    return 0;
}

int wg_couple(int B, const WgCouple& p, hipStream_t s) {
    const char* who = "waveglow coupling";
    T2_TRY_RC(wg_check_common(who, B, p.L));
    T2_TRY_RC(wg_check_nc(who, p.nc));
    T2_TRY_RC(wg_check_half(who, p.n_half));
    T2_REQUIRE(p.n_early >= 0 && p.n_early + 2 * p.n_half <= 8, "%s: %d early channels on top of %d exceed 8", who, p.n_early, 2 * p.n_half);
    T2_REQUIRE(p.out && p.w_end && p.b_end && p.in && p.winv && (p.dst || p.inter) && (p.n_early == 0 || (p.z && p.dst)), "%s: null pointer", who);
    hipLaunchKernelGGL(wg_couple_kernel, dim3((unsigned)((p.L + 255) / 256), (unsigned)B), dim3(256), 0, s, p);
    T2_LAUNCH_CHECK();
    return 0;
}

int wg_head(int B, int G, long N, const float* audio, const float* w, float* dst, hipStream_t s) {
    const char* who = "waveglow head";
    T2_TRY_RC(wg_check_group(who, G));
    T2_REQUIRE(N >= G, "%s: n_samples=%ld is shorter than one group of %d", who, N, G);
    T2_TRY_RC(wg_check_common(who, B, N / G));
    T2_REQUIRE(audio && w && dst, "%s: null pointer", who);
    hipLaunchKernelGGL(wg_head_kernel, dim3((unsigned)((N / G + 255) / 256), (unsigned)B), dim3(256), 0, s, audio, w, dst, G, N, N / G);
    T2_LAUNCH_CHECK();
    return 0;
}

int wg_tail(int B, const WgTail& p, hipStream_t s) {
    const char* who = "waveglow forward tail";
    const int C = 2 * p.n_half;
    T2_TRY_RC(wg_check_common(who, B, p.L));
    T2_TRY_RC(wg_check_nc(who, p.nc));
    T2_TRY_RC(wg_check_half(who, p.n_half));
    T2_TRY_RC(wg_check_peel(who, p.n_peel, C, p.zoff, p.G));
    T2_REQUIRE(p.out && p.w_end && p.b_end && p.in && (p.n_peel == C || (p.wnext && p.dst)) && (p.n_peel == 0 || p.z || p.part_z) &&
               !p.part_s == !p.part_z, "%s: null pointer", who);
    hipLaunchKernelGGL(wg_tail_kernel, dim3((unsigned)((p.L + 255) / 256), (unsigned)B), dim3(256), 0, s, p);
    T2_LAUNCH_CHECK();
    return 0;
}

int wg_logdet(const float* w, int c, int n, float* out, hipStream_t s) {
    T2_REQUIRE(c >= 1 && c <= 8, "waveglow logdet: matrices of %d x %d, at most 8 x 8 are taken", c, c);
    T2_REQUIRE(n >= 1 && w && out, "waveglow logdet: %d matrices or a null pointer", n);
    hipLaunchKernelGGL(wg_logdet_kernel, dim3((unsigned)n), dim3(64), 0, s, w, c, out);
    T2_LAUNCH_CHECK();
    return 0;
}

int wg_nll_item(int n_flows, int B, int nblk, long L, int G, float sigma, const double* part_s, const double* part_z, const float* logdet_w,
                       double* sums, double* item, float* nll_item, hipStream_t s) {
    hipLaunchKernelGGL(wg_nll_item_kernel, dim3((unsigned)B), dim3(64), 0, s, part_s, part_z, n_flows, B, nblk, L, G, sigma, logdet_w, sums, item, nll_item);
    T2_LAUNCH_CHECK();
    return 0;
}

int wg_nll_loss(int n_flows, int B, long L, const double* item, const float* logdet_w, float* logdet, float* loss, hipStream_t s) {
    hipLaunchKernelGGL(wg_nll_loss_kernel, dim3(1), dim3(256), 0, s, item, B, L, n_flows, logdet_w, logdet, loss);
    T2_LAUNCH_CHECK();
    return 0;
}

// ---- the backward of the forward direction: gradients of every folded tensor from dz and the dlog_s[k]
// Weight gradient  C[m][n] = sum_b sum_l A[b][m][l] * Bop[b][n][l + shift_n]: both operands are contiguous along the reduction, so
// a workgroup stages 128 rows of each over 32 time steps in LDS (coalesced along time, guarded at both ends) and the MFMA reads
// its 32 rows at one time step: lanes stride by the row stride, 34 floats, which puts rows 0..31 of both k-halves on 64 distinct
// banks.  The columns n come in segments (x at three shifts, spect, a row of ones whose column is the bias gradient); a tile of
// 128 columns lies inside one segment.  The reduction over (item, chunk of 32 steps) is split into `nsplit` contiguous runs that
// depend on the shape alone; every run writes a partial plane, which wg_wgrad_reduce_kernel adds in ascending order in fp64.
static_assert(kWgGradStride % 4 == 2 && kWgGradStride >= kWgGradTL, "rows 0..31 x 2 k-halves on 64 distinct banks");

__global__ void __launch_bounds__(256) wg_wgrad_kernel(WgGrad p) {
    __shared__ float As[kWgGradTile * kWgGradStride], Bs[kWgGradTile * kWgGradStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave & 1, wn = wave >> 1, hk = lane >> 5;
    const int mt = blockIdx.x % p.mtiles, nt = blockIdx.x / p.mtiles;
    int si = 0;
    for (int s = 1; s < p.nseg; ++s)
        if (nt >= p.seg[s].tile0) si = s;
    const WgGradSeg sg = p.seg[si];
    const int ch0 = (nt - sg.tile0) * kWgGradTile, m0 = mt * kWgGradTile;
    const int total = p.B * p.nchunk, u0 = blockIdx.y * p.per, u1 = min(total, u0 + p.per);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) { acc[i][0] = f32x16{0}; acc[i][1] = f32x16{0}; }
    for (int u = u0; u < u1; ++u) {
        const int b = u / p.nchunk;
        const long l0 = (long)(u % p.nchunk) * kWgGradTL;
        if (u > u0) __syncthreads();               // every wave is done reading the previous slabs
        // 16-byte loads where L, the shift and the base address are multiples of four floats (a quad is then inside the row or
        // outside it as a whole); element by element otherwise.  Both branches are uniform over the workgroup.
        if (p.avec) {
            for (int idx = threadIdx.x; idx < kWgGradTile * kWgGradTL / 4; idx += 256) {
                const int row = idx / (kWgGradTL / 4), col = idx % (kWgGradTL / 4) * 4, m = m0 + row;
                const long t = l0 + col;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (m < p.M && t < p.L) v = *reinterpret_cast<const f32x4*>(p.a + ((size_t)b * p.Mbuf + m) * p.L + t);
                float* d = As + row * kWgGradStride + col;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        } else {
            for (int idx = threadIdx.x; idx < kWgGradTile * kWgGradTL; idx += 256) {
                const int row = idx / kWgGradTL, col = idx % kWgGradTL, m = m0 + row;
                const long t = l0 + col;
                As[row * kWgGradStride + col] = (m < p.M && t < p.L) ? p.a[((size_t)b * p.Mbuf + m) * p.L + t] : 0.f;
            }
        }
        if (sg.vec) {
            for (int idx = threadIdx.x; idx < kWgGradTile * kWgGradTL / 4; idx += 256) {
                const int row = idx / (kWgGradTL / 4), col = idx % (kWgGradTL / 4) * 4, ch = ch0 + row;
                const long t = l0 + col, tb = t + sg.shift;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (ch < sg.C && t < p.L && tb >= 0 && tb < p.L) {
                    if (sg.src) v = *reinterpret_cast<const f32x4*>(sg.src + ((size_t)b * sg.Cbuf + ch) * p.L + tb);
                    else v = f32x4{1.f, 1.f, 1.f, 1.f};
                }
                float* d = Bs + row * kWgGradStride + col;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        } else {
            for (int idx = threadIdx.x; idx < kWgGradTile * kWgGradTL; idx += 256) {
                const int row = idx / kWgGradTL, col = idx % kWgGradTL, ch = ch0 + row;
                const long t = l0 + col, tb = t + sg.shift;
                float v = 0.f;
                if (ch < sg.C && t < p.L && tb >= 0 && tb < p.L) v = sg.src ? sg.src[((size_t)b * sg.Cbuf + ch) * p.L + tb] : 1.f;
                Bs[row * kWgGradStride + col] = v;
            }
        }
        __syncthreads();
        const float* ap = As + (wm * 64 + (lane & 31)) * kWgGradStride + hk;
        const float* bp = Bs + (wn * 64 + (lane & 31)) * kWgGradStride + hk;
#pragma unroll
        for (int kk = 0; kk < kWgGradTL / 2; ++kk) {
            const float a0 = ap[2 * kk], a1 = ap[32 * kWgGradStride + 2 * kk], b0 = bp[2 * kk], b1 = bp[32 * kWgGradStride + 2 * kk];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // lane holds column (of C) lane & 31 and rows (e&3) + 8*(e>>2) + 4*hk of each 32x32 tile
    float* pp = p.part + (size_t)blockIdx.y * p.M * p.Ntot;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ch = ch0 + wn * 64 + j * 32 + (lane & 31);
            if (ch >= sg.C) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hk;
                if (m < p.M) pp[(size_t)m * p.Ntot + sg.col0 + ch] = acc[i][j][e];
            }
        }
}

__global__ void __launch_bounds__(256) wg_wgrad_reduce_kernel(WgGrad p) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, plane = (size_t)p.M * p.Ntot;
    if (idx >= plane) return;
    const int m = (int)(idx / p.Ntot), n = (int)(idx % p.Ntot);
    double acc = 0.0;
    for (int y = 0; y < p.nsplit; ++y) acc += (double)p.part[(size_t)y * plane + idx];
    int si = 0;
    for (int s = 1; s < p.nseg; ++s)
        if (n >= p.seg[s].col0) si = s;
    const WgGradDst d = p.dst[si];
    const size_t o = (size_t)m * d.rs + (size_t)(n - p.seg[si].col0) * d.cs;
    d.dst[o] = (float)acc;
    if (d.dst2) d.dst2[o] = (float)acc;
}

// sums of the products dn[r] * v[c] (r, c < Cn) over the wave, in fp64 from exact products, to part[r * Cn + c] (lane 0 writes)
__device__ __forceinline__ void wg_mix_grad(const float (&dn)[8], const float (&vn)[8], int Cn, double* part) {
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (r < Cn && c < Cn) {
                const double v = wg_wave_sum((double)dn[r] * (double)vn[c]);
                if ((threadIdx.x & 63) == 0) part[r * Cn + c] = v;
            }
}

// One flow's tail backwards, one thread per (item, column).  dV, the gradient on cat(a0, a1'), is dz for the channels that left
// for z and W_{k+1}^T d(audio_in_{k+1}) for the rest; (b, s) = end(out) is recomputed as the forward computes it;
// db = dV[n_half:], ds = db * exp(s) * a1 + dlog_s, da1 = db * exp(s), d_out = W_end^T [db; ds].  The sums over (item, column)
// -- dW_end = [db; ds] out^T, db_end, dW_{k+1} = d(audio_in_{k+1}) v[n_peel:]^T -- leave as one fp64 partial per wave.
__global__ void __launch_bounds__(256) wg_tail_bwd_kernel(WgTailBwd p) {
    __shared__ float we[8 * 512], be[8], wi[64];
    const int nh = p.n_half, C = 2 * nh, Cn = C - p.n_peel;
    wg_load_end(we, be, wi, p.w_end, p.b_end, p.wnext, C, p.nc, Cn);
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = t < p.L;
    const int b = blockIdx.y;
    const float* ob = p.out + (size_t)b * p.nc * p.L + (valid ? t : 0);
    float e[8], v[8], dn[8], dV[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { e[r] = 0.f; v[r] = 0.f; dn[r] = 0.f; dV[r] = 0.f; }
    if (valid) {
        float o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) o[r] = 0.f;
        for (int c = 0; c < p.nc; ++c) {
            const float x = ob[(size_t)c * p.L];
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (r < C) o[r] = fmaf(we[r * p.nc + c], x, o[r]);
        }
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (r < Cn) dn[r] = p.dnext[((size_t)b * Cn + r) * p.L + t];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (r < p.n_peel) {
                dV[r] = p.dz ? p.dz[((size_t)b * p.G + p.zoff + r) * p.L + t] : 0.f;
            } else if (r < C) {
                float y = 0.f;
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (q < Cn) y = fmaf(wi[q * Cn + r - p.n_peel], dn[q], y);
                dV[r] = y;
            }
        }
        const float* ib = p.in + (size_t)b * C * p.L + t;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            if (h < nh) {
                const float a0 = ib[(size_t)h * p.L], a1 = ib[(size_t)(nh + h) * p.L];
                float bb = 0.f, s = 0.f, db = 0.f, da0 = 0.f;
                wg_get_pair_plus(o, be, h, nh, bb, s);
                wg_get_pair(dV, h, nh, da0, db);
                const float es = expf(s), da1 = db * es;
                const float ds = fmaf(da1, a1, p.dlog_s ? p.dlog_s[((size_t)b * nh + h) * p.L + t] : 0.f);
                const float y1 = fmaf(es, a1, bb);
                p.d_in[((size_t)b * C + h) * p.L + t] = da0;
                p.d_in[((size_t)b * C + nh + h) * p.L + t] = da1;
                wg_put_pair(v, h, nh, a0, y1);
                wg_put_pair(e, h, nh, db, ds);
            }
        }
    }
    const int lane = threadIdx.x & 63;
    double* part = p.part + (((size_t)b * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6)) * ((size_t)C * p.nc + C + Cn * Cn);
    for (int c = 0; c < p.nc; ++c) {
        const float x = valid ? ob[(size_t)c * p.L] : 0.f;
        float d = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (r < C) d = fmaf(we[r * p.nc + c], e[r], d);
        if (valid) p.d_out[((size_t)b * p.nc + c) * p.L + t] = d;
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (r < C) {
                const double w = wg_wave_sum((double)e[r] * (double)x);
                if (lane == 0) part[(size_t)r * p.nc + c] = w;
            }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r)
        if (r < C) {
            const double w = wg_wave_sum((double)e[r]);
            if (lane == 0) part[(size_t)C * p.nc + r] = w;
        }
    float vn[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        vn[c] = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (r == p.n_peel + c) vn[c] = v[r];
    }
    wg_mix_grad(dn, vn, Cn, part + (size_t)C * p.nc + C);
}

// dW_0 [G][G] = sum d(audio_in_0)[b, r, l] * audio[b, l*G + g]: the partials of flow 0's mix, whose input is the regrouped audio
__global__ void __launch_bounds__(256) wg_head_bwd_kernel(const float* __restrict__ d_in, const float* __restrict__ audio, int G, long N, long L,
                                                         double* __restrict__ part) {
    const long l = (long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    float dn[8], vn[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const bool ok = l < L && g < G;
        dn[g] = ok ? d_in[((size_t)b * G + g) * L + l] : 0.f;
        vn[g] = ok ? audio[(size_t)b * N + (size_t)l * G + g] : 0.f;
    }
    wg_mix_grad(dn, vn, G, part + (((size_t)b * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6)) * ((size_t)G * G));
}

// dst_j[i] = sum over the slots (ascending, fp64) of part[slot][off_j + i], rounded to fp32 once: finishes the partials above
struct WgFinish { const double* part; size_t nslots, stride; float* dst[3]; int n[3]; };
__global__ void __launch_bounds__(256) wg_finish_kernel(WgFinish p) {
    int idx = blockIdx.x * 256 + threadIdx.x;
    const int at = idx;
    int j = 0;
    while (j < 3 && idx >= p.n[j]) { idx -= p.n[j]; ++j; }
    if (j == 3) return;
    double acc = 0.0;
    for (size_t sl = 0; sl < p.nslots; ++sl) acc += p.part[sl * p.stride + at];
    if (p.dst[j]) p.dst[j][idx] = (float)acc;
}

// d(audio_in)[b, h, t] += sum_c w_start[c][h] * dx[b, c, t] (c ascending), h < n_half: the rows of a0 that fed `start`
__global__ void __launch_bounds__(256) wg_start_bwd_kernel(const float* __restrict__ dx, const float* __restrict__ w, float* __restrict__ d_in, int nc,
                                                          int ctot, int n_half, long L) {
    __shared__ float ws[512 * 4];
    for (int i = threadIdx.x; i < nc * n_half; i += 256) ws[i] = w[i];
    __syncthreads();
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= L) return;
    const int b = blockIdx.y;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nc; ++c) {
        const float d = dx[((size_t)b * nc + c) * L + t];
#pragma unroll
        for (int h = 0; h < 4; ++h)
            if (h < n_half) a[h] = fmaf(ws[c * n_half + h], d, a[h]);
    }
#pragma unroll
    for (int h = 0; h < 4; ++h)
        if (h < n_half) d_in[((size_t)b * ctot + h) * L + t] += a[h];
}

// The upsample's weight gradient: dW_up[ci][co][r + 256 m] = sum_b sum_q mel[b, ci, q - m] * d_up[b, co, 256 q + r] with
// d_up[b, co, s] = d_spect[b, co*G + s % G, s / G] for s < Lg*G (the frames q past T, whose taps reach back into the mel, included).
// One thread per (ci, co, tap), b then q ascending, in fp64: K is only B * (T + 3).
__global__ void __launch_bounds__(256) wg_up_bwd_kernel(const float* __restrict__ mel, const float* __restrict__ d_spect, float* __restrict__ dw, int B,
                                                       int n_mel, int T, int G, long Lg, int Nq) {
    const int j = blockIdx.x * 256 + threadIdx.x, co = blockIdx.y, ci = blockIdx.z;      // j < 1024: one workgroup row per m
    const int r = j % kWgUpStride, m = j / kWgUpStride;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* mb = mel + ((size_t)b * n_mel + ci) * T;
        const float* db = d_spect + (size_t)b * n_mel * G * Lg + (size_t)co * G * Lg;
        for (int q = m; q < Nq && q - m < T; ++q) {
            const long s = (long)q * kWgUpStride + r, l = s / G;
            if (l < Lg) acc += (double)mb[q - m] * (double)db[(size_t)(s % G) * Lg + l];
        }
    }
    dw[((size_t)ci * n_mel + co) * kWgUpK + j] = (float)acc;
}
// db_up[co] = sum over b, the G rows of co and l of d_spect: thread j takes elements j, j + 256, .. ascending, then a tree in LDS
__global__ void __launch_bounds__(256) wg_up_bias_bwd_kernel(const float* __restrict__ d_spect, float* __restrict__ db, int B, int n_mel, int G, long Lg) {
    __shared__ double red[256];
    const int co = blockIdx.x;
    const size_t row = (size_t)G * Lg;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* p = d_spect + ((size_t)b * n_mel + co) * row;
        for (size_t i = threadIdx.x; i < row; i += 256) acc += (double)p[i];
    }
    const double sum = wg_tree_sum(red, acc);
    if (threadIdx.x == 0) db[co] = (float)sum;
}

// the transposed operands of the data gradients.  conv^T: rows c < nc, k = r < 2nc, tap j' reads du at l + (j' - 1) d, which W_in[r][c][2 - j'] multiplies
int wg_pack_conv_t(const float* w_in, float* out, int nc, hipStream_t s) {
    SlabPack p{}; p.out = out; p.gates = 1; p.rows = nc; p.split = 1;
    p.s0.w = w_in; p.s0.K = 2 * nc; p.s0.taps = 3; p.s0.base = 2; p.s0.rhi = 3; p.s0.ks = (long)nc * 3; p.s0.ts = -1;
    return slab_pack(p, s);
}
int wg_pack_cond_t(const float* w_cond_i, float* out, int nc, int n_cond, hipStream_t s) {      // [2nc][n_cond] -> rows n_cond, K = 2nc
    SlabPack p{}; p.out = out; p.gates = 1; p.rows = n_cond; p.split = 1;
    p.s0.w = w_cond_i; p.s0.K = 2 * nc; p.s0.taps = 1; p.s0.rhi = 1; p.s0.ks = n_cond;
    return slab_pack(p, s);
}
int wg_pack_rs_t(const float* w_rs, float* out, int nc, int last, hipStream_t s) {             // [2nc | nc][nc] -> rows nc, K = nc (x part) | nc (out part)
    SlabPack p{}; p.out = out; p.gates = 1; p.rows = nc; p.split = 1;
    p.s0.w = w_rs; p.s0.K = nc; p.s0.taps = 1; p.s0.rhi = 1; p.s0.ks = nc;
    if (!last) { p.s1.w = w_rs + (size_t)nc * nc; p.s1.K = nc; p.s1.rhi = 1; p.s1.ks = nc; }
    return slab_pack(p, s);
}

int wg_wgrad(const WgGrad& p, hipStream_t s) {
    T2_REQUIRE(p.a && p.part && (long)p.B * p.nchunk <= INT32_MAX, "waveglow weight gradient: null pointer or too many chunks");
    hipLaunchKernelGGL(wg_wgrad_kernel, dim3((unsigned)(p.mtiles * p.ntiles), (unsigned)p.nsplit), dim3(256), 0, s, p);
    T2_LAUNCH_CHECK();
    return 0;
}
int wg_wgrad_reduce(const WgGrad& p, hipStream_t s) {
    hipLaunchKernelGGL(wg_wgrad_reduce_kernel, dim3((unsigned)(((size_t)p.M * p.Ntot + 255) / 256)), dim3(256), 0, s, p);
    T2_LAUNCH_CHECK();
    return 0;
}
int wg_gate_bwd(int B, int nc, long L, int last, const float* dx, const float* d_out, const float* packed_t, const float* t, const float* g, float* du,
                       float* acts, hipStream_t s) {
    const char* who = "waveglow gate backward";
    T2_TRY_RC(wg_check_common(who, B, L));
    T2_TRY_RC(wg_check_nc(who, nc));
    T2_REQUIRE(d_out && (last || dx) && packed_t && t && g && du && acts, "%s: null pointer", who);
    WgGemm p{};
    p.x0 = last ? d_out : dx; p.x1 = last ? nullptr : d_out; p.wp = packed_t; p.y0 = du; p.y1 = acts;
    p.s0 = const_cast<float*>(t); p.s1 = const_cast<float*>(g);
    p.C0 = nc; p.C1 = last ? 0 : nc; p.N = p.Nq = (int)L; p.taps = 1;
    p.rows = nc; p.mtiles = (nc + 31) / 32; p.nch0 = slab_chunks(nc); p.nch1 = last ? 0 : slab_chunks(nc);
    return wg_launch<kWgGateBwd>(p, B, s);
}
// y [B, rows, L] (+)= W^T du: rows = nc with the flipped taps at distance d (dx), or rows = n_cond with one tap (d_spect)
int wg_data_bwd(int B, int rows, int nc, long L, int taps, int d, int first, const float* du, const float* packed_t, float* y, hipStream_t s) {
    const char* who = "waveglow conv backward";
    T2_TRY_RC(wg_check_common(who, B, L));
    T2_TRY_RC(wg_check_nc(who, nc));
    T2_REQUIRE(rows >= 1 && (taps == 1 || (taps == 3 && d >= 1 && d <= kWgMaxD && (d & (d - 1)) == 0)), "%s: rows=%d, taps=%d, d=%d", who, rows, taps, d);
    T2_REQUIRE(du && packed_t && y, "%s: null pointer", who);
    WgGemm p{};
    p.x0 = du; p.wp = packed_t; p.y0 = y; p.first = first;
    p.C0 = 2 * nc; p.N = p.Nq = (int)L; p.taps = taps; p.coff0 = 0; p.cstep = taps == 3 ? d : 0; p.halo = taps == 3 ? d : 0;
    p.rows = rows; p.mtiles = (rows + 31) / 32; p.nch0 = slab_chunks(2 * nc);
    return wg_launch<kWgAccum>(p, B, s);
}

int wg_tail_bwd(int B, const WgTailBwd& p, hipStream_t s) {
    const char* who = "waveglow tail backward";
    const int C = 2 * p.n_half;
    T2_TRY_RC(wg_check_common(who, B, p.L));
    T2_TRY_RC(wg_check_nc(who, p.nc));
    T2_TRY_RC(wg_check_half(who, p.n_half));
    T2_TRY_RC(wg_check_peel(who, p.n_peel, C, p.zoff, p.G));
    T2_REQUIRE(p.out && p.w_end && p.b_end && p.in && p.d_out && p.d_in && p.part && (p.n_peel == C || (p.wnext && p.dnext)), "%s: null pointer", who);
    hipLaunchKernelGGL(wg_tail_bwd_kernel, dim3((unsigned)((p.L + 255) / 256), (unsigned)B), dim3(256), 0, s, p);
    T2_LAUNCH_CHECK();
    return 0;
}
int wg_finish(const double* part, size_t nslots, size_t stride, float* d0, int n0, float* d1, int n1, float* d2, int n2, hipStream_t s) {
    WgFinish p{part, nslots, stride, {d0, d1, d2}, {n0, n1, n2}};
    if (n0 + n1 + n2 == 0) return 0;
    hipLaunchKernelGGL(wg_finish_kernel, dim3((unsigned)((n0 + n1 + n2 + 255) / 256)), dim3(256), 0, s, p);
    T2_LAUNCH_CHECK();
    return 0;
}
int wg_head_bwd(int B, int G, long N, const float* d_in, const float* audio, double* part, float* dw, hipStream_t s) {
    const long L = N / G;
    const unsigned nblk = (unsigned)((L + 255) / 256);
    hipLaunchKernelGGL(wg_head_bwd_kernel, dim3(nblk, (unsigned)B), dim3(256), 0, s, d_in, audio, G, N, L, part);
    T2_LAUNCH_CHECK();
    return wg_finish(part, (size_t)B * nblk * 4, (size_t)G * G, dw, G * G, nullptr, 0, nullptr, 0, s);
}
int wg_start_bwd(int B, int nc, int ctot, int n_half, long L, const float* dx, const float* w, float* d_in, hipStream_t s) {
    hipLaunchKernelGGL(wg_start_bwd_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)B), dim3(256), 0, s, dx, w, d_in, nc, ctot, n_half, L);
    T2_LAUNCH_CHECK();
    return 0;
}
int wg_up_bwd(int B, int n_mel, int T, int G, long n_samples, const float* mel, const float* d_spect, float* dw, float* db, hipStream_t s) {
    const char* who = "waveglow upsample backward";
    T2_TRY_RC(wg_check_common(who, B, T));
    T2_REQUIRE(n_mel >= 1 && n_mel <= 512, "%s: n_mel_channels=%d outside 1..512", who, n_mel);
    T2_TRY_RC(wg_check_group(who, G));
    T2_REQUIRE(n_samples / G >= 1 && n_samples <= (long)T * kWgUpStride + kWgUpK - kWgUpStride, "%s: %ld samples, %d frames", who, n_samples, T);
    T2_REQUIRE(mel && d_spect && dw && db, "%s: null pointer", who);
    const long Lg = n_samples / G;
    const int Nq = (int)std::max((long)T, (Lg * G + kWgUpStride - 1) / kWgUpStride);
    hipLaunchKernelGGL(wg_up_bwd_kernel, dim3(kWgUpK / 256, (unsigned)n_mel, (unsigned)n_mel), dim3(256), 0, s, mel, d_spect, dw, B, n_mel, T, G, Lg, Nq);
    T2_LAUNCH_CHECK();
    hipLaunchKernelGGL(wg_up_bias_bwd_kernel, dim3((unsigned)n_mel), dim3(256), 0, s, d_spect, db, B, n_mel, G, Lg);
    T2_LAUNCH_CHECK();
    return 0;
}

}  // namespace t2
