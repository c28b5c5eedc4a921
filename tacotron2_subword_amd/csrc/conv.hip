// Conv1d(k) + BatchNorm1d + activation + dropout stacks on channels-last frames X[B*T, C]
// (Postnet.forward, model.py:65-70; the conv part of Encoder.forward, model.py:97-99), forward and
// backward, plus the embedding gather / gradient.
//
// The convolution is an implicit-im2col GEMM (gemm.hip, ConvAddr): no column matrix is
// materialised.  Which kernel runs it is plan_gemm's decision: the exact fp32 kernels in mode f32,
// in mode bf16 the bf16-source kernels on bf16 copies of the frames and the weights (forward and
// d(input): conv_a, 256- or 128-tiles; d(weight): the k-major 256-tile kernel with the frames as
// conv_b) or the converting kernel for shapes that are no whole tiles, in mode bf16x3 the same
// routes on split copies.  Weights are re-laid-out per call from the reference's [Cout, Cin, k] to
// [Cout, k*Cin] (and flipped/transposed for the data gradient) — 5 MB per layer.
// bf16 hand-offs (mode bf16, on request): instead of leaving every cast to gemm(), a layer writes
// its output also as bf16 for the next layer's product, dz once as bf16 for both backward
// products, and the re-laid-out weights straight as bf16 — only where gemm_handoff (gemm.hip)
// finds that the product keeps its kernel and split-K, so the results are the same bits.
// BatchNorm statistics use two passes (mean, then centred sum of squares) over two-stage
// fixed-order column reductions (common.h), so results are reproducible run to run.
#include "kernels.h"
#include <atomic>
#include <cstdlib>

namespace t2 {

namespace {

inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v && *v ? atoi(v) : dflt; }
inline int grid_for(size_t n, int block = 256, int cap = 8192) {
    size_t g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > (size_t)cap ? cap : g));
}

// The re-laid-out weights are written as fp32, or straight as the bf16 copy when the product takes one (OUT = __bf16: the
// round-to-nearest cast the staging kernels apply to the fp32 array).
// The element index and its three divisions are 32-bit (IDX = uint32_t) where Co*Ci*K < 2^31 (a 64-bit division by a
// run-time value is some 100 instructions, three of them per element for 1.3 M elements a layer), size_t otherwise.
// wp[co][dk*Ci + ci] = w[co][ci][dk]
template <class OUT, class IDX>
__global__ void permute_w_fwd_kernel(const float* __restrict__ w, OUT* __restrict__ wp, int Co, int Ci, int K) {
    const IDX n = (IDX)Co * Ci * K;
    for (IDX i = blockIdx.x * (IDX)blockDim.x + threadIdx.x; i < n; i += (IDX)gridDim.x * blockDim.x) {
        const IDX ci = i % (IDX)Ci, r = i / (IDX)Ci, dk = r % (IDX)K, co = r / (IDX)K;
        wp[i] = (OUT)w[(co * Ci + ci) * K + dk];
    }
}
// wt[ci][dk*Co + co] = w[co][ci][K-1-dk]     (data gradient = correlation with the flipped kernel)
template <class OUT, class IDX>
__global__ void permute_w_bwd_kernel(const float* __restrict__ w, OUT* __restrict__ wt, int Co, int Ci, int K) {
    const IDX n = (IDX)Co * Ci * K;
    for (IDX i = blockIdx.x * (IDX)blockDim.x + threadIdx.x; i < n; i += (IDX)gridDim.x * blockDim.x) {
        const IDX co = i % (IDX)Co, r = i / (IDX)Co, dk = r % (IDX)K, ci = r / (IDX)K;
        wt[i] = (OUT)w[(co * Ci + ci) * K + ((IDX)K - 1 - dk)];
    }
}
template <class OUT>
void permute_w(bool bwd, const float* w, OUT* out, int Co, int Ci, int K, hipStream_t s) {
    const size_t n = (size_t)Co * Ci * K;
    const dim3 grid(grid_for(n)), block(256);
    if (n < (1ull << 31)) {
        if (bwd) hipLaunchKernelGGL((permute_w_bwd_kernel<OUT, uint32_t>), grid, block, 0, s, w, out, Co, Ci, K);
        else hipLaunchKernelGGL((permute_w_fwd_kernel<OUT, uint32_t>), grid, block, 0, s, w, out, Co, Ci, K);
    } else {
        if (bwd) hipLaunchKernelGGL((permute_w_bwd_kernel<OUT, size_t>), grid, block, 0, s, w, out, Co, Ci, K);
        else hipLaunchKernelGGL((permute_w_fwd_kernel<OUT, size_t>), grid, block, 0, s, w, out, Co, Ci, K);
    }
}
// dw[co][ci][dk] = dwp[co][dk*Ci + ci]
__global__ void unpermute_dw_kernel(const float* __restrict__ dwp, float* __restrict__ dw, int Co, int Ci, int K) {
    const size_t n = (size_t)Co * Ci * K;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int dk = (int)(i % K); const size_t r = i / K; const int ci = (int)(r % Ci), co = (int)(r / Ci);
        dw[i] = dwp[((size_t)co * K + dk) * Ci + ci];
    }
}

struct BnElem {
    const float* z; const float* mean; const float* invstd; const float* gamma; const float* beta;
    int C; int act; float drop_p; RngKey key;
};
__device__ __forceinline__ float act_fwd(float u, int act) {
    return act == ACT_RELU ? fmaxf(u, 0.f) : (act == ACT_TANH ? tanhf(u) : u);
}

// Two-stage column reductions.  MODE 0: sum z.  MODE 1: sum (z-mean)^2.
// MODE 2 (backward): du = dy * keep/(1-p) * act'(u), written to `du`; s0 = sum du, s1 = sum du*xhat.
// One term of a column.  Which products are fused into the following add is part of the result's bits, so it is
// written out (fmaf) and nothing else is contracted: MODE 1 accumulates fma(d, d, a0); MODE 2 forms u and 1 - t*t
// with one fma each and adds the rounded product g*xh.
struct BnCol { float mean, inv, ga, be; };
template <int MODE>
__device__ __forceinline__ float colreduce_term(const BnElem& e, const BnCol& k, float scale, float z, float g, uint32_t i,
                                                float& a0, float& a1) {
#pragma clang fp contract(off)
    if (MODE == 0) a0 += z;
    else if (MODE == 1) { const float d = z - k.mean; a0 = fmaf(d, d, a0); }
    else {
        const float xh = (z - k.mean) * k.inv, u = fmaf(xh, k.ga, k.be);
        if (e.drop_p > 0.f) g = rng_keep(e.key, i, e.drop_p) ? g * scale : 0.f;
        if (e.act == ACT_RELU) g = u > 0.f ? g : 0.f;
        else if (e.act == ACT_TANH) { const float t = tanhf(u); g *= fmaf(-t, t, 1.0f); }
        const float gx = g * xh;
        a0 += g; a1 += gx;
    }
    return g;
}
// FIN (MODE 1): the mean is not read from e.mean but finished here, from the MODE 0 slab partials in `scratch`: the ordered
// sum over the slabs, divided by M, as colreduce_stage2_kernel does it.  The workgroups of slab 0 store it to mean_out, and
// the partials of this pass go behind the ones being read (other workgroups may still read those).
template <int MODE, int V, bool FIN>
__global__ void __launch_bounds__(kColThreads) colreduce_stage1_kernel(BnElem e, const float* __restrict__ dy, float* __restrict__ du,
                                                                       int M, int slabs, float* scratch, float* __restrict__ mean_out) {
    static_assert(!FIN || MODE == 1, "only the centred squares have a sum to finish");
    // rows requested ahead: 16 x 16 bytes per lane, twice (MODE 2 reads z and dy; its narrower lanes ask for 16 rows each)
    constexpr int R = MODE == 2 ? (V == 4 ? 8 : 16) : 16;
    static_assert(MODE == 2 || V != 2, "the forward passes run with 16-byte groups or one column per lane");
    const int C = e.C;
    const int lane = threadIdx.x % kColLanes, sub = threadIdx.x / kColLanes;
    const int c = (blockIdx.x * kColLanes + lane) * V;
    const int rows = (M + slabs - 1) / slabs;
    const int m0 = blockIdx.y * rows, m1 = min(M, m0 + rows);
    __shared__ float p0[4][kColLanes * V], p1[4][kColLanes * V];
    __shared__ float fin[FIN ? kColLanes * V : 1];
    if (FIN) {
        block_ordered_sums(scratch, C, slabs, blockIdx.x * kColLanes * V, kColLanes * V, fin);
        __syncthreads();
        scratch += (size_t)slabs * C;
    }
    float a0[V] = {}, a1[V] = {};
    if (c < C) {
        BnCol col[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (FIN) {
                col[k].mean = fin[lane * V + k] / (float)M;
                if (blockIdx.y == 0 && sub == 0) mean_out[c + k] = col[k].mean;
            } else
                col[k].mean = MODE >= 1 ? e.mean[c + k] : 0.f;
            col[k].inv = MODE == 2 ? e.invstd[c + k] : 0.f; col[k].ga = MODE == 2 ? e.gamma[c + k] : 0.f; col[k].be = MODE == 2 ? e.beta[c + k] : 0.f;
        }
        const float scale = e.drop_p > 0.f ? 1.0f / (1.0f - e.drop_p) : 1.0f;
        struct Row { ColVec<V> z, g; };
        rows_in_flight<R, Row>(m0 + sub, m1,
            [&](int m) {
                const size_t i = (size_t)m * C + c;
                Row r;
                r.z = load_cols<V>(e.z + i);
                if (MODE == 2) r.g = load_cols<V>(dy + i);
                return r;
            },
            [&](int m, const Row& r) {
                const size_t i = (size_t)m * C + c;
                ColVec<V> g;
#pragma unroll
                for (int k = 0; k < V; ++k)
                    g.v[k] = colreduce_term<MODE>(e, col[k], scale, r.z.v[k], MODE == 2 ? r.g.v[k] : 0.f, (uint32_t)(i + k), a0[k], a1[k]);
                if (MODE == 2) store_cols<V>(du + i, g);
            });
    }
#pragma unroll
    for (int k = 0; k < V; ++k) { p0[sub][lane * V + k] = a0[k]; p1[sub][lane * V + k] = a1[k]; }
    __syncthreads();
    if (sub == 0 && c < C) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int l = lane * V + k;
            scratch[(size_t)blockIdx.y * C + c + k] = p0[0][l] + p0[1][l] + p0[2][l] + p0[3][l];
            if (MODE == 2) scratch[(size_t)(slabs + blockIdx.y) * C + c + k] = p1[0][l] + p1[1][l] + p1[2][l] + p1[3][l];
        }
    }
}
// running statistics (momentum 0.1, unbiased variance), model.py:42 nn.BatchNorm1d defaults.  Every product is rounded on its
// own (what the compiler made of this line in bn_running_kernel, which multiplies in pairs): no fma, wherever it is inlined.
__device__ __forceinline__ void bn_running_update(float mean, float var, int M, float momentum, float* rm, float* rv) {
#pragma clang fp contract(off)
    const float unb = var * ((float)M / (float)(M > 1 ? M - 1 : 1));
    *rm = (1.0f - momentum) * *rm + momentum * mean;
    *rv = (1.0f - momentum) * *rv + momentum * unb;
}
// out0[c] = f(sum over slabs); MODE 0: mean = s/M ; MODE 1: invstd = rsqrt(s/M + eps), var_out = s/M ; MODE 2: raw sums
// MODE 1 with rm (the fused forward): also the running statistics, from mean[] and the variance just finished
__global__ void colreduce_stage2_kernel(const float* __restrict__ scratch, int C, int slabs, int M, int mode, float eps,
                                        float* out0, float* out1, const float* mean, float momentum, float* rm, float* rv) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    // the slab partials are requested 16 at a time and added in slab order (common.h)
    const float s0 = ordered_sum16(scratch + c, slabs, C);
    const float s1 = mode == 2 ? ordered_sum16(scratch + (size_t)slabs * C + c, slabs, C) : 0.f;
    if (mode == 0) out0[c] = s0 / (float)M;
    else if (mode == 1) {
        const float var = s0 / (float)M;
        out0[c] = 1.0f / sqrtf(var + eps);
        if (out1) out1[c] = var;
        if (rm) bn_running_update(mean[c], var, M, momentum, rm + c, rv + c);
    }
    else { out0[c] = s0; out1[c] = s1; }
}

// y = dropout(act((z-mean)*invstd*gamma + beta)) (+ residual)
// A lane handles V adjacent channels per step (V = 4: 16-byte accesses).  The channel of a lane's first element is
// divided out once and then stepped, so the loop holds no division.  As in the reductions, the fused products are
// written out: u = fma(xhat, gamma, beta); the two mean corrections of dz are one fma each.
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
// the bf16 copy of V adjacent values for the next GEMM (round to nearest even, as the staging cast of the fp32 array)
template <int V> __device__ __forceinline__ void store_cols16(__bf16* p, const ColVec<V>& r) {
    if constexpr (V == 4) { bf16x4 t; t[0] = (__bf16)r.v[0]; t[1] = (__bf16)r.v[1]; t[2] = (__bf16)r.v[2]; t[3] = (__bf16)r.v[3]; *reinterpret_cast<bf16x4*>(p) = t; }
    else if constexpr (V == 2) { bf16x2 t; t[0] = (__bf16)r.v[0]; t[1] = (__bf16)r.v[1]; *reinterpret_cast<bf16x2*>(p) = t; }
    else *p = (__bf16)r.v[0];
}
__device__ __forceinline__ float bn_apply_term(const BnElem& e, float scale, float z, float mean, float inv, float ga, float be, uint32_t i) {
#pragma clang fp contract(off)
    float v = act_fwd(fmaf((z - mean) * inv, ga, be), e.act);
    if (e.drop_p > 0.f) v = rng_keep(e.key, i, e.drop_p) ? v * scale : 0.f;
    return v;
}
template <int V>
__global__ void bn_apply_kernel(BnElem e, const float* __restrict__ residual, float* __restrict__ y, __bf16* __restrict__ y16, size_t n) {
    const float scale = e.drop_p > 0.f ? 1.0f / (1.0f - e.drop_p) : 1.0f;
    const size_t stride = (size_t)gridDim.x * blockDim.x * V;
    size_t i = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) * V;
    int c = (int)(i % e.C);
    const int cstep = (int)(stride % e.C);
    for (; i < n; i += stride) {
        const ColVec<V> z = load_cols<V>(e.z + i), mean = load_cols<V>(e.mean + c), inv = load_cols<V>(e.invstd + c),
                        ga = load_cols<V>(e.gamma + c), be = load_cols<V>(e.beta + c);
        ColVec<V> v;
#pragma unroll
        for (int k = 0; k < V; ++k) v.v[k] = bn_apply_term(e, scale, z.v[k], mean.v[k], inv.v[k], ga.v[k], be.v[k], (uint32_t)(i + k));
        if (residual) {
            const ColVec<V> r = load_cols<V>(residual + i);
#pragma unroll
            for (int k = 0; k < V; ++k) v.v[k] += r.v[k];
        }
        store_cols<V>(y + i, v);
        if (y16) store_cols16<V>(y16 + i, v);
        c += cstep;
        if (c >= e.C) c -= e.C;
    }
}
// training: dz = gamma*invstd*(du - sum_du/M - xhat*sum_duxh/M) ; eval: dz = du*gamma*invstd
__device__ __forceinline__ float bn_bwd_dz_term(float g, float z, float mean, float inv, float ga, float sdu, float sduxh, float invM, int training) {
#pragma clang fp contract(off)
    if (training) {
        const float xh = (z - mean) * inv;
        g = fmaf(-invM, sdu, g);
        g = fmaf(-invM, xh * sduxh, g);
    }
    return g * ga * inv;
}
template <int V>
__global__ void bn_bwd_dz_kernel(BnElem e, const float* du, const float* __restrict__ sdu, const float* __restrict__ sduxh,
                                 int M, int training, float* dz, __bf16* __restrict__ dz16, size_t n) {
    const float invM = 1.0f / (float)M;
    const size_t stride = (size_t)gridDim.x * blockDim.x * V;
    size_t i = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) * V;
    int c = (int)(i % e.C);
    const int cstep = (int)(stride % e.C);
    for (; i < n; i += stride) {
        const ColVec<V> g = load_cols<V>(du + i), inv = load_cols<V>(e.invstd + c), ga = load_cols<V>(e.gamma + c);
        ColVec<V> z{}, mean{}, s0{}, s1{};
        if (training) { z = load_cols<V>(e.z + i); mean = load_cols<V>(e.mean + c); s0 = load_cols<V>(sdu + c); s1 = load_cols<V>(sduxh + c); }
        ColVec<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = bn_bwd_dz_term(g.v[k], z.v[k], mean.v[k], inv.v[k], ga.v[k], s0.v[k], s1.v[k], invM, training);
        store_cols<V>(dz + i, o);
        if (dz16) store_cols16<V>(dz16 + i, o);
        c += cstep;
        if (c >= e.C) c -= e.C;
    }
}
// running statistics (bn_running_update above)
__global__ void bn_running_kernel(const float* mean, const float* var, int C, int M, float momentum, float* rm, float* rv) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    bn_running_update(mean[c], var[c], M, momentum, rm + c, rv + c);
}

// The dz kernel in the shape of the reductions (a workgroup is 4 row phases x kColLanes lanes, a lane owns V fixed columns),
// so a column's statistics are registers, and what the kernel before left as slab partials is finished in the prologue:
// thread j sums column j of the block in slab order into LDS, no launch of its own.
// It runs on the partition of the reduction that wrote `sums` (MODE 2: slabs x C partials of sum du, then of sum du*xhat).
// The prologue finishes both; the workgroups of slab 0 store d(beta) and d(gamma).  The rows of a slab are walked as
// colsum_stage1_kernel walks them (4 phases, rows ascending, the slab's sum p0 + p1 + p2 + p3), so the slab partials of
// d(bias) = sum dz fall out into dbias_part (nullable) and dz is not read again: colsum's stage 2 finishes them.
template <int V>
__global__ void __launch_bounds__(kColThreads) bn_bwd_dz_cols_kernel(BnElem e, const float* du, const float* __restrict__ sums, int M, int slabs,
                                                                     int training, float* dz, __bf16* __restrict__ dz16,
                                                                     float* __restrict__ dbeta, float* __restrict__ dgamma,
                                                                     float* __restrict__ dbias_part) {
    constexpr int R = V == 4 ? 8 : 16, NC = kColLanes * V;
    const int C = e.C;
    const int lane = threadIdx.x % kColLanes, sub = threadIdx.x / kColLanes;
    const int c = (blockIdx.x * kColLanes + lane) * V;
    const int rows = (M + slabs - 1) / slabs;
    const int m0 = blockIdx.y * rows, m1 = min(M, m0 + rows);
    __shared__ float fin[2][NC], part[4][NC];
    for (int j = threadIdx.x; j < 2 * NC; j += kColThreads) {
        const int w = j / NC, cc = blockIdx.x * NC + j % NC;
        fin[w][j % NC] = cc < C ? ordered_sum64(sums + (size_t)w * slabs * C + cc, slabs, C) : 0.f;
    }
    __syncthreads();
    float acc[V] = {};
    if (c < C) {
        BnCol col[V];
        float s0[V], s1[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            col[k].mean = e.mean[c + k]; col[k].inv = e.invstd[c + k]; col[k].ga = e.gamma[c + k]; col[k].be = 0.f;
            s0[k] = fin[0][lane * V + k]; s1[k] = fin[1][lane * V + k];
            if (blockIdx.y == 0 && sub == 0) { dbeta[c + k] = s0[k]; dgamma[c + k] = s1[k]; }
        }
        const float invM = 1.0f / (float)M;
        struct Row { ColVec<V> g, z; };
        rows_in_flight<R, Row>(m0 + sub, m1,
            [&](int m) {
                const size_t i = (size_t)m * C + c;
                Row r;
                r.g = load_cols<V>(du + i);
                if (training) r.z = load_cols<V>(e.z + i);
                return r;
            },
            [&](int m, const Row& r) {
                const size_t i = (size_t)m * C + c;
                ColVec<V> o;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    o.v[k] = bn_bwd_dz_term(r.g.v[k], training ? r.z.v[k] : 0.f, col[k].mean, col[k].inv, col[k].ga, s0[k], s1[k], invM, training);
                    acc[k] += o.v[k];
                }
                store_cols<V>(dz + i, o);
                if (dz16) store_cols16<V>(dz16 + i, o);
            });
    }
    if (!dbias_part) return;
#pragma unroll
    for (int k = 0; k < V; ++k) part[sub][lane * V + k] = acc[k];
    __syncthreads();
    if (sub == 0 && c < C) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int l = lane * V + k;
            dbias_part[(size_t)blockIdx.y * C + c + k] = part[0][l] + part[1][l] + part[2][l] + part[3][l];
        }
    }
}
__global__ void invstd_from_var_kernel(const float* var, int C, float eps, float* invstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) invstd[c] = 1.0f / sqrtf(var[c] + eps);
}

// out[row, :] = table[ids[row], :]
__global__ void embedding_fwd_kernel(const long* __restrict__ ids, const float* __restrict__ table, float* __restrict__ out, int rows, int D) {
    const size_t n = (size_t)rows * (D / 4);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / (D / 4)), q = (int)(i % (D / 4));
        reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(table + ids[r] * (long)D)[q];
    }
}
// dtable[v, :] = sum over rows with ids[row] == v of dout[row, :]   (one workgroup per vocabulary entry: fixed order)
// The ordered list of the rows that hit v is built in passes of kEmbRounds * kEmbThreads rows.  A thread requests all its
// ids of a pass at once (row = pass base + j * kEmbThreads + thread in round j) and keeps one hit bit per round, so a
// pass costs one load latency and one barrier, not one of each per round: the 6400 tokens of a training batch are one
// pass.  A round's hits are placed by a ballot inside the wave and the prefix over the (round, wave) counts in front of it,
// which every thread walks in LDS: ascending rows, whatever the scheduling.
constexpr int kEmbThreads = 256, kEmbWaves = kEmbThreads / 64, kEmbRounds = 32;
// V = 4: a thread sums 4 adjacent columns with 16-byte requests (D % 4 == 0, 16-byte aligned arrays).  The additions of
// a column are the same in the same order for either V: rows ascending, fp32, requested 8 at a time.
template <int V>
__global__ __launch_bounds__(kEmbThreads) void embedding_bwd_kernel(const long* __restrict__ ids, const float* __restrict__ dout,
                                                                    float* __restrict__ dtable, int rows, int D) {
    const int v = blockIdx.x;
    extern __shared__ int hits[];
    __shared__ __attribute__((aligned(16))) int wave_cnt[2][kEmbRounds][kEmbWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    int run = 0;
    for (int r0 = 0, it = 0; r0 < rows; r0 += kEmbRounds * kEmbThreads, ++it) {
        long id[kEmbRounds];
#pragma unroll
        for (int j = 0; j < kEmbRounds; ++j) {
            const int r = r0 + j * kEmbThreads + tid;
            id[j] = r < rows ? ids[r] : -1;
        }
        unsigned mine = 0;
#pragma unroll
        for (int j = 0; j < kEmbRounds; ++j) mine |= (id[j] == v ? 1u : 0u) << j;
        int (*wc)[kEmbWaves] = wave_cnt[it & 1];           // (two buffers: the next pass writes while a slow wave still reads)
#pragma unroll
        for (int j = 0; j < kEmbRounds; ++j) {
            const unsigned long long m = __ballot((mine >> j) & 1u);
            if (lane == 0) wc[j][wave] = __popcll(m);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kEmbRounds; ++j) {
            int base = run, tot = 0;
#pragma unroll
            for (int w = 0; w < kEmbWaves; ++w) { const int cw = wc[j][w]; if (w < wave) base += cw; tot += cw; }
            const bool hit = (mine >> j) & 1u;
            const unsigned long long m = __ballot(hit);
            if (hit) hits[base + __popcll(m & below)] = r0 + j * kEmbThreads + tid;
            run += tot;
        }
    }
    __syncthreads();
    const int nhit = run;
    typedef float vec __attribute__((ext_vector_type(V)));
    for (int c = tid * V; c < D; c += kEmbThreads * V) {
        vec acc = 0.f;                                     // rows requested 8 at a time, added in row order
        int h = 0;
        for (; h + 8 <= nhit; h += 8) {
            vec x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const vec*>(dout + (size_t)hits[h + j] * D + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += x[j];
        }
        for (; h < nhit; ++h) acc += *reinterpret_cast<const vec*>(dout + (size_t)hits[h] * D + c);
        *reinterpret_cast<vec*>(dtable + (size_t)v * D + c) = acc;
    }
}

// 16-byte accesses need C % 4 == 0 and every array on a 16-byte boundary (p, q: the kernel's other arrays, may be null)
bool bn_vectorisable(const BnElem& e, const void* p, const void* q) {
    for (const void* a : {(const void*)e.z, (const void*)e.mean, (const void*)e.invstd, (const void*)e.gamma, (const void*)e.beta, p, q})
        if (!cols_vectorisable(a, e.C, e.C)) return false;
    return true;
}
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }
inline bool same_route(const GemmPlan& p, const GemmPlan& q) { return p.kernel == q.kernel && p.split == q.split && p.splitk == q.splitk && p.kchunks == q.kchunks; }

std::atomic<int> g_bn_fuse{env_int("T2_BN_FUSE", 1)};
std::atomic<uint64_t> g_bn_counts[3];

inline int col_blocks(int C, int V) { return (C + V * kColLanes - 1) / (V * kColLanes); }
// Columns per lane on the reduction partition.  16-byte groups where the arrays allow them, as ever.  narrow = the fused
// backward: the order of additions leaves C/V * 4 * slabs lanes, 512 waves for 512 columns at V = 4, and the MODE 2 pass
// (tanh, the dropout hash, two arrays in, one out) gains from every halving (profiles/r16_conv_widths.txt: 89 / 61 / 43 us
// at 25600 x 512), so with (nearly) all 64 slabs it takes the widest lane that gives each of the 1024 SIMDs two waves, else
// one column per lane.  The forward passes (one array in, an add or an fma per element) do not move with V and keep 4.
int col_width(int C, int slabs, bool vec, bool narrow) {
    if (!vec) return 1;
    if (narrow && slabs >= 48) {
        for (int v = 4; v > 1; v >>= 1)
            if (col_blocks(C, v) * slabs * (kColThreads / kWave) >= 2048) return v;
        return 1;
    }
    return 4;
}

template <int MODE, bool FIN>
int colreduce_stage1(const BnElem& e, const float* dy, float* du, int M, float* scratch, float* mean_out, int V, hipStream_t s) {
    const int slabs = col_slabs(M);
    const dim3 grid(col_blocks(e.C, V), slabs), block(kColThreads);
    if (V == 4) hipLaunchKernelGGL((colreduce_stage1_kernel<MODE, 4, FIN>), grid, block, 0, s, e, dy, du, M, slabs, scratch, mean_out);
    else if constexpr (MODE == 2) {
        if (V == 2) hipLaunchKernelGGL((colreduce_stage1_kernel<2, 2, false>), grid, block, 0, s, e, dy, du, M, slabs, scratch, mean_out);
        else hipLaunchKernelGGL((colreduce_stage1_kernel<2, 1, false>), grid, block, 0, s, e, dy, du, M, slabs, scratch, mean_out);
    } else hipLaunchKernelGGL((colreduce_stage1_kernel<MODE, 1, FIN>), grid, block, 0, s, e, dy, du, M, slabs, scratch, mean_out);
    T2_LAUNCH_CHECK();
    return 0;
}
template <int MODE>
int colreduce(const BnElem& e, const float* dy, float* du, int M, float eps, float* out0, float* out1, float* scratch, hipStream_t s) {
    const int slabs = col_slabs(M);
    const bool vec = cols_vectorisable(e.z, e.C, e.C) && cols_vectorisable(dy, e.C, e.C) && cols_vectorisable(du, e.C, e.C);
    T2_TRY_RC((colreduce_stage1<MODE, false>(e, dy, du, M, scratch, nullptr, col_width(e.C, slabs, vec, false), s)));
    hipLaunchKernelGGL(colreduce_stage2_kernel, dim3((e.C + 255) / 256), dim3(256), 0, s, scratch, e.C, slabs, M, MODE, eps, out0, out1,
                       (const float*)nullptr, 0.f, (float*)nullptr, (float*)nullptr);
    T2_LAUNCH_CHECK();
    return 0;
}

}  // namespace

void set_bn_fuse(int on) { g_bn_fuse = on != 0; }
int get_bn_fuse() { return g_bn_fuse; }
void bn_fuse_counts(uint64_t* out, int reset) {
    for (int i = 0; i < 3; ++i) { out[i] = g_bn_counts[i]; if (reset) g_bn_counts[i] = 0; }
}

int conv_bn_fwd(const ConvBnFwd& a, hipStream_t s) {
    const int M = a.B * a.T;
    T2_REQUIRE(a.Cin % 4 == 0 && a.K % 2 == 1, "conv_bn_fwd: Cin=%d must be a multiple of 4 and the kernel size odd (%d)", a.Cin, a.K);
    T2_REQUIRE((size_t)M * a.Cout < (1ull << 32), "conv_bn_fwd: B*T*Cout too large for 32-bit RNG indices");
    const size_t nw = (size_t)a.Cout * a.Cin * a.K;
    GemmDesc g = gemm_desc();
    g.A = a.x; g.conv_a = 1; g.conv_T = a.T; g.conv_C = a.Cin; g.conv_pad = (a.K - 1) / 2;
    g.B = a.wperm; g.sbn = (long)a.K * a.Cin; g.sbk = 1;
    g.C = a.z; g.ldc = a.Cout; g.M = M; g.N = a.Cout; g.K = a.K * a.Cin; g.bias1 = a.bias;
    g.ws = a.gemm_ws; g.ws_bytes = a.gemm_ws_bytes;
    // bf16 hand-offs (a.handoff: a stack in bf16 mode): the frames an earlier layer wrote next to its y (x16, if any),
    // and the weights re-laid-out straight into bf16 — if gemm_handoff says the product is the same with them
    GemmDesc g16 = g;
    g16.A16 = a.x16; g16.lda16 = a.Cin;
    g16.B16 = reinterpret_cast<const __bf16*>(a.wperm); g16.ldb16 = (long)a.K * a.Cin;
    if (a.handoff && gemm_handoff(g, g16)) {
        g = g16;
        permute_w(false, a.w, reinterpret_cast<__bf16*>(a.wperm), a.Cout, a.Cin, a.K, s);
    } else
        permute_w(false, a.w, a.wperm, a.Cout, a.Cin, a.K, s);
    T2_LAUNCH_CHECK();
    T2_TRY_RC(gemm(g, s));
    BnElem e{a.z, a.mean, a.invstd, a.gamma, a.beta, a.Cout, a.act, a.drop_p, rng_key(a.seed, a.site)};
    const size_t n = (size_t)M * a.Cout;
    if (a.training && get_bn_fuse()) {
        // four launches for six: the MODE 1 pass finishes the mean from the MODE 0 partials (first half of the scratch) and
        // leaves its own behind them; one stage 2 finishes var / invstd from those and updates the running statistics
        const int slabs = col_slabs(M);
        const int V = col_width(e.C, slabs, cols_vectorisable(e.z, e.C, e.C), false);
        T2_TRY_RC((colreduce_stage1<0, false>(e, nullptr, nullptr, M, a.scratch, nullptr, V, s)));
        T2_TRY_RC((colreduce_stage1<1, true>(e, nullptr, nullptr, M, a.scratch, a.mean, V, s)));
        hipLaunchKernelGGL(colreduce_stage2_kernel, dim3((a.Cout + 255) / 256), dim3(256), 0, s, a.scratch + (size_t)slabs * e.C, a.Cout, slabs, M, 1,
                           a.eps, a.invstd, a.var, a.mean, 0.1f, a.run_mean, a.run_var);
        T2_LAUNCH_CHECK();
        ++g_bn_counts[0];
    } else if (a.training) {
        T2_TRY_RC(colreduce<0>(e, nullptr, nullptr, M, a.eps, a.mean, nullptr, a.scratch, s));
        T2_TRY_RC(colreduce<1>(e, nullptr, nullptr, M, a.eps, a.invstd, a.var, a.scratch, s));
        if (a.run_mean) {
            hipLaunchKernelGGL(bn_running_kernel, dim3((a.Cout + 255) / 256), dim3(256), 0, s, a.mean, a.var, a.Cout, M, 0.1f, a.run_mean, a.run_var);
            T2_LAUNCH_CHECK();
        }
    } else {
        T2_CHECK_HIP(hipMemcpyAsync(a.mean, a.run_mean, sizeof(float) * a.Cout, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(invstd_from_var_kernel, dim3((a.Cout + 255) / 256), dim3(256), 0, s, a.run_var, a.Cout, a.eps, a.invstd);
        T2_LAUNCH_CHECK();
    }
    if (bn_vectorisable(e, a.residual, a.y) && aligned8(a.y16))
        hipLaunchKernelGGL(bn_apply_kernel<4>, dim3(grid_for(n / 4)), dim3(256), 0, s, e, a.residual, a.y, a.y16, n);
    else
        hipLaunchKernelGGL(bn_apply_kernel<1>, dim3(grid_for(n)), dim3(256), 0, s, e, a.residual, a.y, a.y16, n);
    T2_LAUNCH_CHECK();
    return 0;
}

int conv_bn_bwd(const ConvBnBwd& a, hipStream_t s) {
    const int M = a.B * a.T;
    const size_t n = (size_t)M * a.Cout;
    BnElem e{a.z, a.mean, a.invstd, a.gamma, a.beta, a.Cout, a.act, a.drop_p, rng_key(a.seed, a.site)};
    // d(weight)[co][dk*Ci+ci] = sum_m dz[m,co] * V[m, dk*Ci+ci]   (implicit im2col on the B side)
    GemmDesc g = gemm_desc();
    g.A = a.dz; g.sam = 1; g.sak = a.Cout;
    g.B = a.x; g.conv_b = 1; g.conv_T = a.T; g.conv_C = a.Cin; g.conv_pad = (a.K - 1) / 2;
    g.C = a.wperm; g.ldc = (long)a.K * a.Cin; g.M = a.Cout; g.N = a.K * a.Cin; g.K = M;
    g.ws = a.gemm_ws; g.ws_bytes = a.gemm_ws_bytes;
    // the product (or its split-K reduce) writes column dk*Ci + ci at ci*K + dk: the reference layout [Cout][Cin][K], straight
    // into a.dw (set_gemm_fold(0): into wperm, and unpermute_dw_kernel copies it over)
    const bool fold = get_gemm_fold() != 0;
    if (fold) { g.C = a.dw; g.ccol_mod = a.Cin; g.ccol_mul = a.K; }
    // d(input) = correlation of dz with the flipped, transposed kernel
    GemmDesc h = gemm_desc();
    h.A = a.dz; h.conv_a = 1; h.conv_T = a.T; h.conv_C = a.Cout; h.conv_pad = (a.K - 1) / 2;
    h.B = a.wperm; h.sbn = (long)a.K * a.Cout; h.sbk = 1;
    h.C = a.dx; h.ldc = a.Cin; h.M = M; h.N = a.Cin; h.K = a.K * a.Cout;
    h.beta = a.dx_accumulate ? 1.f : 0.f;
    h.ws = a.gemm_ws; h.ws_bytes = a.gemm_ws_bytes;
    if (a.dx) T2_REQUIRE(a.Cout % 4 == 0, "conv_bn_bwd: Cout=%d must be a multiple of 4", a.Cout);
    // bf16 hand-offs (a.handoff: a stack in bf16 mode).  dz16, the bf16 copy of dz, is written once by bn_bwd_dz_kernel
    // at the head of the GEMM scratch — where d(weight) would stage its A operand and d(input) its frames, the same
    // bytes — and serves both products; the saved x16 is d(weight)'s frames, the flipped weights go straight to bf16.
    // Each product takes its copies only if gemm_handoff allows it, and d(weight), if it runs without them while dz16
    // is alive, must plan the same on the scratch behind it (d(input) runs after dz16's last reader).
    __bf16* dz16 = nullptr;
    bool w16 = false;
    const size_t dz16_bytes = round256(n * sizeof(__bf16));
    if (a.handoff && a.gemm_ws && (reinterpret_cast<uintptr_t>(a.gemm_ws) & 15) == 0 && a.gemm_ws_bytes >= dz16_bytes) {
        float* behind = a.gemm_ws + dz16_bytes / sizeof(float);
        GemmDesc g16 = g, h16 = h;
        g16.ws = h16.ws = behind; g16.ws_bytes = h16.ws_bytes = a.gemm_ws_bytes - dz16_bytes;
        g16.A16 = h16.A16 = reinterpret_cast<const __bf16*>(a.gemm_ws);
        g16.lda16 = a.Cout; g16.a16_kmajor = 1; h16.lda16 = a.Cout;
        g16.B16 = a.x16; g16.ldb16 = a.Cin; g16.b16_kmajor = 1;
        h16.B16 = reinterpret_cast<const __bf16*>(a.wperm); h16.ldb16 = (long)a.K * a.Cout;
        const bool tw = gemm_handoff(g, g16);
        bool tx = a.dx && gemm_handoff(h, h16);
        if (tx && !tw) {                                   // d(weight) runs on fp32 operands next to a live dz16
            GemmDesc gb = g;
            gb.ws = behind; gb.ws_bytes = g16.ws_bytes;
            if (same_route(plan_gemm(g), plan_gemm(gb))) g = gb; else tx = false;
        }
        if (tw) g = g16;
        if (tx) { h = h16; w16 = true; }
        if (tw || tx) dz16 = reinterpret_cast<__bf16*>(a.gemm_ws);
    }
    // du (into a.dz) + the two column sums; d(gamma) = sum du*xhat, d(beta) = sum du
    const size_t nw = (size_t)a.Cout * a.Cin * a.K;
    if (get_bn_fuse()) {
        // three launches: the dz kernel finishes the two sums in its prologue and leaves the slab partials of d(bias) in wperm,
        // which nobody uses before the products (64*Cout floats: it has them when Cin*K >= 64; a smaller layer runs colsum)
        const int slabs = col_slabs(M);
        const bool vec = cols_vectorisable(e.z, e.C, e.C) && cols_vectorisable(a.dy, e.C, e.C) && cols_vectorisable(a.dz, e.C, e.C);
        const int V = col_width(e.C, slabs, vec, true);
        T2_TRY_RC((colreduce_stage1<2, false>(e, a.dy, a.dz, M, a.scratch, nullptr, V, s)));
        float* part = (size_t)a.Cin * a.K >= 64 ? a.wperm : nullptr;
        const dim3 grid(col_blocks(e.C, V), slabs), block(kColThreads);
        if (V == 4) hipLaunchKernelGGL(bn_bwd_dz_cols_kernel<4>, grid, block, 0, s, e, a.dz, a.scratch, M, slabs, a.training, a.dz, dz16, a.dbeta, a.dgamma, part);
        else if (V == 2) hipLaunchKernelGGL(bn_bwd_dz_cols_kernel<2>, grid, block, 0, s, e, a.dz, a.scratch, M, slabs, a.training, a.dz, dz16, a.dbeta, a.dgamma, part);
        else hipLaunchKernelGGL(bn_bwd_dz_cols_kernel<1>, grid, block, 0, s, e, a.dz, a.scratch, M, slabs, a.training, a.dz, dz16, a.dbeta, a.dgamma, part);
        T2_LAUNCH_CHECK();
        if (part) T2_TRY_RC(colsum_finish(part, M, a.Cout, a.dbias, s));
        else T2_TRY_RC(colsum(a.dz, a.Cout, M, a.Cout, a.dbias, nullptr, a.scratch, s));
        ++g_bn_counts[part ? 1 : 2];
    } else {
        T2_TRY_RC(colreduce<2>(e, a.dy, a.dz, M, a.eps, a.dbeta, a.dgamma, a.scratch, s));
        if (bn_vectorisable(e, a.dz, a.dbeta) && cols_vectorisable(a.dgamma, e.C, e.C))
            hipLaunchKernelGGL(bn_bwd_dz_kernel<4>, dim3(grid_for(n / 4)), dim3(256), 0, s, e, a.dz, a.dbeta, a.dgamma, M, a.training, a.dz, dz16, n);
        else
            hipLaunchKernelGGL(bn_bwd_dz_kernel<1>, dim3(grid_for(n)), dim3(256), 0, s, e, a.dz, a.dbeta, a.dgamma, M, a.training, a.dz, dz16, n);
        T2_LAUNCH_CHECK();
        T2_TRY_RC(colsum(a.dz, a.Cout, M, a.Cout, a.dbias, nullptr, a.scratch, s));
    }
    T2_TRY_RC(gemm(g, s));
    if (!fold) {
        hipLaunchKernelGGL(unpermute_dw_kernel, dim3(grid_for(nw)), dim3(256), 0, s, a.wperm, a.dw, a.Cout, a.Cin, a.K);
        T2_LAUNCH_CHECK();
    }
    if (a.dx) {
        if (w16) permute_w(true, a.w, reinterpret_cast<__bf16*>(a.wperm), a.Cout, a.Cin, a.K, s);
        else permute_w(true, a.w, a.wperm, a.Cout, a.Cin, a.K, s);
        T2_LAUNCH_CHECK();
        T2_TRY_RC(gemm(h, s));
    }
    return 0;
}

int embedding_fwd(const long* ids, const float* table, float* out, int rows, int D, hipStream_t s) {
    T2_REQUIRE(D % 4 == 0, "embedding: dim %d must be a multiple of 4", D);
    hipLaunchKernelGGL(embedding_fwd_kernel, dim3(grid_for((size_t)rows * (D / 4))), dim3(256), 0, s, ids, table, out, rows, D);
    T2_LAUNCH_CHECK();
    return 0;
}
int embedding_bwd(const long* ids, const float* dout, float* dtable, int rows, int D, int vocab, hipStream_t s) {
    const size_t smem = (size_t)rows * sizeof(int);
    T2_REQUIRE(smem <= 150 * 1024, "embedding_bwd: %d tokens do not fit the LDS hit list", rows);
    const bool vec = cols_vectorisable(dout, D, D) && cols_vectorisable(dtable, D, D);
    const void* fn = vec ? reinterpret_cast<const void*>(embedding_bwd_kernel<4>) : reinterpret_cast<const void*>(embedding_bwd_kernel<1>);
    T2_TRY_RC(t2_allow_dynamic_lds(fn, smem));
    if (vec) hipLaunchKernelGGL(embedding_bwd_kernel<4>, dim3(vocab), dim3(kEmbThreads), smem, s, ids, dout, dtable, rows, D);
    else hipLaunchKernelGGL(embedding_bwd_kernel<1>, dim3(vocab), dim3(kEmbThreads), smem, s, ids, dout, dtable, rows, D);
    T2_LAUNCH_CHECK();
    return 0;
}

}  // namespace t2
