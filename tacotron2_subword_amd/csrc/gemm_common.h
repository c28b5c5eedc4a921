// What the GEMM kernel families share (gemm_f32.hip, gemm_bf16conv.hip, gemm.hip) and what gemm_dispatch.hip launches:
// the kernel-side descriptor, the element epilogue, the two store paths (direct from the accumulator fragments, and a
// row walk through LDS), the LDS swizzle of the bf16 tiles, the XCD tile remap and each family's launcher.
#pragma once
#include "kernels.h"
#include <type_traits>

namespace t2 {
namespace gemm_detail {

constexpr int BK = 16;                     // the unit of GemmK::kchunks (and the exact kernel's K-chunk)
constexpr int BK16 = 64, PK16 = BK16;      // K-step of the bf16 kernels and the pitch of their LDS rows
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct GemmK {
    GemmDesc d;
    int kchunks;    // K-chunks (of BK) per split
    int avec, bvec;  // 16-byte loads legal for A / B
    int xcd_swizzle; // bf16-source kernels: XCD-aware tile order (tile count a multiple of 8)
};

__host__ __device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The launchers of the kernel families (grid: tiles of the family's size x batch * splitk; block size and LDS are theirs).
int launch_gemm_f32(const GemmK& g, GemmKernel kernel, dim3 grid, hipStream_t s);                      // gemm_f32.hip: f32_64 / f32_128
int launch_gemm_bf16conv(const GemmK& g, dim3 grid, hipStream_t s);                                    // gemm_bf16conv.hip
int launch_gemm_bf16src(const GemmK& g, GemmKernel kernel, const __bf16* pa, long lda, const __bf16* pb, long ldb, dim3 grid, hipStream_t s);   // gemm.hip: src128 / src256 / src256km

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    if (act == ACT_TANH) return tanhf(v);
    if (act == ACT_GELU) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    return v;
}

// v + a * b as the K = 1, beta = 1 product it replaces leaves it: the product rounded on its own (the fp32 MFMA adds it
// to a zero accumulator, so a zero product is +0), then one rounded sum.  Nothing here may be contracted into an fma, which
// would round once.  Written with the operators under the pragma, not with __fmul_rn / __fadd_rn: the headers define those
// as the same operators compiled with contraction allowed (unless the rounded OCML operations are switched on), so after
// inlining they promise nothing.
__device__ __forceinline__ float add_rank1(float v, float a, float b) {
#pragma clang fp contract(off)
    const float p = a * b + 0.0f;
    return p + v;
}
// The column map costs an integer division per element, and left as a select on d.ccol_mod the compiler computes it for
// every element of every product (the 25600 x 2048 x 80 product: 152 -> 211 us).  So the kernels branch once, outside their
// store loops, into a copy of the loop compiled with the map (CMAP) or without it: with_col_map.
template <bool CMAP>
__device__ __forceinline__ long out_col(const GemmDesc& d, int n) {
    if constexpr (CMAP) return (long)(n % d.ccol_mod) * d.ccol_mul + n / d.ccol_mod;
    else return (long)n;
}
template <class F>
__device__ __forceinline__ void with_col_map(const GemmDesc& d, F f) {
    if (d.ccol_mod) f(std::true_type{}); else f(std::false_type{});
}
// the row map (GemmDesc::crow_mod)
__device__ __forceinline__ long out_row(const GemmDesc& d, int m) {
    return d.crow_mod ? (long)(m % d.crow_mod) * d.crow_mul + m / d.crow_mod : (long)m;
}

// the finished element (m, n) short of the beta term
__device__ __forceinline__ float epilogue_value(const GemmDesc& d, int m, int n, float acc, RngKey key) {
    float v = d.alpha * acc;
    if (d.bias1) v += d.bias1[n];
    if (d.bias2) v += d.bias2[n];
    v = apply_act(v, d.act);
    if (d.drop_p > 0.f) {
        uint32_t idx = d.drop_base + (uint32_t)m * d.drop_mstride + (uint32_t)n;
        v = rng_keep(key, idx, d.drop_p) ? v * (1.0f / (1.0f - d.drop_p)) : 0.f;
    }
    if (d.r1_m) v = add_rank1(v, d.r1_m[m], d.r1_n[n]);
    return v;
}
template <bool CMAP>
__device__ __forceinline__ void epilogue_store(const GemmDesc& d, float* C, int m, int n, float acc, RngKey key) {
    float v = epilogue_value(d, m, n, acc, key);
    float* p = C + out_row(d, m) * d.ldc + out_col<CMAP>(d, n);
    if (d.beta != 0.f) v += d.beta * (*p);
    *p = v;
}

// Implicit im2col for a k-tap 1-D convolution over channels-last frames X[B*T, C]: the operand is
// the virtual matrix V[m, dk*C + ci] = X[m + dk - pad, ci] if the shifted frame stays inside the
// same utterance (0 <= m%T + dk - pad < T), else 0.  T == 0: ordinary strided operand.
struct ConvAddr { int T, C, pad; };

// 16-byte slot s (8 bf16) of row R lives at slot s ^ ((R ^ (R >> 2)) & 7): with unpadded 128-byte rows this
// makes the K-contiguous stores, the row-contiguous (transposing) stores and the ds_read_b128 fragment
// reads all bank-conflict-free (checked exhaustively over the lane groups of MI355X_MICROARCH.md §LDS).
__device__ __forceinline__ int swz16(int row, int slot) { return row * PK16 + ((slot ^ ((row ^ (row >> 2)) & 7)) << 3); }

__device__ __forceinline__ bf16x8 pack8(const f32x4& lo, const f32x4& hi) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = (__bf16)lo[j]; v[4 + j] = (__bf16)hi[j]; }
    return v;
}

template <int TM, int TN>
__device__ __forceinline__ void zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}

// Tile of a workgroup of the bf16-source kernels.  Workgroups are dealt round-robin over the 8 XCDs (linear id % 8) and
// every XCD has its own 4 MB L2: with the plain (x, y) -> (n, m) map each XCD sees every A row panel and one eighth of the
// B panels and re-fetches operands 5-6x (profiles/r01_pmc_gemm_traffic.json).  Remap so that an XCD works through a
// CONTIGUOUS run of tiles, ordered in groups of gm tile rows (a group's tiles share gm A panels and walk the B panels once).
__device__ __forceinline__ void xcd_remap(int gm, int& bx, int& by) {
    const int gx = gridDim.x, gy = gridDim.y, total = gx * gy;
    const int lin = by * gx + bx;
    const int pid = (lin & 7) * (total >> 3) + (lin >> 3);
    const int per_group = gm * gx, group = pid / per_group, first_m = group * gm;
    const int gsz = min(gy - first_m, gm);
    by = first_m + (pid % per_group) % gsz;
    bx = (pid % per_group) / gsz;
}

// Direct stores of a wave's TM x TN accumulator fragments (32 x 32 each) whose first element is (m0, n0): lane (r, hk) holds
// column r, rows (e & 3) + 8 * (e >> 2) + 4 * hk of each fragment.  ws: this split's partial plane (plain stores) or null
// (finished elements into C).  PARTIAL: the tile may reach past M or N.
template <bool PARTIAL, int TM, int TN>
__device__ __forceinline__ void store_direct(const GemmDesc& d, float* C, float* ws, const f32x16 (&acc)[TM][TN], int m0, int n0, int r, int hk) {
    const RngKey key = rng_key(d.seed, d.site);
    with_col_map(d, [&](auto cmap) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + j * 32 + r;
                if (PARTIAL && n >= d.N) continue;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = m0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hk;
                    if (PARTIAL && m >= d.M) continue;
                    if (ws) ws[(long)m * d.N + n] = acc[i][j][e];
                    else epilogue_store<decltype(cmap)::value>(d, C, m, n, acc[i][j][e], key);
                }
            }
    });
}

// Stores of a wave's 64 x 64 sub-tile (2 x 2 fragments, acc[0..1][0..1]) through LDS: the wave lays the sub-tile out
// row-major in its own 16 KB (stg) and walks it 4 rows per iteration with 16-byte reads, so a row leaves as 256 contiguous
// bytes in 16-byte stores (16 store instructions per lane instead of 64) and the row map is resolved once per 4 elements.
// m0: first row of the sub-tile; n: the first of the lane's 4 columns, i.e. the column of element 4 * (lane & 15) of an LDS
// row (the kernel's: a kernel may interleave its columns); elem(m, n, c, x): the finished element (m, n + c) short of the
// beta term.  Lanes whose 4 columns are not all inside N, a column map and unaligned outputs take scalar stores.  The LDS
// must be free on entry (a barrier behind its last reader).  The converting kernel stores through it; the 256-tile kernel
// has the same walk written out for whole tiles (gemm.hip says why).
template <bool PARTIAL, class Elem>
__device__ __forceinline__ void store_rows_lds(const GemmDesc& d, float* C, float* ws, float* stg, const f32x16 (*acc)[2], int m0, int n, Elem elem) {
    const int lane = threadIdx.x & 63, r = lane & 31, hk = lane >> 5, c4 = (lane & 15) * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) stg[(i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hk) * 64 + j * 32 + r] = acc[i][j][e];
    __syncthreads();
    const bool vec = (!PARTIAL || n + 3 < d.N) && (ws ? !PARTIAL || (aligned16(ws) && d.N % 4 == 0) : aligned16(C) && d.ldc % 4 == 0 && !d.ccol_mod);
    if (PARTIAL && n >= d.N) return;
    for (int it = 0; it < 16; ++it) {
        const int row = it * 4 + (lane >> 4);
        const int m = m0 + row;
        if (PARTIAL && m >= d.M) continue;
        f32x4 v = *reinterpret_cast<const f32x4*>(stg + row * 64 + c4);
        if (ws) {
            float* pw = ws + (long)m * d.N + n;
            if (!PARTIAL || vec) *reinterpret_cast<f32x4*>(pw) = v;
            else
#pragma unroll
                for (int c = 0; c < 4; ++c) if (n + c < d.N) pw[c] = v[c];
            continue;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) if (!PARTIAL || n + c < d.N) v[c] = elem(m, n, c, v[c]);
        float* pr = C + out_row(d, m) * d.ldc;
        if (vec) {
            float* pc = pr + n;
            if (d.beta != 0.f) v += d.beta * *reinterpret_cast<const f32x4*>(pc);
            *reinterpret_cast<f32x4*>(pc) = v;
        } else {
            with_col_map(d, [&](auto cmap) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (PARTIAL && n + c >= d.N) continue;
                    float* pc = pr + out_col<decltype(cmap)::value>(d, n + c);
                    *pc = d.beta != 0.f ? v[c] + d.beta * *pc : v[c];
                }
            });
        }
    }
}

}  // namespace gemm_detail
}  // namespace t2
