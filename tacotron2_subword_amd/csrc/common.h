// Shared device helpers for the gfx950 (MI355X / CDNA4) Tacotron2 kernels.
// Wave = 64 lanes everywhere; no other target is supported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace t2 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWave = 64;

// ---------------------------------------------------------------------------------------------
// Counter-based RNG (dropout keep-masks, SMA pre-sigmoid noise).  A value depends only on
// (seed, site, index) so the backward pass regenerates a mask instead of storing it, and the
// parity tests can export exactly the bits the kernels use (t2_rng_keep_mask / t2_rng_normal).
// ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
struct RngKey { uint32_t k0, k1; };
__host__ __device__ __forceinline__ RngKey rng_key(uint64_t seed, uint32_t site) {
    RngKey k;
    k.k0 = mix32((uint32_t)seed ^ mix32(site * 0x9E3779B9u + 0x85ebca6bu));
    k.k1 = mix32((uint32_t)(seed >> 32) + site * 0xc2b2ae35u + 0x27d4eb2fu);
    return k;
}
__host__ __device__ __forceinline__ uint32_t rng_u32(RngKey k, uint32_t idx) {
    return mix32((idx ^ k.k0) * 0x9E3779B1u + k.k1);
}
// uniform in [0,1) with 24 bits
__host__ __device__ __forceinline__ float rng_uniform(RngKey k, uint32_t idx) {
    return (float)(rng_u32(k, idx) >> 8) * (1.0f / 16777216.0f);
}
__host__ __device__ __forceinline__ bool rng_keep(RngKey k, uint32_t idx, float p) {
    return rng_uniform(k, idx) >= p;
}
// standard normal via Box-Muller on two decorrelated draws of the same index
__device__ __forceinline__ float rng_normal(RngKey k, uint32_t idx) {
    uint32_t a = rng_u32(k, idx);
    uint32_t b = mix32(a ^ 0x68bc21ebu) + k.k0;
    float u1 = ((float)(a >> 8) + 1.0f) * (1.0f / 16777216.0f);   // (0,1]
    float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// ---------------------------------------------------------------------------------------------
// activations (accurate forms: the 1e-4 parity contract is on 400 recurrent steps)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---------------------------------------------------------------------------------------------
// Stage 1 of the fixed-order column reductions (colsum, the BatchNorm statistics).  The sum of a
// column over a slab of rows is defined as ((p0 + p1) + p2) + p3, where phase p adds rows
// m0+p, m0+p+4, ... one after the other.  That order fixes the bits; how many loads are in flight
// does not, so a lane owns V adjacent columns (one 16-byte load per row for V = 4), requests R rows
// before it consumes the first, and has the next R on their way while it consumes.
// A workgroup is 4 phases x kColLanes lanes and covers kColLanes*V columns of one slab.
// The order leaves C/V * 4 * slabs lanes to work with: 512 waves for 512 columns at V = 4, half the
// SIMDs of the device, so a caller picks a smaller V (and a larger R) where that fills it.
// ---------------------------------------------------------------------------------------------
constexpr int kColLanes = 32;
constexpr int kColThreads = 4 * kColLanes;

template <int V> struct ColVec { float v[V]; };
template <int V> __device__ __forceinline__ ColVec<V> load_cols(const float* p) {
    static_assert(V == 1 || V == 2 || V == 4, "one column, or one 8- or 16-byte group per lane");
    ColVec<V> r;
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else if constexpr (V == 2) {
        const f32x2 t = *reinterpret_cast<const f32x2*>(p);
        r.v[0] = t.x; r.v[1] = t.y;
    } else r.v[0] = *p;
    return r;
}
template <int V> __device__ __forceinline__ void store_cols(float* p, const ColVec<V>& r) {
    if constexpr (V == 4) { f32x4 t; t.x = r.v[0]; t.y = r.v[1]; t.z = r.v[2]; t.w = r.v[3]; *reinterpret_cast<f32x4*>(p) = t; }
    else if constexpr (V == 2) { f32x2 t; t.x = r.v[0]; t.y = r.v[1]; *reinterpret_cast<f32x2*>(p) = t; }
    else *p = r.v[0];
}
// use(m, load(m)) for m = m, m+4, ... < m1, in that order.  The tail requests a full group too (rows past the end
// repeat the last valid one and are not used), so no load sits behind a branch of its own.
template <int R, class Row, class Load, class Use>
__device__ __forceinline__ void rows_in_flight(int m, const int m1, Load load, Use use) {
    int left = m < m1 ? (m1 - m + 3) / 4 : 0;
    Row a[R], b[R];                                        // two groups by name: a copy between them would wait for the loads
    auto request = [&](Row (&x)[R], int mm) {
#pragma unroll
        for (int j = 0; j < R; ++j) x[j] = load(mm + 4 * j);
    };
    auto consume = [&](const Row (&x)[R]) {
#pragma unroll
        for (int j = 0; j < R; ++j) use(m + 4 * j, x[j]);
        m += 4 * R;
        left -= R;
    };
    if (left >= R) request(a, m);
    while (left >= R) {
        if (left >= 2 * R) request(b, m + 4 * R);
        consume(a);
        if (left < R) break;
        if (left >= 2 * R) request(a, m + 4 * R);
        consume(b);
    }
    if (left > 0) {
#pragma unroll
        for (int j = 0; j < R; ++j) a[j] = load(m + 4 * (j < left ? j : left - 1));
#pragma unroll
        for (int j = 0; j < R; ++j) if (j < left) use(m + 4 * j, a[j]);
    }
}
// the partition both stages agree on
__host__ __device__ inline int col_slabs(int M) { return M >= 64 * 64 ? 64 : (M >= 64 ? M / 64 : 1); }
// Stage 2: sum_{s < count} p[s * stride], terms requested 16 at a time and added in index order (a dependent load per term
// costs ~0.3 us each: 20 us for 64 slabs)
__device__ __forceinline__ float ordered_sum16(const float* __restrict__ p, int count, long stride) {
    float acc = 0.f;
    int s = 0;
    for (; s + 16 <= count; s += 16) {
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = p[(long)(s + j) * stride];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc += v[j];
    }
    for (; s < count; ++s) acc += p[(long)s * stride];
    return acc;
}
// The same additions with all 64 terms of a full partition requested at once: in a consuming kernel's prologue the whole
// workgroup waits for this sum, so it pays one load latency instead of four.
__device__ __forceinline__ float ordered_sum64(const float* __restrict__ p, int count, long stride) {
    if (count != 64) return ordered_sum16(p, count, stride);
    float v[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) v[j] = p[(long)j * stride];
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 64; ++j) acc += v[j];
    return acc;
}
// Stage 2 in the prologue of the kernel that consumes the sums: thread j of the workgroup sums column c0 + j of the slab
// partials part[slab][C] into out[j] (LDS, ncols entries; columns past C give 0).  The caller synchronises.
__device__ __forceinline__ void block_ordered_sums(const float* __restrict__ part, int C, int slabs, int c0, int ncols, float* out) {
    for (int j = threadIdx.x; j < ncols; j += blockDim.x) out[j] = c0 + j < C ? ordered_sum64(part + c0 + j, slabs, C) : 0.f;
}
inline bool cols_vectorisable(const void* p, long ld, int N) {
    return N % 4 == 0 && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace t2

// ---------------------------------------------------------------------------------------------
// host-side error plumbing for the C ABI
// ---------------------------------------------------------------------------------------------
void t2_set_error(const char* fmt, ...);
#define T2_CHECK_HIP(expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            t2_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return -2;                                                                       \
        }                                                                                    \
    } while (0)
#define T2_REQUIRE(cond, ...)                                                                \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            t2_set_error(__VA_ARGS__);                                                       \
            return -1;                                                                       \
        }                                                                                    \
    } while (0)
#define T2_LAUNCH_CHECK() T2_CHECK_HIP(hipGetLastError())
#define T2_TRY_RC(expr)             \
    do {                            \
        int rc__ = (expr);          \
        if (rc__ != 0) return rc__; \
    } while (0)

// Dynamic LDS above 64 KB needs hipFuncSetAttribute once per (device, kernel) (and again only for a larger size): the call
// costs the host tens of microseconds, and the per-step kernels are launched hundreds of times per pass.
#include <mutex>
#include <tuple>
#include <vector>
inline int t2_allow_dynamic_lds(const void* fn, size_t smem) {
    if (smem <= 64 * 1024) return 0;
    int dev = 0;
    T2_CHECK_HIP(hipGetDevice(&dev));
    static std::mutex mu;
    static std::vector<std::tuple<int, const void*, size_t>> done;
    std::lock_guard<std::mutex> lock(mu);
    for (auto& e : done)
        if (std::get<0>(e) == dev && std::get<1>(e) == fn) {
            if (std::get<2>(e) >= smem) return 0;
            T2_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
            std::get<2>(e) = smem;
            return 0;
        }
    T2_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    done.emplace_back(dev, fn, smem);
    return 0;
}
