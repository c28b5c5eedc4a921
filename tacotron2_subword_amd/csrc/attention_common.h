// Private to the per-step attention sources (attention.hip, attention_lsa_bwd.hip, attention_gmm.hip, attention_dca.hip):
// block sizes, the forward kernels' block reduction, the one launcher, and the launchers of the kernels that live
// outside attention.hip.
#pragma once
#include <algorithm>

#include "kernels.h"

namespace t2 {

constexpr int NT = 1024;     // forward kernels, 16 waves: latency-bound row streams, more waves = more loads in flight
constexpr int NTB = 512;     // backward kernels, 8 waves (1024 threads spill at 128 VGPRs)
constexpr int NTL = 1024;    // LSA backward on the matrix cores

// The one launch path of the per-step kernels: LDS limit, opt-in to dynamic LDS above 64 KiB, launch, check.
template <class Desc>
inline int attention_launch(void (*kernel)(Desc), dim3 grid, int block, size_t smem, const Desc& d, hipStream_t s, const char* name) {
    T2_REQUIRE(smem <= 160 * 1024, "%s: T_in too long for LDS (%zu bytes)", name, smem);
    T2_TRY_RC(t2_allow_dynamic_lds(reinterpret_cast<const void*>(kernel), smem));
    hipLaunchKernelGGL(kernel, grid, dim3(block), smem, s, d);
    T2_LAUNCH_CHECK();
    return 0;
}
inline int attention_tmax(const AttnStream* st, int n) { int t = 0; for (int i = 0; i < n; ++i) t = std::max(t, st[i].Tin); return t; }
inline int attention_tmax(const AttnBwdStream* st, int n) { int t = 0; for (int i = 0; i < n; ++i) t = std::max(t, st[i].Tin); return t; }

// Kernels outside attention.hip, launched from its two dispatch functions (validation stays there; Tmax = longest memory).
int attention_gmm_fwd_launch(const AttnStepDesc& d, int Tmax, hipStream_t s);
int attention_gmm_bwd_launch(const AttnBwdDesc& d, int Tmax, hipStream_t s);
int attention_dca_fwd_launch(const AttnStepDesc& d, int Tmax, hipStream_t s);
int attention_dca_bwd_launch(const AttnBwdDesc& d, int Tmax, hipStream_t s);
int attention_lsa_bwd_launch(const AttnBwdDesc& d, int Tmax, hipStream_t s);      // chooses matrix-core or scalar kernel

#ifdef __HIPCC__
// max or sum over the NT threads of a forward workgroup.  red: >= NT/64 floats of LDS; result broadcast to all threads
__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
    v = is_max ? wave_max(v) : wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
    return r;
}
#endif  // __HIPCC__

}  // namespace t2
