// The one weight pack of the slab GEMM (slab_gemm.h says the layout and how a source is described): vocoder.hip and
// waveglow_kernels.hip fill in strides and call slab_pack.
#include "slab_gemm.h"

namespace t2 {

__global__ void __launch_bounds__(256) slab_pack_kernel(SlabPack p, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int nst0 = slab_chunks(p.s0.K) * p.s0.taps, nsteps = nst0 + slab_chunks(p.s1.K);
    const int i = idx & 3, lane = (idx >> 2) & 63, pg = (idx >> 8) & 1;
    size_t rest = idx >> 9;
    const int gate = rest % p.gates; rest /= p.gates;
    const int step = rest % nsteps, mt = (int)(rest / nsteps);
    const int r = mt * 32 + (lane & 31), kloc = 2 * (4 * pg + i) + (lane >> 5);
    const bool first = step < nst0;
    const SlabPackSeg sg = first ? p.s0 : p.s1;
    const int st = first ? step : step - nst0, kk = (st / sg.taps) * kSlabCK + kloc, j = st % sg.taps;
    float v = 0.f;
    if (r < p.rows && kk < sg.K)
        v = sg.w[sg.base + gate * sg.gs + (long)(r / p.split) * sg.rhi + (long)(r % p.split) * sg.rlo + (long)kk * sg.ks + (long)j * sg.ts];
    p.out[idx] = v;
}

int slab_pack(SlabPack p, hipStream_t s) {
    p.s1.taps = 1;
    if (p.split < 1) p.split = 1;                  // a description that leaves it out means no split
    const size_t total = slab_packed_floats(p.gates, p.rows, p.s0.K, p.s0.taps, p.s1.K);
    hipLaunchKernelGGL(slab_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, total);
    T2_LAUNCH_CHECK();
    return 0;
}

}  // namespace t2
