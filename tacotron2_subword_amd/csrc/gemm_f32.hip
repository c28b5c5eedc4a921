// fp32 GEMM on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 fma chains, so the
// result is an ordinary k-ordered fp32 dot product — this is the path the 1e-4 parity contract
// is stated on).  C = act(alpha * A.B + bias) [dropout] + beta * C.
//
// Layout: 256 threads = 4 waves (2x2); block tile BM x BN, BK = 16; each wave owns a
// (BM/2)x(BN/2) sub-tile as (BM/64)x(BN/64) MFMA tiles of 32x32.  Both operands are staged
// k-major in LDS ([BK][BM+4]) so that a fragment read is 32 consecutive floats per half-wave
// (conflict-free ds_read_b32) whichever of the two source strides is the contiguous one.
// Global loads are 16 B per lane along the contiguous stride; the next K-chunk is prefetched
// into registers while the current one feeds the MFMAs (one barrier per chunk).
#include "gemm_common.h"

namespace t2 {
namespace gemm_detail {
namespace {

// Load one operand tile (R rows x BK) into registers.  KC: k is the contiguous stride.
template <int R, bool KC>
__device__ __forceinline__ void load_tile(const float* __restrict__ base, long srow, long sk, int row0, int nrows,
                                          int k0, int kend, int vec, ConvAddr cv, f32x4 (&regs)[R * 4 / 256]) {
    constexpr int NQ = R * 4 / 256;
    if (!cv.T && vec && row0 + R <= nrows && k0 + BK <= kend) {          // interior tile: unconditional 16-byte loads
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = threadIdx.x + i * 256;
            const float* p = KC ? base + (long)(row0 + (q >> 2)) * srow + k0 + (q & 3) * 4
                                : base + (long)(k0 + q / (R / 4)) * sk + row0 + (q % (R / 4)) * 4;
            regs[i] = *reinterpret_cast<const f32x4*>(p);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        int q = threadIdx.x + i * 256;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (KC) {
            int row = row0 + (q >> 2), k = k0 + (q & 3) * 4;
            if (row < nrows) {
                if (cv.T) {                                  // rows = frames m, k = dk*C + ci  (C % 4 == 0)
                    if (k < kend) {
                        const int dk = k / cv.C, ci = k - dk * cv.C, t = row % cv.T + dk - cv.pad;
                        if (t >= 0 && t < cv.T) v = *reinterpret_cast<const f32x4*>(base + (long)(row + dk - cv.pad) * cv.C + ci);
                    }
                } else {
                    const float* p = base + (long)row * srow + k;
                    if (vec && k + 3 < kend) {
                        v = *reinterpret_cast<const f32x4*>(p);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) if (k + j < kend) v[j] = p[j];
                    }
                }
            }
        } else {
            int k = k0 + q / (R / 4), row = row0 + (q % (R / 4)) * 4;
            if (k < kend) {
                if (cv.T) {                                  // k = frames m, rows = dk*C + ci
                    if (row < nrows) {
                        const int dk = row / cv.C, ci = row - dk * cv.C, t = k % cv.T + dk - cv.pad;
                        if (t >= 0 && t < cv.T) v = *reinterpret_cast<const f32x4*>(base + (long)(k + dk - cv.pad) * cv.C + ci);
                    }
                } else {
                    const float* p = base + (long)k * sk + row;
                    if (vec && row + 3 < nrows) {
                        v = *reinterpret_cast<const f32x4*>(p);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) if (row + j < nrows) v[j] = p[j];
                    }
                }
            }
        }
        regs[i] = v;
    }
}

template <int R, bool KC>
__device__ __forceinline__ void store_tile(float* __restrict__ lds, const f32x4 (&regs)[R * 4 / 256]) {
    constexpr int NQ = R * 4 / 256;
    constexpr int P = R + 4;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        int q = threadIdx.x + i * 256;
        if (KC) {
            int row = q >> 2, k = (q & 3) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) lds[(k + j) * P + row] = regs[i][j];
        } else {
            int k = q / (R / 4), row = (q % (R / 4)) * 4;
            *reinterpret_cast<f32x4*>(&lds[k * P + row]) = regs[i];
        }
    }
}

template <int BM, int BN, bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void gemm_kernel(GemmK g) {
    const GemmDesc& d = g.d;
    constexpr int TM = BM / 64, TN = BN / 64;
    constexpr int PA = BM + 4, PB = BN + 4;
    __shared__ __attribute__((aligned(16))) float As[2][BK * PA];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK * PB];

    const int z = blockIdx.z;
    const int split = z % d.splitk, bz = z / d.splitk;
    const float* A = d.A + (long)bz * d.bsA;
    const float* B = d.B + (long)bz * d.bsB;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int kbeg = split * g.kchunks * BK;
    const int kend = min(d.K, kbeg + g.kchunks * BK);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, hk = lane >> 5;

    f32x16 acc[TM][TN];
    zero(acc);

    const ConvAddr cva{d.conv_a ? d.conv_T : 0, d.conv_C, d.conv_pad}, cvb{d.conv_b ? d.conv_T : 0, d.conv_C, d.conv_pad};
    f32x4 ra[BM * 4 / 256], rb[BN * 4 / 256];
    if (kbeg < kend) {
        load_tile<BM, A_KC>(A, d.sam, d.sak, m0, d.M, kbeg, kend, g.avec, cva, ra);
        load_tile<BN, B_KC>(B, d.sbn, d.sbk, n0, d.N, kbeg, kend, g.bvec, cvb, rb);
        store_tile<BM, A_KC>(As[0], ra);
        store_tile<BN, B_KC>(Bs[0], rb);
    }
    __syncthreads();
    int cur = 0;
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        const bool more = k0 + BK < kend;
        if (more) {
            load_tile<BM, A_KC>(A, d.sam, d.sak, m0, d.M, k0 + BK, kend, g.avec, cva, ra);
            load_tile<BN, B_KC>(B, d.sbn, d.sbk, n0, d.N, k0 + BK, kend, g.bvec, cvb, rb);
        }
        const float* as = As[cur] + wm * (BM / 2) + r;
        const float* bs = Bs[cur] + wn * (BN / 2) + r;
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = as[(2 * kk + hk) * PA + i * 32];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = bs[(2 * kk + hk) * PB + j * 32];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) {
            store_tile<BM, A_KC>(As[cur ^ 1], ra);
            store_tile<BN, B_KC>(Bs[cur ^ 1], rb);
        }
        __syncthreads();
        cur ^= 1;
    }

    float* ws = d.splitk > 1 ? d.ws + ((long)split * d.batch + bz) * (long)d.M * d.N : nullptr;
    store_direct<true>(d, d.C + (long)bz * d.bsC, ws, acc, m0 + wm * (BM / 2), n0 + wn * (BN / 2), r, hk);
}

}  // namespace

int launch_gemm_f32(const GemmK& g, GemmKernel kernel, dim3 grid, hipStream_t s) {
    // one instantiation per pair of unit strides, K-contiguous first: [A k-contiguous ? 0 : 2] + [B k-contiguous ? 0 : 1]
    using Kernel = void (*)(GemmK);
    static const Kernel f32_64[] = {gemm_kernel<64, 64, true, true>, gemm_kernel<64, 64, true, false>, gemm_kernel<64, 64, false, true>, gemm_kernel<64, 64, false, false>};
    static const Kernel f32_128[] = {gemm_kernel<128, 128, true, true>, gemm_kernel<128, 128, true, false>, gemm_kernel<128, 128, false, true>, gemm_kernel<128, 128, false, false>};
    const Kernel k = (kernel == GemmKernel::f32_64 ? f32_64 : f32_128)[(g.d.sak == 1 ? 0 : 2) + (g.d.sbk == 1 ? 0 : 1)];
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, g);
    T2_LAUNCH_CHECK();
    return 0;
}

}  // namespace gemm_detail
}  // namespace t2
