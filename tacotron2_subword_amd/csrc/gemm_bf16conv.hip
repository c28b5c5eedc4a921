// ---------------------------------------------------------------------------------------------
// bf16-operand variant (fp32 in HBM, converted while staging; fp32 accumulate):
// v_mfma_f32_32x32x16_bf16, tile 128x128x64, LDS tiles row-major [row][k] bf16 with an XOR
// swizzle of the 16-byte slots (swz16), double buffered, next chunk prefetched into registers.  16x the matrix rate of the fp32 path, so
// this kernel is bound by operand delivery (each thread moves 64 B of fp32 per MFMA).
// ---------------------------------------------------------------------------------------------
#include "gemm_common.h"

namespace t2 {
namespace gemm_detail {
namespace {

// ---- two-phase loaders of a WHOLE tile (all 128 rows and all 64 k in range, 16-byte aligned): `issue` only requests
// the fp32 data into registers, `finish` converts and stores to LDS.  Keeping the raw registers alive lets the main loop
// hold TWO k-steps in flight per wave: measured on the old loop the wait + convert sat directly behind the loads, in
// front of the MFMAs (one k-step of 64 KB in flight per workgroup = the ~50 GB/s per CU that bounded the kernel).
// An implicit-conv operand selects, without branches: a task outside its utterance reads the base and converts zeros.
struct RawKC { f32x4 lo[4], hi[4]; unsigned ok; };
struct RawMC { f32x4 v[8]; unsigned ok; };
// 128 rows x 64 k, k contiguous in the source: 4 tasks (row, 8 k) per thread.
__device__ __forceinline__ void issue_kc(const float* __restrict__ base, long srow, int row0, int k0, ConvAddr cv, RawKC& r) {
    r.ok = 0xFu;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = threadIdx.x + i * 256, row = row0 + (q >> 3), k = k0 + (q & 7) * 8;
        const float* p;
        if (cv.T) {
            const int dk = k / cv.C, ci = k - dk * cv.C, t = row % cv.T + dk - cv.pad;
            const bool ok = t >= 0 && t < cv.T;
            if (!ok) r.ok &= ~(1u << i);
            p = base + (ok ? (long)(row + dk - cv.pad) * cv.C + ci : 0l);
        } else {
            p = base + (long)row * srow + k;
        }
        r.lo[i] = *reinterpret_cast<const f32x4*>(p); r.hi[i] = *reinterpret_cast<const f32x4*>(p + 4);
    }
}
__device__ __forceinline__ bf16x8 convert_kc(const RawKC& r, int i) {
    const f32x4 zz = {0.f, 0.f, 0.f, 0.f};
    const bool ok = (r.ok >> i) & 1u;
    return pack8(ok ? r.lo[i] : zz, ok ? r.hi[i] : zz);
}
__device__ __forceinline__ void store16_kc(__bf16* __restrict__ lds, const bf16x8 (&regs)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = threadIdx.x + i * 256;
        *reinterpret_cast<bf16x8*>(lds + swz16(q >> 3, q & 7)) = regs[i];
    }
}
__device__ __forceinline__ void finish_kc(__bf16* __restrict__ lds, const RawKC& r) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = threadIdx.x + i * 256;
        *reinterpret_cast<bf16x8*>(lds + swz16(q >> 3, q & 7)) = convert_kc(r, i);
    }
}
// 64 k-rows x 128 "rows" (m or n), rows contiguous in the source: one task (4 rows, 8 k) per thread.
__device__ __forceinline__ void issue_mc(const float* __restrict__ base, long sk, int row0, int k0, ConvAddr cv, RawMC& r) {
    const int row = row0 + (threadIdx.x & 31) * 4, kb = k0 + (threadIdx.x >> 5) * 8;
    r.ok = 0xFFu;
    if (cv.T) {
        const int dk = row / cv.C, ci = row - dk * cv.C;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int k = kb + kk, t = k % cv.T + dk - cv.pad;
            const bool ok = t >= 0 && t < cv.T;
            if (!ok) r.ok &= ~(1u << kk);
            r.v[kk] = *reinterpret_cast<const f32x4*>(base + (ok ? (long)(k + dk - cv.pad) * cv.C + ci : 0l));
        }
    } else {
        const float* p = base + (long)kb * sk + row;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) r.v[kk] = *reinterpret_cast<const f32x4*>(p + (long)kk * sk);
    }
}
__device__ __forceinline__ bf16x8 convert_mc(const RawMC& r, int mm) {
    bf16x8 o;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) o[kk] = (__bf16)(((r.ok >> kk) & 1u) ? r.v[kk][mm] : 0.f);
    return o;
}
__device__ __forceinline__ void store16_mc(__bf16* __restrict__ lds, const bf16x8 (&regs)[4]) {
    const int row = (threadIdx.x & 31) * 4, ks = threadIdx.x >> 5;
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) *reinterpret_cast<bf16x8*>(lds + swz16(row + mm, ks)) = regs[mm];
}
__device__ __forceinline__ void finish_mc(__bf16* __restrict__ lds, const RawMC& r) {
    const int row = (threadIdx.x & 31) * 4, ks = threadIdx.x >> 5;
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) *reinterpret_cast<bf16x8*>(lds + swz16(row + mm, ks)) = convert_mc(r, mm);
}
template <bool KC> struct RawOf { using type = RawMC; };
template <> struct RawOf<true> { using type = RawKC; };

// ---- loaders of ANY tile, converted at once: a whole one through the loaders above, an edge tile element by element
__device__ __forceinline__ void load16_kc(const float* __restrict__ base, long srow, int row0, int nrows, int k0, int kend, int vec,
                                          ConvAddr cv, bf16x8 (&regs)[4]) {
    if ((cv.T || vec) && row0 + 128 <= nrows && k0 + BK16 <= kend) {
        RawKC r;
        issue_kc(base, srow, row0, k0, cv, r);
#pragma unroll
        for (int i = 0; i < 4; ++i) regs[i] = convert_kc(r, i);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = threadIdx.x + i * 256, row = row0 + (q >> 3), k = k0 + (q & 7) * 8;
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
        if (row < nrows && k < kend) {
            if (cv.T) {                                      // C % 8 == 0: the 8 k's share one tap
                const int dk = k / cv.C, ci = k - dk * cv.C, t = row % cv.T + dk - cv.pad;
                if (t >= 0 && t < cv.T) {
                    const float* p = base + (long)(row + dk - cv.pad) * cv.C + ci;
                    lo = *reinterpret_cast<const f32x4*>(p); hi = *reinterpret_cast<const f32x4*>(p + 4);
                }
            } else {
                const float* p = base + (long)row * srow + k;
                if (vec && k + 7 < kend) {
                    lo = *reinterpret_cast<const f32x4*>(p); hi = *reinterpret_cast<const f32x4*>(p + 4);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { if (k + j < kend) lo[j] = p[j]; if (k + 4 + j < kend) hi[j] = p[4 + j]; }
                }
            }
        }
        regs[i] = pack8(lo, hi);
    }
}
__device__ __forceinline__ void load16_mc(const float* __restrict__ base, long sk, int row0, int nrows, int k0, int kend, int vec,
                                          ConvAddr cv, bf16x8 (&regs)[4]) {
    if ((cv.T || vec) && row0 + 128 <= nrows && k0 + BK16 <= kend) {
        RawMC r;
        issue_mc(base, sk, row0, k0, cv, r);
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) regs[mm] = convert_mc(r, mm);
        return;
    }
    const int row = row0 + (threadIdx.x & 31) * 4, kb = k0 + (threadIdx.x >> 5) * 8;
    f32x4 v[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
        const int k = kb + kk;
        v[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k < kend && row < nrows) {
            if (cv.T) {
                const int dk = row / cv.C, ci = row - dk * cv.C, t = k % cv.T + dk - cv.pad;
                if (t >= 0 && t < cv.T) v[kk] = *reinterpret_cast<const f32x4*>(base + (long)(k + dk - cv.pad) * cv.C + ci);
            } else {
                const float* p = base + (long)k * sk + row;
                if (vec && row + 3 < nrows) v[kk] = *reinterpret_cast<const f32x4*>(p);
                else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (row + j < nrows) v[kk][j] = p[j];
                }
            }
        }
    }
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
        bf16x8 o;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) o[kk] = (__bf16)v[kk][mm];
        regs[mm] = o;
    }
}

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmK g) {
    const GemmDesc& d = g.d;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem16[];
    __bf16* const lds = reinterpret_cast<__bf16*>(smem16);
    auto As = [&](int b) { return lds + b * (128 * PK16); };
    auto Bs = [&](int b) { return lds + (2 + b) * (128 * PK16); };

    const int z = blockIdx.z;
    const int split = z % d.splitk, bz = z / d.splitk;
    const float* A = d.A + (long)bz * d.bsA;
    const float* B = d.B + (long)bz * d.bsB;
    const int m0 = blockIdx.y * 128, n0 = blockIdx.x * 128;
    const int kbeg = split * g.kchunks * BK, kend = min(d.K, kbeg + g.kchunks * BK);   // kchunks counts 16-wide chunks

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    f32x16 acc[2][2];
    zero(acc);
    auto mma = [&](int buf) {
        const __bf16* as = As(buf);
        const __bf16* bs = Bs(buf);
#pragma unroll
        for (int ks = 0; ks < BK16 / 16; ++ks) {
            bf16x8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const bf16x8*>(as + swz16(wm * 64 + i * 32 + r, 2 * ks + h));
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const bf16x8*>(bs + swz16(wn * 64 + j * 32 + r, 2 * ks + h));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    };

    const ConvAddr cva{d.conv_a ? d.conv_T : 0, d.conv_C, d.conv_pad}, cvb{d.conv_b ? d.conv_T : 0, d.conv_C, d.conv_pad};
    // interior workgroup: every tile row/column in range, whole 64-wide k-steps, aligned operands -> pipelined loop
    const bool interior = m0 + 128 <= d.M && n0 + 128 <= d.N && kbeg < kend && (kend - kbeg) % BK16 == 0 && g.avec && g.bvec;
    if (interior) {
        using RA = typename RawOf<A_KC>::type;
        using RB = typename RawOf<B_KC>::type;
        RA a0; RB b0;
        auto issue = [&](int k0, RA& ra_, RB& rb_) {
            if constexpr (A_KC) issue_kc(A, d.sam, m0, k0, cva, ra_); else issue_mc(A, d.sak, m0, k0, cva, ra_);
            if constexpr (B_KC) issue_kc(B, d.sbn, n0, k0, cvb, rb_); else issue_mc(B, d.sbk, n0, k0, cvb, rb_);
        };
        auto finish = [&](int buf, const RA& ra_, const RB& rb_) {
            if constexpr (A_KC) finish_kc(As(buf), ra_); else finish_mc(As(buf), ra_);
            if constexpr (B_KC) finish_kc(Bs(buf), rb_); else finish_mc(Bs(buf), rb_);
        };
        const int nks = (kend - kbeg) / BK16;
        issue(kbeg, a0, b0);
        finish(0, a0, b0);
        __syncthreads();
        int cur = 0;
        for (int ks = 0; ks < nks; ++ks) {
            const bool more = ks + 1 < nks;
            if (more) issue(kbeg + (ks + 1) * BK16, a0, b0);          // in flight during the MFMAs below
            __builtin_amdgcn_sched_barrier(0);
            mma(cur);
            __builtin_amdgcn_sched_barrier(0);
            if (more) finish(cur ^ 1, a0, b0);
            __syncthreads();
            cur ^= 1;
        }
    } else {
        bf16x8 ra[4], rb[4];
        auto load = [&](int k0) {
            if (A_KC) load16_kc(A, d.sam, m0, d.M, k0, kend, g.avec, cva, ra); else load16_mc(A, d.sak, m0, d.M, k0, kend, g.avec, cva, ra);
            if (B_KC) load16_kc(B, d.sbn, n0, d.N, k0, kend, g.bvec, cvb, rb); else load16_mc(B, d.sbk, n0, d.N, k0, kend, g.bvec, cvb, rb);
        };
        auto store = [&](int b) {
            if (A_KC) store16_kc(As(b), ra); else store16_mc(As(b), ra);
            if (B_KC) store16_kc(Bs(b), rb); else store16_mc(Bs(b), rb);
        };
        if (kbeg < kend) { load(kbeg); store(0); }
        __syncthreads();
        int cur = 0;
        for (int k0 = kbeg; k0 < kend; k0 += BK16) {
            const bool more = k0 + BK16 < kend;
            if (more) load(k0 + BK16);
            mma(cur);
            if (more) store(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
    }

    // Epilogue through LDS (free behind the loop's last barrier); the element's arithmetic is epilogue_value
    const RngKey key = rng_key(d.seed, d.site);
    float* ws = d.splitk > 1 ? d.ws + ((long)split * d.batch + bz) * (long)d.M * d.N : nullptr;
    store_rows_lds<true>(d, d.C + (long)bz * d.bsC, ws, reinterpret_cast<float*>(smem16) + wave * 4096, acc, m0 + wm * 64, n0 + wn * 64 + (lane & 15) * 4,
                         [&](int m, int n, int c, float x) { return epilogue_value(d, m, n + c, x, key); });
}

}  // namespace

int launch_gemm_bf16conv(const GemmK& g, dim3 grid, hipStream_t s) {
    // one instantiation per pair of unit strides, K-contiguous first: [A k-contiguous ? 0 : 2] + [B k-contiguous ? 0 : 1]
    using Kernel = void (*)(GemmK);
    static const Kernel bf16conv[] = {gemm_bf16_kernel<true, true>, gemm_bf16_kernel<true, false>, gemm_bf16_kernel<false, true>, gemm_bf16_kernel<false, false>};
    const size_t smem = (size_t)4 * 128 * PK16 * sizeof(__bf16);     // (64 KB: needs no t2_allow_dynamic_lds)
    hipLaunchKernelGGL(bf16conv[(g.d.sak == 1 ? 0 : 2) + (g.d.sbk == 1 ? 0 : 1)], grid, dim3(256), smem, s, g);
    T2_LAUNCH_CHECK();
    return 0;
}

}  // namespace gemm_detail
}  // namespace t2
