// What the exact-fp32 matrix-core convolutions of vocoder.hip and waveglow_kernels.hip share, each piece once: the slab staging,
// the MFMA step, the lane-to-element walk of the epilogue, the launcher and the weight pack (slab_gemm.hip).  The dozen lines
// that walk chunks and taps stand in each kernel: the compiler optimises a function before it inlines it, and as a shared
// function they gave the gated instance another schedule, six more registers and + 0.6 % (profiles/README.md, round 29).
//
// Y[row][q] = sum over (channel, tap) of packed weight x act(operand [B][C][N], time contiguous).  A workgroup owns kVocTT = 128
// columns of WM 32-row tiles of one batch item.  Per chunk of kSlabCK = 16 channels it stages the slab [16][128 + 2*halo] in LDS
// once (transform applied, zeros outside [0, N) and past C); every tap reads it at a shifted column: lanes along time, the two
// k-rows of an MFMA step one row stride apart, a stride of 32 mod 64 banks, so the reads are conflict-free.  A wave computes
// 32 rows x 64 columns: two accumulators share each weight fragment.  v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain, so the
// order of every sum is fixed: chunks, taps, then pg and i of slab_mfma_step, ascending.
//
// packed[mtile][step][gate][pg][lane][i] = W[row = 32*mtile + (lane & 31) (+ gate * rows)][k = 16*chunk + 2*(4*pg + i) + (lane >> 5)]
// (zero outside the matrix); step = chunk * taps + tap over segment 0, then the chunks of a second segment of one tap.
#pragma once
#include "kernels.h"

namespace t2 {

// rows ci0 .. ci0 + 15 of xb [C][N], columns t0 - halo .. t0 + kVocTT + halo, to slab [kSlabCK][STRIDE]
template <int STRIDE, int WAVES, class Act>
__device__ __forceinline__ void slab_stage(float* slab, const float* xb, int C, int ci0, int N, long t0, int halo, Act act) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = kVocTT + 2 * halo;
    for (int row = wave; row < kSlabCK; row += WAVES) {
        const int ci = ci0 + row;
        const float* xr = xb + (size_t)ci * N;
        for (int col = lane; col < sw; col += 64) {
            const long t = t0 + col - halo;
            slab[row * STRIDE + col] = (ci < C && t >= 0 && t < N) ? act(xr[t]) : 0.f;
        }
    }
}

// the same for rows that lie `ld` apart and hold N <= ld valid columns (the vocoder's per-item lengths): what lies at or behind
// N is never loaded and stages as zero, as for a row that ends there.  A function of its own, so that the one above and the
// instances built on it stay as they are
template <int STRIDE, int WAVES, class Act>
__device__ __forceinline__ void slab_stage_ld(float* slab, const float* xb, int C, int ci0, int ld, int N, long t0, int halo, Act act) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = kVocTT + 2 * halo;
    for (int row = wave; row < kSlabCK; row += WAVES) {
        const int ci = ci0 + row;
        const float* xr = xb + (size_t)ci * ld;
        for (int col = lane; col < sw; col += 64) {
            const long t = t0 + col - halo;
            slab[row * STRIDE + col] = (ci < C && t >= 0 && t < N) ? act(xr[t]) : 0.f;
        }
    }
}

// one (chunk, tap): 16 k-steps; sb = the lane's column in slab row hk, wj = the lane's fragment of the step's first gate
template <int STRIDE, int GATES>
__device__ __forceinline__ void slab_mfma_step(const float* sb, const f32x4* wj, f32x16 (&acc)[GATES][2]) {
#pragma unroll
    for (int pg = 0; pg < 2; ++pg) {
        f32x4 a[GATES];
#pragma unroll
        for (int g = 0; g < GATES; ++g) a[g] = wj[g * 128 + pg * 64];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* s2 = sb + (pg * 4 + i) * 2 * STRIDE;
            const float b0 = s2[0], b1 = s2[32];
#pragma unroll
            for (int g = 0; g < GATES; ++g) {
                acc[g][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g][i], b0, acc[g][0], 0, 0, 0);
                acc[g][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g][i], b1, acc[g][1], 0, 0, 0);
            }
        }
    }
}

// lane holds column lane & 31 and rows (e&3) + 8*(e>>2) + 4*hk of each 32x32 tile: ep(row, column, values per gate) for every element
// of tile mt inside rows x Nq.  ep captures by value: through a reference the (item, row) part of an address is not hoisted
template <int WM, int GATES, class Ep>
__device__ __forceinline__ void slab_walk(const f32x16 (&acc)[GATES][2], int mt, int rows, int Nq, Ep ep) {
    const int lane = threadIdx.x & 63, wt = (threadIdx.x >> 6) / WM, hk = lane >> 5;
    const long t0 = (long)blockIdx.x * kVocTT;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const long q = t0 + wt * 64 + n * 32 + (lane & 31);
        if (q >= Nq) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = mt * 32 + (e & 3) + 8 * (e >> 2) + 4 * hk;
            if (r >= rows) continue;
            float v[GATES];
#pragma unroll
            for (int g = 0; g < GATES; ++g) v[g] = acc[g][n][e];
            ep(r, q, v);
        }
    }
}

// k4, k2, k1: the kernel's instances for 4, 2 and 1 row tiles per workgroup (WM * 128 threads), chosen by the mtiles row tiles
// there are; grid = column tiles x (row blocks * ygroups) x B
template <class P>
int slab_launch(void (*k4)(P), void (*k2)(P), void (*k1)(P), const P& p, int mtiles, long ncols, int ygroups, int B, hipStream_t s) {
    const int wm = mtiles >= 4 ? 4 : (mtiles >= 2 ? 2 : 1);
    dim3 grid((unsigned)((ncols + kVocTT - 1) / kVocTT), (unsigned)((mtiles + wm - 1) / wm * ygroups), (unsigned)B);
    void (*const k)(P) = wm == 4 ? k4 : (wm == 2 ? k2 : k1);
    hipLaunchKernelGGL(k, grid, dim3(wm * 128), 0, s, p);
    T2_LAUNCH_CHECK();
    return 0;
}

// Source of one packed operand: element (gate, row, k, tap) of a segment is w[base + gate*gs + (row / split)*rhi + (row % split)*rlo
// + k*ks + tap*ts]; K = 0 leaves segment 1 out, split = 0 counts as 1.  slab_pack writes slab_packed_floats(gates, rows, s0.K, s0.taps, s1.K) floats to `out`.
struct SlabPackSeg { const float* w; int K, taps; long base, gs, rhi, rlo, ks, ts; };
struct SlabPack { SlabPackSeg s0, s1; float* out; int gates, rows, split; };
int slab_pack(SlabPack p, hipStream_t s);

}  // namespace t2
