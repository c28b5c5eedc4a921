// The bf16-SOURCE GEMM kernels (128 x 128 and 256 x 256 tiles) and the staging casts that make the bf16 copies they read.
// The exact fp32 kernel is gemm_f32.hip, the converting bf16 kernel gemm_bf16conv.hip, the plan and the executor
// gemm_dispatch.hip; gemm_common.h holds what they share.
#include "gemm_common.h"

namespace t2 {
namespace gemm_detail {
namespace {
// ---------------------------------------------------------------------------------------------
// bf16-SOURCE variant: both operands already bf16 and K-contiguous in memory (A16 [M][lda], B16 [N][ldb]), staged by
// the cast kernels below (or handed over by the caller).  Whole 128x128 tiles and whole 64-wide k-steps only.  Half the
// operand bytes per MFMA of the converting kernel and no conversion in the loop; two k-steps of 16-byte loads
// (8 VGPRs each per operand) are kept in flight per wave.
// ---------------------------------------------------------------------------------------------
// Block tile 128 x 128: 2 x 2 waves, each a 2 x 2 grid of 32x32 MFMA tiles; 256 threads, so 4 tasks (row, 8 k) per thread
// and operand per k-step.  See the launch site for the other shapes that were measured.
struct Raw16 { bf16x8 a[4], b[4]; unsigned ok; };
// CONV_A: A16 is the bf16 copy of the frames X[M][C] and the operand is its implicit im2col (ConvAddr); C % 64 == 0, so
// one 64-wide k-step lies inside one tap: the tile is the frame tile shifted by (tap - pad) rows, rows that leave
// their utterance read as zero.  tpos[i] = (m0 + row_i) % T.
template <bool CONV_A>
__device__ __forceinline__ void issue16(const __bf16* __restrict__ A, long lda, const __bf16* __restrict__ B, long ldb, int k0,
                                        ConvAddr cv, const int (&tpos)[4], Raw16& r) {
    r.ok = ~0u;
    int shift = 0, ka = k0;
    if constexpr (CONV_A) { const int dk = k0 / cv.C; ka = k0 - dk * cv.C; shift = dk - cv.pad; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = threadIdx.x + i * 256;
        long row = q >> 3;
        if constexpr (CONV_A) {
            const bool ok = (unsigned)(tpos[i] + shift) < (unsigned)cv.T;
            if (ok) row += shift; else r.ok &= ~(1u << i);
        }
        r.a[i] = *reinterpret_cast<const bf16x8*>(A + row * lda + ka + (q & 7) * 8);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = threadIdx.x + i * 256;
        r.b[i] = *reinterpret_cast<const bf16x8*>(B + (long)(q >> 3) * ldb + k0 + (q & 7) * 8);
    }
}
template <bool CONV_A>
__device__ __forceinline__ void finish16(__bf16* __restrict__ as, __bf16* __restrict__ bs, const Raw16& r) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = threadIdx.x + i * 256;
        bf16x8 a = r.a[i];
        if constexpr (CONV_A) {
            if (!((r.ok >> i) & 1u)) {
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = (__bf16)0.f;
            }
        }
        *reinterpret_cast<bf16x8*>(as + swz16(q >> 3, q & 7)) = a;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = threadIdx.x + i * 256;
        *reinterpret_cast<bf16x8*>(bs + swz16(q >> 3, q & 7)) = r.b[i];
    }
}

template <bool CONV_A>
__global__ __launch_bounds__(256) void gemm_bf16src_kernel(GemmK g, const __bf16* __restrict__ A16, long lda, const __bf16* __restrict__ B16, long ldb) {
    constexpr int BM = 128, BN = 128;
    const ConvAddr cva{g.d.conv_T, g.d.conv_C, g.d.conv_pad};
    int tpos[4];
    const GemmDesc& d = g.d;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem16[];
    __bf16* const lds = reinterpret_cast<__bf16*>(smem16);
    auto As = [&](int b) { return lds + b * (BM * PK16); };
    auto Bs = [&](int b) { return lds + 2 * (BM * PK16) + b * (BN * PK16); };

    const int split = blockIdx.z;
    int bx = blockIdx.x, by = blockIdx.y;
    if (g.xcd_swizzle) xcd_remap(8, bx, by);
    const int m0 = by * BM, n0 = bx * BN;
    const int kbeg = split * g.kchunks * BK, kend = min(d.K, kbeg + g.kchunks * BK);
    const __bf16* A = A16 + (long)m0 * lda;
    const __bf16* B = B16 + (long)n0 * ldb;
#pragma unroll
    for (int i = 0; i < 4; ++i) tpos[i] = CONV_A ? (m0 + ((int)(threadIdx.x + i * 256) >> 3)) % cva.T : 0;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / 2, wn = wave % 2;
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
    const int nks = (kend - kbeg) / BK16;
    if (nks > 0) {
        Raw16 r0, r1;
        issue16<CONV_A>(A, lda, B, ldb, kbeg, cva, tpos, r0);
        if (nks > 1) issue16<CONV_A>(A, lda, B, ldb, kbeg + BK16, cva, tpos, r1);
        finish16<CONV_A>(As(0), Bs(0), r0);
        __syncthreads();
        // invariant at the top of step ks: LDS buffer ks&1 holds k-step ks, `nxt` holds k-step ks+1 (in flight),
        // `free` is empty and receives k-step ks+2 before the MFMAs
        auto step = [&](int ks, Raw16& nxt, Raw16& free_) {
            if (ks + 2 < nks) issue16<CONV_A>(A, lda, B, ldb, kbeg + (ks + 2) * BK16, cva, tpos, free_);
            __builtin_amdgcn_sched_barrier(0);
            mma(ks & 1);
            __builtin_amdgcn_sched_barrier(0);
            if (ks + 1 < nks) finish16<CONV_A>(As((ks & 1) ^ 1), Bs((ks & 1) ^ 1), nxt);
            __syncthreads();
        };
        int ks = 0;
        for (; ks + 1 < nks; ks += 2) { step(ks, r1, r0); step(ks + 1, r0, r1); }
        if (ks < nks) step(ks, r1, r0);
    }

    float* ws = d.splitk > 1 ? d.ws + (long)split * (long)d.M * d.N : nullptr;
    store_direct<false>(d, d.C, ws, acc, m0 + wm * 64, n0 + wn * 64, r, h);
}

template <bool CONV_A>
int launch_bf16src(const GemmK& g, const __bf16* pa, long lda, const __bf16* pb, long ldb, dim3 grid, hipStream_t s) {
    const size_t smem = (size_t)2 * (128 + 128) * PK16 * sizeof(__bf16);
    T2_TRY_RC(t2_allow_dynamic_lds(reinterpret_cast<const void*>(gemm_bf16src_kernel<CONV_A>), smem));   // (per device and kernel)
    GemmK gk = g;
    gk.xcd_swizzle = (grid.x * grid.y) % 8 == 0 && grid.y >= 8;
    hipLaunchKernelGGL((gemm_bf16src_kernel<CONV_A>), grid, dim3(256), smem, s, gk, pa, lda, pb, ldb);
    T2_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// 256 x 256 block tile, BK = 64, 8 waves as 2 (M) x 4 (N), each owning 128 x 64 of the tile as 4 x 2 MFMA tiles of
// 32 x 32 (128 accumulator registers).  One workgroup per CU; 128 KB of LDS = 2 K-tiles x 4 half-tiles of 16 KB:
//     A0 / A1: the first / second 64 rows of BOTH wave rows        B0 / B1: the first / second 32 columns of the 4 wave columns
// so a half-tile holds what every wave needs for one operand of one quadrant of its output.  Operands go global -> LDS
// with LDS-DMA (buffer_load_dwordx4 ... lds: no staging registers); an instruction writes 1 KB = 8 rows of 128 B in lane
// order, and the bank swizzle (16-byte chunk ^= (row >> 1) & 7: conflict-free ds_read_b128 of 32 rows x 2 chunks) is put on
// the SOURCE address of each lane.
//
// K loop: 4 phases per K-tile, one output quadrant x K = 64 (8 MFMAs) each:
//     phase   quadrant   fragment reads      LDS-DMA issued (one half-tile = 2 instructions per thread)
//       0     (a0, b0)   A0, B0 of kt        B1 of kt+1
//       1     (a0, b1)   B1 of kt            A1 of kt+1
//       2     (a1, b1)   A1 of kt            A0 of kt+2
//       3     (a1, b0)   -                   B0 of kt+2
//   phase = { reads ; issue ; s_waitcnt vmcnt(8) ; s_barrier ; MFMAs ; s_barrier }: raw barriers and counted waits, so
//   four half-tiles stay in flight across every barrier (a half-tile is read 5-6 phases after it was issued).  A staged
//   buffer is read one phase after the wait + barrier that retires it and restaged at least two phases after its last
//   read.  The two wave rows run one barrier apart (wave row 1 enters through an extra barrier), so on each SIMD one wave
//   reads fragments while the other one issues MFMAs.  The last two K-tiles drain with vmcnt 4 / 2 / 0.
// ---------------------------------------------------------------------------------------------
//
// KM (k-major operands): A16 is [K][lda] (element (m, k) at k * lda + m), B16 is [K][ldb], the layout the weight-gradient
// products find their operands in (K = frames).  A half-tile is then 64 k-rows of 128 columns = 256-byte rows, still 16 KB,
// staged by the same LDS-DMA instructions (1 KB = 4 k-rows per wave) and read with ds_read_b64_tr_b16: a 16-lane group
// reads 4 k-rows x 16 columns and each lane receives the 4 k of ITS column, so two reads (k rows 8 hk .. + 3, + 4 .. + 7)
// give a lane exactly the 8 k of the ds_read_b128 fragment in the same slots: the products are bit-identical to the
// K-contiguous path.  Rows are 64 dwords, so the 4 k-rows of a read would share their banks; 16-byte chunk c of k-row kr
// is kept at chunk c ^ ((kr & 3) << 2) (on the source offsets, like the K-contiguous swizzle), which spreads the 4 rows
// x 64 bytes of a half-wave over all 64 banks.  kr & 3 is a function of the lane alone, so the K-step and the 4-row
// half of a fragment are immediate offsets on one address register per MFMA tile.  The B half-tiles take the columns
// h * 64 .. + 63 of each 128-column half of the tile (wave column wc: 32 of them), not h * 32 .. + 31 of each 64, so that
// every k-row of a half-tile is made of whole 128-byte lines, as in the A half-tiles (64-byte pieces measured the same).
// CONV_B (with KM): B16 holds the frames X[K][C] and the operand is their implicit im2col [K][taps * C]; a workgroup's
// 256 columns lie inside one tap (C % 256 == 0), so its B tile is X with the ROWS shifted by tap - pad (folded into the
// buffer base) and k-rows that leave their utterance read as zero through an offset past the buffer's range.
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
// One 8-k fragment of a k-major tile: two transposed reads (k rows + 0 .. 3 and + 4 .. 7 of the 16-k step at byte OFF).
// Inline assembly, not __builtin_amdgcn_ds_read_tr16_b64: the compiler orders the builtin behind every LDS-DMA in flight
// (s_waitcnt vmcnt(0) in front of each group of reads, which empties the staging pipeline: 0.66 instead of 0.56 ms on
// 4096 x 3072 x 25600).  Nor does it count these reads in lgkmcnt: lds_tr_wait() stands between them and their MFMAs.
template <int OFF>
__device__ __forceinline__ bf16x8 lds_read_tr16(unsigned addr) {
    bf16x4 lo, hi;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(addr), "n"(OFF));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(addr), "n"(OFF + 1024));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// waits until at most N of the LDS reads issued so far are outstanding; the fragments pass through it so that no MFMA
// that reads them moves in front
template <int N>
__device__ __forceinline__ void lds_tr_wait(bf16x8& a0, bf16x8& a1, bf16x8& b) {
    asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(a0), "+v"(a1), "+v"(b) : "n"(N));
}
template <bool CONV_A, bool KM, bool CONV_B>
__global__ __launch_bounds__(512) void gemm_bf16src256_kernel(GemmK g, const __bf16* __restrict__ A16, long lda, const __bf16* __restrict__ B16, long ldb) {
    const GemmDesc& d = g.d;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem16[];
    typedef __attribute__((address_space(3))) void* lds_ptr;
    int bx = blockIdx.x, by = blockIdx.y;
    if (g.xcd_swizzle) xcd_remap(4, bx, by);
    const int m0 = by * 256, n0 = bx * 256, split = blockIdx.z;
    const int kbeg = split * g.kchunks * BK, kend = min(d.K, kbeg + g.kchunks * BK);
    const int nkt = (kend - kbeg) / 64;                    // >= 2 (launch site)
    const int nkt2 = (nkt + 1) & ~1;                       // the loop runs whole pairs: an odd count gets one K-tile of zeros
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // (scalar: LDS-DMA bases live in SGPRs)
    const int wr = wave >> 2, wc = wave & 3, r = lane & 31, hk = lane >> 5;

    // per-thread source offsets (bytes) of the two LDS-DMA instructions of each half-tile, swizzled
    unsigned offA[2][2], offB[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int s = i * 512 + tid;
            if constexpr (KM) {                            // LDS slot s: k-row kr, chunk s & 15 holds logical chunk ch (8 columns)
                const int kr = s >> 4, ch = (s & 15) ^ ((kr & 3) << 2);
                offA[h][i] = (unsigned)((kr * lda + (ch >> 3) * 128 + h * 64 + (ch & 7) * 8) * 2);
                offB[h][i] = (unsigned)((kr * ldb + (ch >> 3) * 128 + h * 64 + (ch & 7) * 8) * 2);
            } else {
                const int hr = s >> 3, gc = (s & 7) ^ ((hr >> 1) & 7);
                offA[h][i] = (unsigned)((((hr >> 6) * 128 + h * 64 + (hr & 63)) * lda + gc * 8) * 2);
                offB[h][i] = (unsigned)((((hr >> 5) * 64 + h * 32 + (hr & 31)) * ldb + gc * 8) * 2);
            }
        }
    // CONV_A: A16 holds the frames X[M][C] (lda = C) and the operand is their implicit im2col: K-tile k0 lies inside tap
    // dk = k0 / C (C % 64 == 0), so its rows are the frame rows shifted by dk - pad; a row that leaves its utterance gets
    // an offset past the buffer's range, which the LDS-DMA fills with zeros.
    const ConvAddr cva{d.conv_T, d.conv_C, d.conv_pad};
    int tposA[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int hr = (i * 512 + tid) >> 3;
            tposA[h][i] = CONV_A ? (m0 + (hr >> 6) * 128 + h * 64 + (hr & 63)) % cva.T : 0;
        }
    int cdk[2], cka[2];                                    // tap and channel offset of the next K-tile of A half 0 / 1
    cdk[0] = cdk[1] = CONV_A ? kbeg / cva.C : 0;
    cka[0] = cka[1] = CONV_A ? kbeg % cva.C : 0;
    // CONV_B: tap of this workgroup's columns, its first channel, and the position in its utterance of the k-row each
    // LDS-DMA instruction of B half 0 / 1 fetches next (k-row i * 32 + tid / 16 of the K-tile; 64 further per K-tile)
    const int bdk = CONV_B ? n0 / cva.C : 0, bshift = bdk - cva.pad, bstep = CONV_B ? 64 % cva.T : 0;
    int tposB[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i) tposB[h][i] = CONV_B ? (kbeg + i * 32 + (tid >> 4)) % cva.T : 0;
    // KM: the buffers span the split's k-rows of the tile's 256 columns, the K-tile is the scalar offset
    const long krange = nkt * 64 - 1;
    auto rsA = CONV_A ? __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(A16), 0, (int)((long)d.M * lda * 2), 0x00020000)
               : KM   ? __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(A16 + (long)kbeg * lda + m0), 0, (int)((krange * lda + 256) * 2), 0x00020000)
                      : __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(A16 + (long)m0 * lda + kbeg), 0, (int)(256 * lda * 2), 0x00020000);
    auto rsB = CONV_B ? __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(B16 + (long)(kbeg + bshift) * ldb + (n0 - bdk * cva.C)), 0, (int)((krange * ldb + 256) * 2), 0x00020000)
               : KM   ? __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(B16 + (long)kbeg * ldb + n0), 0, (int)((krange * ldb + 256) * 2), 0x00020000)
                      : __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(B16 + (long)n0 * ldb + kbeg), 0, (int)(256 * ldb * 2), 0x00020000);
    const int ktA = KM ? (int)(lda * 128) : 128, ktB = KM ? (int)(ldb * 128) : 128;        // bytes from one K-tile to the next
    // half-tile ht (0: A0, 1: A1, 2: B0, 3: B1) of K-tile kt -> LDS slot (kt & 1, ht); the calls of one half come in kt order
    auto stage = [&](int ht, int kt) {
        unsigned char* dst = smem16 + (((kt & 1) * 4 + ht) << 14) + wave * 1024;
        const bool live = kt < nkt;                        // (the padding K-tile of an odd count: offsets past the range read zeros)
        if (ht < 2) {
            if constexpr (CONV_A) {
                const int shift = cdk[ht] - cva.pad;
                const unsigned rel = (unsigned)(((long)(m0 + shift) * lda + cka[ht]) * 2);      // (wraps for m0 + shift < 0: those rows are masked)
                const unsigned o0 = live && (unsigned)(tposA[ht][0] + shift) < (unsigned)cva.T ? offA[ht][0] + rel : 0x80000000u;
                const unsigned o1 = live && (unsigned)(tposA[ht][1] + shift) < (unsigned)cva.T ? offA[ht][1] + rel : 0x80000000u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr)dst, 16, o0, 0, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr)(dst + 8192), 16, o1, 0, 0, 0);
                cka[ht] += 64;
                if (cka[ht] == cva.C) { cka[ht] = 0; ++cdk[ht]; }
            } else {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr)dst, 16, live ? offA[ht][0] : 0x80000000u, kt * ktA, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr)(dst + 8192), 16, live ? offA[ht][1] : 0x80000000u, kt * ktA, 0, 0);
            }
        } else if constexpr (CONV_B) {
            int (&tp)[2] = tposB[ht - 2];
            const unsigned o0 = live && (unsigned)(tp[0] + bshift) < (unsigned)cva.T ? offB[ht - 2][0] : 0x80000000u;
            const unsigned o1 = live && (unsigned)(tp[1] + bshift) < (unsigned)cva.T ? offB[ht - 2][1] : 0x80000000u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr)dst, 16, o0, kt * ktB, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr)(dst + 8192), 16, o1, kt * ktB, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i) { tp[i] += bstep; if (tp[i] >= cva.T) tp[i] -= cva.T; }
        } else {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr)dst, 16, live ? offB[ht - 2][0] : 0x80000000u, kt * ktB, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr)(dst + 8192), 16, live ? offB[ht - 2][1] : 0x80000000u, kt * ktB, 0, 0);
        }
    };
    // fragment addresses inside a half-tile: row hr, 16-byte chunk c at hr * 128 + ((c ^ ((hr >> 1) & 7)) << 4)
    const int sw = (r >> 1) & 7;
    unsigned cofs[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) cofs[ks] = (unsigned)(((2 * ks + hk) ^ sw) << 4);
    const unsigned rowA = (unsigned)((wr * 64 + r) * 128), rowB = (unsigned)((wc * 32 + r) * 128);
    // KM: lane 4q + p of 16-lane group (hk, gc) gives the address of k-row 8 hk + q (+ 16 ks + 4 u as an immediate), columns
    // 16 gc + 4 p .. + 3 of the MFMA tile, and receives column 16 gc + 4 q + p = r
    const int tq = (lane >> 2) & 3, tp = lane & 3, tgc = (lane >> 4) & 1;
    auto tr_addr = [&](int chunk0) { return (unsigned)(256 * (8 * hk + tq) + 16 * ((chunk0 + 2 * tgc + (tp >> 1)) ^ (tq << 2)) + 8 * (tp & 1)); };
    const unsigned trA[2] = {tr_addr(wr * 8), tr_addr(wr * 8 + 4)}, trB = tr_addr(wc * 4);
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem16;
    auto read_tr = [&](bf16x8 (&f)[4], unsigned addr) {
        f[0] = lds_read_tr16<0>(addr); f[1] = lds_read_tr16<4096>(addr); f[2] = lds_read_tr16<8192>(addr); f[3] = lds_read_tr16<12288>(addr);
    };

    f32x16 acc[4][2];
    zero(acc);
    bf16x8 Af[2][4], Bf[2][4];

    auto read_a = [&](int buf, int h) {
        const unsigned char* base = smem16 + ((buf * 4 + h) << 14);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if constexpr (KM) read_tr(Af[i], lds0 + ((buf * 4 + h) << 14) + trA[i]);
            else
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) Af[i][ks] = *reinterpret_cast<const bf16x8*>(base + rowA + i * 4096 + cofs[ks]);
        }
    };
    auto read_b = [&](int buf, int h) {
        const unsigned char* base = smem16 + ((buf * 4 + 2 + h) << 14);
        if constexpr (KM) read_tr(Bf[h], lds0 + ((buf * 4 + 2 + h) << 14) + trB);
        else
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) Bf[h][ks] = *reinterpret_cast<const bf16x8*>(base + rowB + cofs[ks]);
    };
    auto mma = [&](int a, int b) {
        __builtin_amdgcn_s_setprio(1);
        // KM: whatever a phase reads (B: 8 reads; A: 16; both: 24, B first), the fragments of step ks are complete once at
        // most 6 - 2 ks reads are outstanding (LDS reads return in order and the loop issues no other LDS operation; a
        // scalar load still in flight only makes the count conservative)
        if constexpr (KM) {
            lds_tr_wait<6>(Af[0][0], Af[1][0], Bf[b][0]);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[a * 2 + i][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Af[i][0], Bf[b][0], acc[a * 2 + i][b], 0, 0, 0);
            lds_tr_wait<4>(Af[0][1], Af[1][1], Bf[b][1]);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[a * 2 + i][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Af[i][1], Bf[b][1], acc[a * 2 + i][b], 0, 0, 0);
            lds_tr_wait<2>(Af[0][2], Af[1][2], Bf[b][2]);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[a * 2 + i][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Af[i][2], Bf[b][2], acc[a * 2 + i][b], 0, 0, 0);
            lds_tr_wait<0>(Af[0][3], Af[1][3], Bf[b][3]);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[a * 2 + i][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Af[i][3], Bf[b][3], acc[a * 2 + i][b], 0, 0, 0);
        } else
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[a * 2 + i][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Af[i][ks], Bf[b][ks], acc[a * 2 + i][b], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };
#define T2_G256_WAIT(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
    // one K-tile (buffer BUF): TAIL 0 = steady state, 1 = K-tile nkt-2, 2 = K-tile nkt-1
    auto ktile = [&](auto bufc, auto tailc, int kt) {
        constexpr int BUF = decltype(bufc)::value, TAIL = decltype(tailc)::value;
        // phase 0
        read_b(BUF, 0);
        __builtin_amdgcn_sched_barrier(0);
        read_a(BUF, 0);
        if (TAIL < 2) { stage(3, kt + 1); T2_G256_WAIT(8); } else T2_G256_WAIT(2);
        __builtin_amdgcn_s_barrier();
        mma(0, 0);
        __builtin_amdgcn_s_barrier();
        // phase 1
        read_b(BUF, 1);
        if (TAIL < 2) { stage(1, kt + 1); T2_G256_WAIT(8); } else T2_G256_WAIT(0);
        __builtin_amdgcn_s_barrier();
        mma(0, 1);
        __builtin_amdgcn_s_barrier();
        // phase 2
        read_a(BUF, 1);
        if (TAIL == 0) { stage(0, kt + 2); T2_G256_WAIT(8); }
        __builtin_amdgcn_s_barrier();
        mma(1, 1);
        __builtin_amdgcn_s_barrier();
        // phase 3
        if (TAIL == 0) { stage(2, kt + 2); T2_G256_WAIT(8); } else if (TAIL == 1) T2_G256_WAIT(4);
        __builtin_amdgcn_s_barrier();
        mma(1, 0);
        __builtin_amdgcn_s_barrier();
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;

    // prologue: K-tile 0 and A0, B0 of K-tile 1
    stage(0, 0); stage(2, 0); stage(3, 0); stage(1, 0); stage(0, 1); stage(2, 1);
    T2_G256_WAIT(8);
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();
    int kt = 0;
    for (; kt + 2 < nkt2; kt += 2) { ktile(I0{}, I0{}, kt); ktile(I1{}, I0{}, kt + 1); }
    ktile(I0{}, I1{}, kt);
    ktile(I1{}, I2{}, kt + 1);
    if (wr == 0) __builtin_amdgcn_s_barrier();
#undef T2_G256_WAIT

    // Epilogue through LDS (free now): each wave lays 64 rows x 64 columns of its sub-tile out row-major in its own
    // 16 KB and walks it with 16-byte reads, so a row leaves as 256 contiguous bytes and the per-row work (row map,
    // dropout index base) is done once per 4 elements.  This is the walk of store_rows_lds (gemm_common.h) written out
    // for whole tiles: through the shared helper the K-contiguous variant measured 1 % slower (profiles/README.md, round 19).
    const RngKey key = rng_key(d.seed, d.site);
    float* ws = d.splitk > 1 ? d.ws + (long)split * (long)d.M * d.N : nullptr;
    float* stg = reinterpret_cast<float*>(smem16) + wave * 4096;
    const bool vec_ok = ws || ((reinterpret_cast<uintptr_t>(d.C) & 15) == 0 && d.ldc % 4 == 0 && !d.ccol_mod);
    const float inv_keep = d.drop_p > 0.f ? 1.0f / (1.0f - d.drop_p) : 1.0f;
    // (KM: wave column wc owns columns (wc >> 1) * 128 + j * 64 + (wc & 1) * 32 + r, so that a B half-tile's k-rows are whole
    // 128-byte lines in memory like the A half-tile's)
    const int c4 = (lane & 15) * 4, n = n0 + (KM ? (wc >> 1) * 128 + (c4 >> 5) * 64 + (wc & 1) * 32 + (c4 & 31) : wc * 64 + c4);
    f32x4 bias = {0.f, 0.f, 0.f, 0.f}, r1n = {0.f, 0.f, 0.f, 0.f};
    if (!ws) {
#pragma unroll
        for (int c = 0; c < 4; ++c) bias[c] = (d.bias1 ? d.bias1[n + c] : 0.f) + (d.bias2 ? d.bias2[n + c] : 0.f);
        if (d.r1_m) {
#pragma unroll
            for (int c = 0; c < 4; ++c) r1n[c] = d.r1_n[n + c];
        }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) stg[(ii * 32 + (e & 3) + 8 * (e >> 2) + 4 * hk) * 64 + j * 32 + r] = acc[2 * p + ii][j][e];
        __syncthreads();
        for (int it = 0; it < 16; ++it) {
            const int row = it * 4 + (lane >> 4);
            const int m = m0 + wr * 128 + p * 64 + row;
            f32x4 v = *reinterpret_cast<const f32x4*>(stg + row * 64 + c4);
            if (ws) { *reinterpret_cast<f32x4*>(ws + (long)m * d.N + n) = v; continue; }
            const uint32_t ibase = d.drop_base + (uint32_t)m * d.drop_mstride + (uint32_t)n;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float x = apply_act(d.alpha * v[c] + bias[c], d.act);
                if (d.drop_p > 0.f) x = rng_keep(key, ibase + c, d.drop_p) ? x * inv_keep : 0.f;
                v[c] = x;
            }
            if (d.r1_m) {
                const float r1m = d.r1_m[m];
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = add_rank1(v[c], r1m, r1n[c]);
            }
            float* pr = d.C + out_row(d, m) * d.ldc;
            if (vec_ok) {
                float* pc = pr + n;
                if (d.beta != 0.f) v += d.beta * *reinterpret_cast<const f32x4*>(pc);
                *reinterpret_cast<f32x4*>(pc) = v;
            } else {
                with_col_map(d, [&](auto cmap) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        float* pc = pr + out_col<decltype(cmap)::value>(d, n + c);
                        *pc = d.beta != 0.f ? v[c] + d.beta * *pc : v[c];
                    }
                });
            }
        }
        if (p == 0) __syncthreads();
    }
}

template <bool CONV_A, bool KM, bool CONV_B>
int launch_bf16src256(const GemmK& g, const __bf16* pa, long lda, const __bf16* pb, long ldb, dim3 grid, hipStream_t s) {
    constexpr size_t smem = 128 * 1024;
    T2_TRY_RC(t2_allow_dynamic_lds(reinterpret_cast<const void*>(gemm_bf16src256_kernel<CONV_A, KM, CONV_B>), smem));
    GemmK gk = g;
    gk.xcd_swizzle = (grid.x * grid.y) % 8 == 0 && grid.y >= 4;
    hipLaunchKernelGGL((gemm_bf16src256_kernel<CONV_A, KM, CONV_B>), grid, dim3(512), smem, s, gk, pa, lda, pb, ldb);
    T2_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// staging casts: fp32 operand -> bf16 [rows][K] (K contiguous, leading dimension K), or (SPLIT) its hi / lo parts.
//
// split-bf16 staging (precision mode 2): x = hi + lo with hi = RN-bf16(x), lo = RN-bf16(x - hi) (the subtraction is exact
// in fp32), and x.w ~ hi.hi + lo.hi + hi.lo.  The three terms become ONE product of the bf16-source kernels with K' = 3K:
// per 64-wide K-tile j the staged A holds the tiles (hi_j lo_j hi_j) and the staged B (hi_j hi_j lo_j), so the small terms
// are accumulated (fp32) right next to their large term and the repeated hi tile is an L2 hit.  lo_slot names the slot
// (1: A, 2: B) that takes lo.
//   row_group == 0: K-concatenation, dst[row][3K]: source column k of term t at (k / 64) * 192 + t * 64 + k % 64
//   row_group  > 0: the k-major copies, dst[3 rows][K]: source row r of term t at row (r / G) * 3G + t * G + r % G
//                   (G = 64: K-tile interleave; G = rows: three whole copies, which the implicit-conv B operand of the
//                   k-major route needs: its kernel shifts k-rows per tap inside an utterance)
// ---------------------------------------------------------------------------------------------
// (an |x| above 3.39e38 rounds to a bf16 infinity, so its lo part is the opposite infinity and the product NaN where the
// exact kernel stays finite: the last 0.4 % of the fp32 range is outside this mode's contract, infinities as in fp32 give NaN/inf)
__device__ __forceinline__ void split8(const f32x4& lo4, const f32x4& hi4, bf16x8& h, bf16x8& l) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = j < 4 ? lo4[j] : hi4[j - 4];
        const __bf16 xh = (__bf16)x;
        h[j] = xh; l[j] = (__bf16)(x - (float)xh);
    }
}
// 8 consecutive k as one 16-byte store (plain cast), or as three of them `step` elements apart (SPLIT)
template <bool SPLIT>
__device__ __forceinline__ void store_cast8(__bf16* o, long step, int lo_slot, const f32x4& lo4, const f32x4& hi4) {
    if constexpr (SPLIT) {
        bf16x8 h, l;
        split8(lo4, hi4, h, l);
#pragma unroll
        for (int slot = 0; slot < 3; ++slot) *reinterpret_cast<bf16x8*>(o + slot * step) = slot == lo_slot ? l : h;
    } else {
        *reinterpret_cast<bf16x8*>(o) = pack8(lo4, hi4);
    }
}
// source contiguous along K (src[row * ld + k]): 8 elements per task
template <bool SPLIT>
__global__ void stage_kc_kernel(const float* __restrict__ src, long ld, __bf16* __restrict__ dst, int rows, int K, int lo_slot, int row_group) {
    const int k8 = K >> 3;
    const long total = (long)rows * k8;
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const long row = t / k8; const int k = (int)(t - row * k8) * 8;
        const float* p = src + row * ld + k;
        const f32x4 lo4 = *reinterpret_cast<const f32x4*>(p), hi4 = *reinterpret_cast<const f32x4*>(p + 4);
        if constexpr (SPLIT) {
            long o, step;
            if (row_group) { o = ((row / row_group) * 3 * row_group + row % row_group) * (long)K + k; step = (long)row_group * K; }
            else { o = row * 3 * (long)K + (k >> 6) * 192 + (k & 63); step = 64; }
            store_cast8<true>(dst + o, step, lo_slot, lo4, hi4);
        } else {
            store_cast8<false>(dst + row * (long)K + k, 0, 0, lo4, hi4);
        }
    }
}
// source contiguous along the rows (src[k * ld + row]) -> dst[row][K] (SPLIT: dst[row][3K]): 64 k x 64 rows per workgroup
// through LDS
template <bool SPLIT>
__global__ __launch_bounds__(256) void stage_mc_kernel(const float* __restrict__ src, long ld, __bf16* __restrict__ dst, int rows, int K, int lo_slot) {
    __shared__ float tile[64][65];
    const int r0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = (threadIdx.x >> 4) + 16 * i, r4 = (threadIdx.x & 15) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + (long)(k0 + k) * ld + r0 + r4);
#pragma unroll
        for (int j = 0; j < 4; ++j) tile[k][r4 + j] = v[j];
    }
    __syncthreads();
    constexpr int T = SPLIT ? 3 : 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int kg = threadIdx.x & 7, row = (threadIdx.x >> 3) + 32 * i;
        f32x4 a, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = tile[kg * 8 + j][row]; b[j] = tile[kg * 8 + 4 + j][row]; }
        store_cast8<SPLIT>(dst + (long)(r0 + row) * T * K + T * (long)k0 + kg * 8, 64, lo_slot, a, b);
    }
}

// kc: the source is contiguous along its second index; lo_slot, row_group: split copies only (row_group 0 with !kc)
int launch_stage(const float* src, bool kc, long ld, __bf16* dst, int rows, int K, bool split, int lo_slot, int row_group, hipStream_t s) {
    if (kc) {
        long blocks = ((long)rows * (K >> 3) + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(split ? stage_kc_kernel<true> : stage_kc_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, src, ld, dst, rows, K, lo_slot, row_group);
    } else {
        hipLaunchKernelGGL(split ? stage_mc_kernel<true> : stage_mc_kernel<false>, dim3(rows / 64, K / 64), dim3(256), 0, s, src, ld, dst, rows, K, lo_slot);
    }
    T2_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int launch_gemm_bf16src(const GemmK& g, GemmKernel kernel, const __bf16* pa, long lda, const __bf16* pb, long ldb, dim3 grid, hipStream_t s) {
    const GemmDesc& d = g.d;
    // 128x128 block tile, two k-steps in flight.  Measured alternatives (same template, other parameters): 256x128 with
    // 8 waves 5-12 % slower, 256x256 with 128x64 wave tiles and one k-step in flight 4.6x slower (one workgroup per CU:
    // nothing overlaps its barriers) — the kernel is bound by latency hiding, not by operand bytes per CU
    if (kernel == GemmKernel::src256km && d.conv_b) return launch_bf16src256<false, true, true>(g, pa, lda, pb, ldb, grid, s);
    if (kernel == GemmKernel::src256km) return launch_bf16src256<false, true, false>(g, pa, lda, pb, ldb, grid, s);
    if (kernel == GemmKernel::src256 && d.conv_a) return launch_bf16src256<true, false, false>(g, pa, lda, pb, ldb, grid, s);
    if (kernel == GemmKernel::src256) return launch_bf16src256<false, false, false>(g, pa, lda, pb, ldb, grid, s);
    if (d.conv_a) return launch_bf16src<true>(g, pa, lda, pb, ldb, grid, s);
    return launch_bf16src<false>(g, pa, lda, pb, ldb, grid, s);
}

}  // namespace gemm_detail

using gemm_detail::aligned16;

int stage_bf16(const float* src, bool kc, long ld, __bf16* dst, int rows, int K, hipStream_t s) {
    T2_REQUIRE(rows > 0 && K > 0 && rows % 64 == 0 && K % 64 == 0 && ld % 4 == 0 && aligned16(src) && aligned16(dst),
               "stage_bf16: rows=%d K=%d ld=%ld must be whole 64-tiles of 16-byte aligned rows", rows, K, ld);
    return gemm_detail::launch_stage(src, kc, ld, dst, rows, K, false, 0, 0, s);
}

int stage_split_bf16(const float* src, bool kc, long ld, __bf16* dst, int rows, int K, int lo_slot, int row_group, hipStream_t s) {
    T2_REQUIRE(rows > 0 && K > 0 && rows % 64 == 0 && K % 64 == 0 && ld % 4 == 0 && aligned16(src) && aligned16(dst) &&
               (lo_slot == 1 || lo_slot == 2) && row_group >= 0 && (!row_group || (kc && rows % row_group == 0)),
               "stage_split_bf16: rows=%d K=%d ld=%ld must be whole 64-tiles of 16-byte aligned rows", rows, K, ld);
    return gemm_detail::launch_stage(src, kc, ld, dst, rows, K, true, lo_slot, row_group, s);
}

int stage_planned(const float* src, const GemmOperandPlan& o, bool split, __bf16* dst, hipStream_t s) {
    return gemm_detail::launch_stage(src, o.kc, o.ld_src, dst, o.rows, o.K, split, o.lo_slot, o.row_group, s);
}

}  // namespace t2
