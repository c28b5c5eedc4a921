// Log-mel front end: ragged waveforms to log-mel spectrograms in one kernel.  Replaces the reference's layers.py:
// TacotronSTFT.mel_spectrogram (:60-80) with stft.py: STFT.transform (:77-105) and audio_processing.py:
// dynamic_range_compression (:78-84), and the torch.stft(center=False) form of utils.py: mel_spectrogram (:73-79).
//
//   out[b][m][f] = log(max(clip, sum_bin melb[m][bin] * sqrt(re^2 + im^2 + mag_eps)) * C),
//   (re, im)[bin][f] = sum_k basis[.][k] * xpad_b[f*hop + k],  xpad_b = item b reflect-padded by `pad` samples per side.
//
// The shape is stft_analysis_kernel's: a workgroup of 4 waves owns 32 frames of one item, the loader reads the waveform
// itself (reflect padding is index arithmetic on the item's own length), the forward table is t2_stft_pack's.  A pass
// forms re and im of 4 x 16 bins over K = N; its epilogue writes the 64 x 32 magnitudes into a second LDS slab instead of
// memory, and wave w then multiplies mel rows 32w .. 32w+31 with them on the matrix cores, from a mel table packed in
// consumption order.  Arithmetic is exact fp32 (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain), whatever
// t2_set_precision says.
//
// Order of the mel sum, independent of the launch shape: each pass accumulates a partial from zero over its 64 bins in
// ascending order, and  total = total + partial  in ascending pass order, a separate rounded add.  With few frame tiles the
// passes are split over blockIdx.y into contiguous ranges: every pass partial then goes to scratch [passes][B][nf][n_mels]
// and melspec_finish_kernel does the same adds in the same order, so the bits are those of the unsplit launch.
// Frames past an item's own count are written as pad_value.  Offsets are 64-bit.
#include "kernels.h"

namespace t2 {

constexpr int kMelMaxMels = 128;                 // four waves x 32 mel rows
constexpr int kMelPassBins = 64;                 // bins whose magnitudes one pass holds in LDS: four waves x 16
// Measured (profiles/README.md "Log-mel front end"): a frame tile alone on its CU takes 0.30 ms at 1024/513, and every launch
// of fewer than 3 workgroups per CU ran faster with its passes split, fastest with one pass per workgroup (an uneven split,
// 7 ranges over 9 passes, was slower than 3 even ones).
constexpr int kMelSplitBelow = 768;              // frame tiles x B below which every pass gets a workgroup of its own
// Sizes in floats; the packed buffer is [forward (stft_pack_forward's order) | mel].
struct MelPlan { int cutoff, bin_tiles, kchunks, passes, row_tiles, splits; long nf_max, frame_tiles; size_t fwd_floats, mel_floats, split_scratch_floats; };
// The backward of the log-mel front end with respect to the samples.  Two tables beside the forward's: the mel
// basis in the order the transposed product consumes it, and the forward basis in the synthesis kernel's order.
// Workspace, in floats: [d_re | d_im : B * bins * nf_max each][dxpad : B * (n + 2*pad)].
struct MelGradPlan {
    int cutoff, bin_tiles, kchunks, passes, row_tiles, overlap, col_tiles, wave_cols; long nf_max, frame_tiles, q_tiles;
    size_t melt_floats, basis_floats, dz_floats, dxpad_floats;
};

constexpr int kMelKC = 32;                                    // k per slab, as the analysis kernel
constexpr int kMelSlabStride = kStftTile + 1;                 // odd: the loader's lanes run along k, one bank each
constexpr int kMelMagStride = kStftTile + 1;
constexpr int kMelSlabFloats = kMelKC * kMelSlabStride;
constexpr int kMelLdsFloats = kMelSlabFloats + kMelPassBins * kMelMagStride;
constexpr int kMelStageStride = 65;                           // [32 frames][64 mel rows], odd stride
static_assert(kStftTile * kMelStageStride <= kMelLdsFloats, "the store staging reuses the two slabs");
static_assert(kMelLdsFloats * sizeof(float) < 16 * 1024, "under 16 KB of LDS");

struct MelSpec {
    const float* x; const int* lengths; const f32x4* pf; const f32x4* pm; float* out; float* scratch; int* frame_lengths;
    long n, nf_max;
    int B, N, hop, pad, cutoff, bin_tiles, kchunks, passes, n_mels, row_tiles, splits, time_major, power;
    float mag_eps, clip, C, pad_value;
    float* sums;                                               // nullable: the mel sum [B][nf_max][n_mels] kept for the backward
};

struct MelChunk { float x[4]; f32x4 a[4]; int live; };   // what a thread holds of one chunk: 4 samples for the slab (bit i of live: sample i counts), 16 table values

// the item's own length, clamped to the row
__device__ __forceinline__ long mel_item_len(const MelSpec& p, int b) {
    if (!p.lengths) return p.n;
    const long l = p.lengths[b];
    return l < 0 ? 0 : (l > p.n ? p.n : l);
}

// torch.log(torch.clamp(x, min=clip) * C); the power mode (tests) returns the mel sum itself
__device__ __forceinline__ float mel_finish(const MelSpec& p, float total) {
    return p.power ? total : logf(__fmul_rn(fmaxf(total, p.clip), p.C));
}

// A wave's 32 x 32 tile v (lane: frame lane & 31; element e: mel row 32*wave + (e&3) + 8*(e>>2) + 4*(lane>>5)) to time-major
// memory dst[frame][n_mels], dst at the tile's first frame, through LDS so that 64 lanes run along the mel axis.  Frames
// below `live` get the values, frames from `live` to `limit` get `fill`.  Every thread of the workgroup calls it.
__device__ __forceinline__ void mel_store_time_major(float* lds, const f32x16& v, float* dst, int n_mels, int row_tiles, long live, long limit, float fill) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hk = lane >> 5;
    for (int r = 0; 2 * r < row_tiles; ++r) {
        __syncthreads();                                       // whoever read the LDS before is done
        if ((wave >> 1) == r) {
#pragma unroll
            for (int e = 0; e < 16; ++e) lds[(lane & 31) * kMelStageStride + 32 * (wave & 1) + (e & 3) + 8 * (e >> 2) + 4 * hk] = v[e];
        }
        __syncthreads();
        const int m = 64 * r + lane;
        if (m < n_mels) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int fl = wave + 4 * i;
                if (fl < limit) dst[(size_t)fl * n_mels + m] = fl < live ? lds[fl * kMelStageStride + lane] : fill;
            }
        }
    }
}

// three waves per SIMD: 160 registers with the accumulators among them (149 before the optional store of the mel sum) instead of
// 154 + 16 (two waves), still nothing spilled
__global__ void __launch_bounds__(256, 3) melspec_kernel(MelSpec p) {
    __shared__ float lds[kMelLdsFloats];
    float* slab = lds;
    float* mags = lds + kMelSlabFloats;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hk = lane >> 5;
    const int b = blockIdx.z;
    const long f0 = (long)blockIdx.x * kStftTile;
    const long ilen = mel_item_len(p, b);
    const long nf = mel_frames(ilen, p.N, p.hop, p.pad);
    if (p.frame_lengths && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.frame_lengths[b] = (int)nf;
    const long limit = p.nf_max - f0 < kStftTile ? p.nf_max - f0 : kStftTile;   // frames of this tile inside out
    if (f0 >= nf) {                                            // uniform over the workgroup: nothing but padding here
        if (p.splits > 1) return;                              // the finishing kernel writes out
        for (int idx = threadIdx.x; idx < kStftTile * p.n_mels; idx += 256) {
            const int fl = p.time_major ? idx / p.n_mels : idx % kStftTile, m = p.time_major ? idx % p.n_mels : idx / kStftTile;
            if (fl >= limit) continue;
            const size_t o = p.time_major ? ((size_t)b * p.nf_max + f0 + fl) * p.n_mels + m : ((size_t)b * p.n_mels + m) * p.nf_max + f0 + fl;
            p.out[o] = p.pad_value;
        }
        return;
    }
    const float* xb = p.x + (size_t)b * p.n;
    const int ps0 = (int)((long)blockIdx.y * p.passes / p.splits), ps1 = (int)((long)(blockIdx.y + 1) * p.passes / p.splits);
    f32x16 total = {0}, acc = {0};
    // The samples and the table rows of a chunk are requested one chunk ahead, so that their latency passes under the 16 MFMAs
    // of the chunk before (a workgroup is alone on its CU when there are few tiles).  Two register sets by name, used in turn:
    // a copy from "next" to "current" would wait for the loads.
    const int kl = threadIdx.x & 31, fl0 = threadIdx.x >> 5;
    auto fetch = [&](MelChunk& r, int ps, int c) {
        const int k = c * kMelKC + kl;
        r.live = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long f = f0 + fl0 + 8 * i;
            long t = f * p.hop + k - p.pad;                    // reflect padding: ilen > pad keeps both mirrors inside [0, ilen)
            if (t < 0) t = -t;
            else if (t >= ilen) t = 2 * (ilen - 1) - t;
            const bool live = f < nf && k < p.N;               // a dead element loads sample 0, dropped when the slab is written:
            r.x[i] = xb[live ? t : 0];                         // no branch around the load, and nothing here waits for it
            r.live |= (int)live << i;
        }
        const int mt = ps * 4 + wave;
        const f32x4* pf = p.pf + ((size_t)(mt < p.bin_tiles ? mt : 0) * p.kchunks + c) * 256 + lane;   // an idle wave loads tile 0 and drops it
#pragma unroll
        for (int g = 0; g < 4; ++g) r.a[g] = pf[g * 64];
    };
    // one chunk of one pass: stage cur, request nxt, multiply; after a pass's last chunk, its magnitudes and mel partial
    auto step = [&](const MelChunk& cur, MelChunk& nxt, int ps, int c) {
        if (c || ps != ps0) __syncthreads();                   // every wave is done with the previous slab, magnitudes and staging
#pragma unroll
        for (int i = 0; i < 4; ++i) slab[kl * kMelSlabStride + fl0 + 8 * i] = (cur.live >> i & 1) ? cur.x[i] : 0.f;
        __syncthreads();
        const bool last = c + 1 == p.kchunks, more = !last || ps + 1 < ps1;
        // always, so that the compiler's count of loads in flight is the same on every path: the final step requests its own
        // chunk again and nobody reads it
        fetch(nxt, more && last ? ps + 1 : ps, more ? (last ? 0 : c + 1) : c);
        const int mt = ps * 4 + wave;
        if (mt < p.bin_tiles) {                                // uniform over the wave
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[g][i], slab[(8 * g + 2 * i + hk) * kMelSlabStride + (lane & 31)], acc, 0, 0, 0);
            }
        }
        if (!last) return;
        f32x4 ma[8];                                           // this wave's mel rows for the pass: on their way during the epilogue
        const f32x4* pm = p.pm + ((size_t)(wave < p.row_tiles ? wave : 0) * p.passes + ps) * 512 + lane;
#pragma unroll
        for (int g = 0; g < 8; ++g) ma[g] = pm[g * 64];
        // element e (bit 2 clear) is re, e + 4 is im of bin 16*mt + 8*(e>>3) + 4*hk + (e&3), frame lane & 31 (stft.hip)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int bl = 8 * h + 4 * hk + i;
                const float re = acc[8 * h + i], im = acc[8 * h + i + 4];
                const float pw = __fadd_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)), p.mag_eps);   // no contraction
                const float mg = p.power ? pw : sqrtf(pw);
                mags[(16 * wave + bl) * kMelMagStride + (lane & 31)] = mt * 16 + bl < p.cutoff ? mg : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        __syncthreads();
        f32x16 part = {0};
        if (wave < p.row_tiles) {
#pragma unroll
            for (int g = 0; g < 8; ++g) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    part = __builtin_amdgcn_mfma_f32_32x32x2f32(ma[g][i], mags[(8 * g + 2 * i + hk) * kMelMagStride + (lane & 31)], part, 0, 0, 0);
            }
        }
        if (p.splits == 1) {
#pragma clang fp contract(off)
            total = total + part;                              // one rounded add per pass, ascending
        } else {
            float* dst = p.scratch + (((size_t)ps * p.B + b) * p.nf_max + f0) * p.n_mels;
            mel_store_time_major(lds, part, dst, p.n_mels, p.row_tiles, nf - f0, nf - f0, 0.f);
        }
    };
    MelChunk ca, cb;
    fetch(ca, ps0, 0);
    for (int ps = ps0, c = 0; ps < ps1;) {
        step(ca, cb, ps, c);
        if (++c == p.kchunks) { c = 0; ++ps; }
        if (ps >= ps1) break;
        step(cb, ca, ps, c);
        if (++c == p.kchunks) { c = 0; ++ps; }
    }
    if (p.splits > 1) return;
    if (p.sums) mel_store_time_major(lds, total, p.sums + ((size_t)b * p.nf_max + f0) * p.n_mels, p.n_mels, p.row_tiles, nf - f0, nf - f0, 0.f);
#pragma unroll
    for (int e = 0; e < 16; ++e) total[e] = mel_finish(p, total[e]);
    if (p.time_major) {
        mel_store_time_major(lds, total, p.out + ((size_t)b * p.nf_max + f0) * p.n_mels, p.n_mels, p.row_tiles, nf - f0, limit, p.pad_value);
    } else if (wave < p.row_tiles && (lane & 31) < limit) {
        const long f = f0 + (lane & 31);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * hk;
            if (m < p.n_mels) p.out[((size_t)b * p.n_mels + m) * p.nf_max + f] = f < nf ? total[e] : p.pad_value;
        }
    }
}

// The split launch's second kernel: one thread per output element adds the pass partials in ascending order.
__global__ void __launch_bounds__(256) melspec_finish_kernel(MelSpec p, size_t count) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    const int m = (int)(idx % p.n_mels);
    const size_t bf = idx / p.n_mels;
    const long f = (long)(bf % p.nf_max);
    const int b = (int)(bf / p.nf_max);
    float v = p.pad_value;
    if (f < mel_frames(mel_item_len(p, b), p.N, p.hop, p.pad)) {
        const size_t plane = (size_t)p.B * p.nf_max * p.n_mels;
        float total = 0.f;
        for (int ps = 0; ps < p.passes; ++ps) {
#pragma clang fp contract(off)
            total = total + p.scratch[(size_t)ps * plane + idx];
        }
        v = mel_finish(p, total);
        if (p.sums) p.sums[idx] = total;
    }
    p.out[p.time_major ? idx : ((size_t)b * p.n_mels + m) * p.nf_max + f] = v;
}

// mel table:  [row_tile][pass][g][lane][i] = melb[32*row_tile + (lane & 31)][64*pass + 8*g + 2*i + (lane >> 5)], g < 8
__global__ void __launch_bounds__(256) melspec_pack_kernel(const float* __restrict__ melb, float* __restrict__ out, int n_mels, int cutoff, int passes, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int i = idx & 3, lane = (idx >> 2) & 63, g = (idx >> 8) & 7;
    const size_t rest = idx >> 11;
    const int ps = (int)(rest % passes), rt = (int)(rest / passes);
    const int row = 32 * rt + (lane & 31), bin = kMelPassBins * ps + 8 * g + 2 * i + (lane >> 5);
    out[idx] = (row < n_mels && bin < cutoff) ? melb[(size_t)row * cutoff + bin] : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------
static int melspec_plan(int N, int hop, int pad, int n_mels, long n, int B, MelPlan* out) {   // validates; no device
    T2_REQUIRE(out, "melspec: null plan");
    T2_REQUIRE(N >= 2 && N <= kStftMaxN, "melspec: filter_length=%d outside 2..%d", N, kStftMaxN);
    T2_REQUIRE(N % 2 == 0, "melspec: filter_length=%d is odd: the reflect padding takes N/2 samples per side", N);
    T2_REQUIRE(hop >= 1 && hop <= N, "melspec: hop_length=%d outside 1..filter_length=%d", hop, N);
    T2_REQUIRE(n_mels >= 1 && n_mels <= kMelMaxMels, "melspec: n_mels=%d outside 1..%d", n_mels, kMelMaxMels);
    T2_REQUIRE(pad >= 0 && pad <= N / 2, "melspec: pad=%d outside 0..filter_length/2=%d", pad, N / 2);
    T2_REQUIRE(B >= 1 && B <= 65535, "melspec: B=%d outside 1..65535", B);
    T2_REQUIRE(n >= 0 && n <= INT32_MAX / 2, "melspec: %ld samples per row outside 0..%d", n, INT32_MAX / 2);
    T2_REQUIRE(n + 2L * pad >= N, "melspec: n=%ld samples with pad=%d per side do not fill one frame of filter_length=%d", n, pad, N);
    MelPlan p;
    p.cutoff = N / 2 + 1;
    p.bin_tiles = (p.cutoff + 15) / 16;
    p.kchunks = (N + kMelKC - 1) / kMelKC;
    p.passes = (p.cutoff + kMelPassBins - 1) / kMelPassBins;
    p.row_tiles = (n_mels + 31) / 32;
    p.nf_max = (n + 2L * pad - N) / hop + 1;
    p.frame_tiles = (p.nf_max + kStftTile - 1) / kStftTile;
    T2_REQUIRE(p.frame_tiles <= INT32_MAX, "melspec: %ld frame tiles exceed the grid", p.frame_tiles);
    // Few workgroups: one 32-frame tile is passes * 4 bin tiles of N fp32 MFMAs on one CU, so a single utterance would sit at
    // that latency on a fraction of the 256 CUs.  Below kMelSplitBelow workgroups (three per CU) the passes spread over
    // blockIdx.y, one each.
    p.splits = p.frame_tiles * B < kMelSplitBelow ? p.passes : 1;
    p.fwd_floats = (size_t)p.bin_tiles * p.kchunks * 1024;
    p.mel_floats = (size_t)p.row_tiles * p.passes * 2048;
    p.split_scratch_floats = (size_t)p.passes * B * p.nf_max * n_mels;
    T2_REQUIRE((size_t)B * p.nf_max * n_mels <= (size_t)INT32_MAX * 256, "melspec: B=%d x %ld frames x n_mels=%d exceed the grid", B, p.nf_max, n_mels);
    *out = p;
    return 0;
}

// fwd: the windowed forward basis [2*(N/2+1)][N]; melb [n_mels][N/2+1]
static int melspec_pack(int N, int n_mels, const float* fwd, const float* melb, float* packed, hipStream_t s) {
    MelPlan pl;
    T2_TRY_RC(melspec_plan(N, N, N / 2, n_mels, N, 1, &pl));
    T2_REQUIRE(fwd && melb && packed, "melspec_pack: null pointer");
    T2_TRY_RC(stft_pack_forward(N, fwd, packed, s));
    hipLaunchKernelGGL(melspec_pack_kernel, dim3((unsigned)((pl.mel_floats + 255) / 256)), dim3(256), 0, s, melb, packed + pl.fwd_floats, n_mels, pl.cutoff, pl.passes,
                       pl.mel_floats);
    T2_LAUNCH_CHECK();
    return 0;
}

static int melspec(const t2_melspec_args& a, hipStream_t s) {
    MelPlan pl;
    T2_TRY_RC(melspec_plan(a.N, a.hop, a.pad, a.n_mels, a.n, a.B, &pl));
    T2_REQUIRE(a.x && a.packed && a.out, "melspec: null pointer");
    T2_REQUIRE(a.force_splits >= 0 && a.force_splits <= pl.passes, "melspec: force_splits=%d outside 0..passes=%d", a.force_splits, pl.passes);
    T2_REQUIRE(a.clip_val > 0.f && a.C > 0.f && a.mag_eps >= 0.f, "melspec: clip_val=%g and C=%g must be positive, mag_eps=%g not negative", a.clip_val, a.C, a.mag_eps);
    const int S = a.force_splits ? a.force_splits : pl.splits;
    T2_REQUIRE(S == 1 || (a.scratch && a.scratch_floats >= pl.split_scratch_floats), "melspec: %d splits need %zu floats of scratch, got %zu", S,
               pl.split_scratch_floats, a.scratch ? a.scratch_floats : (size_t)0);
    MelSpec p;
    p.x = a.x; p.lengths = a.lengths; p.pf = reinterpret_cast<const f32x4*>(a.packed); p.pm = reinterpret_cast<const f32x4*>(a.packed + pl.fwd_floats);
    p.out = a.out; p.scratch = a.scratch; p.frame_lengths = a.frame_lengths;
    p.n = a.n; p.nf_max = pl.nf_max;
    p.B = a.B; p.N = a.N; p.hop = a.hop; p.pad = a.pad; p.cutoff = pl.cutoff; p.bin_tiles = pl.bin_tiles; p.kchunks = pl.kchunks; p.passes = pl.passes;
    p.n_mels = a.n_mels; p.row_tiles = pl.row_tiles; p.splits = S; p.time_major = a.time_major != 0; p.power = a.return_power != 0;
    p.mag_eps = a.mag_eps; p.clip = a.clip_val; p.C = a.C; p.pad_value = a.pad_value;
    p.sums = a.mel_sum;
    hipLaunchKernelGGL(melspec_kernel, dim3((unsigned)pl.frame_tiles, (unsigned)S, (unsigned)a.B), dim3(256), 0, s, p);
    T2_LAUNCH_CHECK();
    if (S > 1) {
        const size_t count = (size_t)a.B * pl.nf_max * a.n_mels;
        hipLaunchKernelGGL(melspec_finish_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, p, count);
        T2_LAUNCH_CHECK();
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// backward with respect to the samples (layers.py:60-80, stft.py:77-105, utils.py:73-79 under torch autograd)
//
//   ds[m][f]  = g[m][f] / s[m][f]  where s >= clip, else 0          (s: the mel sum the forward kept)
//   dmag[bin] = sum_m melb[m][bin] * ds[m]
//   dz        = dmag * z / mag     where mag > 0, else exactly 0    (torch's sqrt gives 0 * inf = NaN there)
// A workgroup owns (32 frames, one pass of 64 bins, item).  Wave w recomputes re, im of bin tile 4*pass + w with the forward's
// table and chain, so z has the forward's bits and is never stored by it.  ds of every mel row is staged once in LDS, and
// the transposed mel product runs on the matrix cores from a table whose 32-row tile repeats each bin in its re and its im
// row: the wave's second accumulator then holds dmag of a bin in the very elements where the first holds its re and im.
// The k of that chain is the mel row, ascending.  dz goes to two planes [B][bins][nf_max]; stft_analysis_backward turns them
// into dx.  Frames at or behind the item's count are neither read nor written.
// ------------------------------------------------------------------------------------------------------------------
constexpr int kMelGradStride = kStftTile + 1;
constexpr int kMelGradLdsFloats = kMelMaxMels * kMelGradStride;   // ds [mel row][frame]; the recompute's slab uses its head before
static_assert(kMelKC * kMelSlabStride <= kMelGradLdsFloats, "the slab fits into the ds stage");

struct MelGrad {
    const float* x; const int* lengths; const f32x4* pf; const f32x4* pt; const float* sums; const float* g; float* d_re; float* d_im;
    long n, nf_max;
    int N, hop, pad, cutoff, bin_tiles, kchunks, n_mels, row_tiles, g_time_major;
    float mag_eps, clip;
};

__global__ void __launch_bounds__(256) melspec_grad_kernel(MelGrad p) {
    __shared__ float lds[kMelGradLdsFloats];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hk = lane >> 5;
    const int b = blockIdx.z;
    const long f0 = (long)blockIdx.x * kStftTile;
    long ilen = p.n;
    if (p.lengths) {
        const long l = p.lengths[b];
        ilen = l < 0 ? 0 : (l > p.n ? p.n : l);
    }
    const long nf = mel_frames(ilen, p.N, p.hop, p.pad);
    if (f0 >= nf) return;                                      // uniform over the workgroup: a tile behind the item's frames
    const int mt = blockIdx.y * 4 + wave;
    const bool active = mt < p.bin_tiles;                      // uniform over the wave
    const float* xb = p.x + (size_t)b * p.n;
    const f32x4* pf = p.pf + (size_t)(active ? mt : 0) * p.kchunks * 256;
    f32x16 acc = {0};
    for (int c = 0; c < p.kchunks; ++c) {
        if (c) __syncthreads();
        const int kl = threadIdx.x & 31, k = c * kMelKC + kl;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int fl = (threadIdx.x >> 5) + 8 * i;
            const long f = f0 + fl;
            float v = 0.f;
            if (f < nf && k < p.N) {
                long t = f * p.hop + k - p.pad;                // reflect padding: ilen > pad keeps both mirrors inside [0, ilen)
                if (t < 0) t = -t;
                else if (t >= ilen) t = 2 * (ilen - 1) - t;
                v = xb[t];
            }
            lds[kl * kMelSlabStride + fl] = v;
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 a = pf[(size_t)c * 256 + g * 64 + lane];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], lds[(8 * g + 2 * i + hk) * kMelSlabStride + (lane & 31)], acc, 0, 0, 0);
            }
        }
    }
    __syncthreads();                                           // the slab is read; ds takes its place
    const int rows = 32 * p.row_tiles;
    for (int idx = threadIdx.x; idx < rows * kStftTile; idx += 256) {
        const int m = idx % rows, fl = idx / rows;             // lanes along the mel row, as s lies in memory
        const long f = f0 + fl;
        float v = 0.f;
        if (m < p.n_mels && f < nf) {
            const size_t ot = ((size_t)b * p.nf_max + f) * p.n_mels + m;
            const float sv = p.sums[ot];
            if (sv >= p.clip) v = p.g[p.g_time_major ? ot : ((size_t)b * p.n_mels + m) * p.nf_max + f] / sv;   // torch.clamp's mask
        }
        lds[m * kMelGradStride + fl] = v;
    }
    __syncthreads();
    if (!active) return;
    f32x16 dm = {0};
    const f32x4* pt = p.pt + (size_t)mt * p.row_tiles * 256 + lane;
    for (int kc = 0; kc < p.row_tiles; ++kc) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 a = pt[(size_t)kc * 256 + g * 64];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                dm = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], lds[(32 * kc + 8 * g + 2 * i + hk) * kMelGradStride + (lane & 31)], dm, 0, 0, 0);
        }
    }
    const long f = f0 + (lane & 31);
    if (f >= nf) return;
    // element e (bit 2 clear) is re, e + 4 is im of bin 16*mt + 8*(e>>3) + 4*hk + (e&3); dm holds that bin's dmag in both
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int bin = mt * 16 + 8 * h + 4 * hk + i;
            if (bin >= p.cutoff) continue;
            const float re = acc[8 * h + i], im = acc[8 * h + i + 4], d = dm[8 * h + i];
            const float mg = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)), p.mag_eps));   // the forward's magnitude
            const size_t o = ((size_t)b * p.cutoff + bin) * p.nf_max + f;
            p.d_re[o] = mg > 0.f ? __fmul_rn(d, re / mg) : 0.f;
            p.d_im[o] = mg > 0.f ? __fmul_rn(d, im / mg) : 0.f;
        }
    }
}

// transposed mel table:  [bin_tile][row_tile][g][lane][i] = melb[32*row_tile + 8*g + 2*i + (lane >> 5)][bin],  tile row r = lane & 31:
//                        bin = 16*bin_tile + 8*(r>>4) + (r&7), whatever (r>>3)&1 says: the re row and the im row of a bin hold the same
__global__ void __launch_bounds__(256) melspec_pack_t_kernel(const float* __restrict__ melb, float* __restrict__ out, int n_mels, int cutoff, int row_tiles, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int i = idx & 3, lane = (idx >> 2) & 63, g = (idx >> 8) & 3;
    const size_t rest = idx >> 10;
    const int kc = (int)(rest % row_tiles), bt = (int)(rest / row_tiles);
    const int r = lane & 31, bin = bt * 16 + 8 * (r >> 4) + (r & 7), m = 32 * kc + 8 * g + 2 * i + (lane >> 5);
    out[idx] = (bin < cutoff && m < n_mels) ? melb[(size_t)m * cutoff + bin] : 0.f;
}

static int melspec_grad_plan(int N, int hop, int pad, int n_mels, long n, int B, MelGradPlan* out) {
    T2_REQUIRE(out, "melspec backward: null plan");
    MelPlan f;
    T2_TRY_RC(melspec_plan(N, hop, pad, n_mels, n, B, &f));
    T2_REQUIRE(N % hop == 0, "melspec backward: filter_length=%d is not a multiple of hop_length=%d: the overlap-add GEMM needs whole overlaps", N, hop);
    T2_REQUIRE(N / hop <= kStftMaxOverlap, "melspec backward: filter_length=%d over hop_length=%d is %d overlaps, at most %d", N, hop, N / hop, kStftMaxOverlap);
    T2_REQUIRE(f.nf_max <= INT32_MAX / 2 / hop, "melspec backward: %ld frames exceed the limit at hop_length=%d", f.nf_max, hop);
    StftPlan sp;
    T2_TRY_RC(stft_plan(N, hop, (int)f.nf_max, &sp));
    MelGradPlan p;
    p.cutoff = f.cutoff; p.bin_tiles = f.bin_tiles; p.kchunks = f.kchunks; p.passes = f.passes; p.row_tiles = f.row_tiles;
    p.overlap = sp.overlap; p.col_tiles = sp.col_tiles;
    p.wave_cols = stft_backward_wave_cols(sp.col_tiles);
    p.nf_max = f.nf_max; p.frame_tiles = f.frame_tiles;
    p.q_tiles = (f.nf_max - 1 + sp.overlap + kStftTile - 1) / kStftTile;
    p.melt_floats = (size_t)f.bin_tiles * f.row_tiles * 1024;
    p.basis_floats = sp.inv_floats;
    p.dz_floats = 2 * (size_t)B * f.cutoff * f.nf_max;
    p.dxpad_floats = (size_t)B * (size_t)(n + 2L * pad);
    *out = p;
    return 0;
}

static int melspec_grad_pack(int N, int hop, int n_mels, const float* fwd, const float* melb, float* packed, hipStream_t s) {
    MelGradPlan pl;
    T2_TRY_RC(melspec_grad_plan(N, hop, N / 2, n_mels, N, 1, &pl));
    T2_REQUIRE(fwd && melb && packed, "melspec_grad_pack: null pointer");
    hipLaunchKernelGGL(melspec_pack_t_kernel, dim3((unsigned)((pl.melt_floats + 255) / 256)), dim3(256), 0, s, melb, packed, n_mels, pl.cutoff, pl.row_tiles,
                       pl.melt_floats);
    T2_LAUNCH_CHECK();
    return stft_pack_overlap(N, hop, fwd, packed + pl.melt_floats, s);
}

static int melspec_backward(const t2_melspec_backward_args& a, hipStream_t s) {
    MelGradPlan pl;
    T2_TRY_RC(melspec_grad_plan(a.N, a.hop, a.pad, a.n_mels, a.n, a.B, &pl));
    T2_REQUIRE(a.x && a.packed && a.grad_packed && a.mel_sum && a.g && a.dx, "melspec backward: null pointer");
    T2_REQUIRE(a.clip_val > 0.f && a.mag_eps >= 0.f, "melspec backward: clip_val=%g must be positive, mag_eps=%g not negative", a.clip_val, a.mag_eps);
    T2_REQUIRE(a.workspace && a.workspace_floats >= pl.dz_floats + pl.dxpad_floats, "melspec backward: the workspace needs %zu floats, got %zu",
               pl.dz_floats + pl.dxpad_floats, a.workspace ? a.workspace_floats : (size_t)0);
    MelGrad p;
    p.x = a.x; p.lengths = a.lengths; p.pf = reinterpret_cast<const f32x4*>(a.packed); p.pt = reinterpret_cast<const f32x4*>(a.grad_packed);
    p.sums = a.mel_sum; p.g = a.g; p.d_re = a.workspace; p.d_im = a.workspace + pl.dz_floats / 2;
    p.n = a.n; p.nf_max = pl.nf_max;
    p.N = a.N; p.hop = a.hop; p.pad = a.pad; p.cutoff = pl.cutoff; p.bin_tiles = pl.bin_tiles; p.kchunks = pl.kchunks; p.n_mels = a.n_mels; p.row_tiles = pl.row_tiles;
    p.g_time_major = a.g_time_major != 0;
    p.mag_eps = a.mag_eps; p.clip = a.clip_val;
    hipLaunchKernelGGL(melspec_grad_kernel, dim3((unsigned)pl.frame_tiles, (unsigned)pl.passes, (unsigned)a.B), dim3(256), 0, s, p);
    T2_LAUNCH_CHECK();
    t2_stft_analysis_backward_args f{};
    f.B = a.B; f.N = a.N; f.hop = a.hop; f.n = a.n;
    f.d_re = p.d_re; f.d_im = p.d_im; f.basis_table = a.grad_packed + pl.melt_floats; f.lengths = a.lengths;
    f.dxpad = a.workspace + pl.dz_floats; f.dx = a.dx;
    return stft_analysis_backward(f, a.pad, s);
}

}  // namespace t2

// ---- C ABI (include/t2amd.h)
using namespace t2;

extern "C" {

int t2_melspec_plan(int N, int hop, int pad, int n_mels, long n, int B, t2_melspec_plan_info* out) {
    T2_REQUIRE(out, "t2_melspec_plan: null pointer");
    MelPlan p;
    T2_TRY_RC(melspec_plan(N, hop, pad, n_mels, n, B, &p));
    out->bins = p.cutoff; out->passes = p.passes; out->frame_tile = kStftTile; out->row_tiles = p.row_tiles; out->splits = p.splits;
    out->nf_max = p.nf_max; out->frame_tiles = p.frame_tiles; out->fwd_floats = p.fwd_floats; out->mel_floats = p.mel_floats;
    out->packed_bytes = (p.fwd_floats + p.mel_floats) * sizeof(float);
    out->scratch_floats = p.splits > 1 ? p.split_scratch_floats : 0; out->split_scratch_floats = p.split_scratch_floats;
    return 0;
}
int t2_melspec_pack(int N, int n_mels, const float* forward_basis, const float* mel_basis, float* packed, void* stream) {
    return melspec_pack(N, n_mels, forward_basis, mel_basis, packed, (hipStream_t)stream);
}
int t2_melspec(const t2_melspec_args* a, void* stream) {
    T2_REQUIRE(a, "t2_melspec: null arguments");
    return melspec(*a, (hipStream_t)stream);
}
int t2_melspec_grad_plan(int N, int hop, int pad, int n_mels, long n, int B, t2_melspec_grad_plan_info* out) {
    T2_REQUIRE(out, "t2_melspec_grad_plan: null pointer");
    MelGradPlan p;
    T2_TRY_RC(melspec_grad_plan(N, hop, pad, n_mels, n, B, &p));
    out->bins = p.cutoff; out->passes = p.passes; out->row_tiles = p.row_tiles; out->overlap = p.overlap; out->nf_max = p.nf_max;
    out->grid_x = p.frame_tiles; out->grid_y = p.passes; out->grid_z = B;
    out->fold_grid_x = p.q_tiles; out->fold_grid_y = (p.col_tiles + p.wave_cols - 1) / p.wave_cols;
    out->melt_floats = p.melt_floats; out->basis_floats = p.basis_floats; out->packed_bytes = (p.melt_floats + p.basis_floats) * sizeof(float);
    out->dz_floats = p.dz_floats; out->dxpad_floats = p.dxpad_floats; out->workspace_floats = p.dz_floats + p.dxpad_floats;
    return 0;
}
int t2_melspec_grad_pack(int N, int hop, int n_mels, const float* forward_basis, const float* mel_basis, float* packed, void* stream) {
    return melspec_grad_pack(N, hop, n_mels, forward_basis, mel_basis, packed, (hipStream_t)stream);
}
int t2_melspec_backward(const t2_melspec_backward_args* a, void* stream) {
    T2_REQUIRE(a, "t2_melspec_backward: null arguments");
    return melspec_backward(*a, (hipStream_t)stream);
}

}  // extern "C"
