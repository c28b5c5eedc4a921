// Silence trim for ragged batches: the reference's pydub trim (remove_silence.py:7-36, best_checkpoint.py:319-333 and
// :495-520) on 16-bit mono audio that stays on the device.  What pydub computes, restated (include/t2amd.h has the rules
// in full): with r = rate / 1000.0 and len_ms = round(1000 * (N / rate)), chunk k of an item is the frames
// [int(a * r), int(b * r)) for a = chunk * k, b = min(a + chunk, len_ms), zero-filled past the item's N frames; it is silent
// when 20 * log10(rms / 32768) < threshold, rms = (unsigned) sqrt(S / n) over its n frames.  The leading silence is
// chunk * (first loud k with chunk * k < len_ms), or None; the trailing silence is the same on the reversed frames.
//
// Every decision is an integer one.  R is the smallest rms in 1..32768 whose level is not below the threshold (host, the
// same log10), and a chunk is silent iff S < n * R^2 in 64-bit integers.  Floating point is left in three places, all fp64
// and none contractible into an fma: the divide, multiply and round-half-even of len_ms, and one multiply per chunk
// boundary.
//
//   silence_scan_kernel  (chunk group, item, direction): a wave owns a chunk and sums squares across its lanes; the workgroup
//                        takes one integer atomicMin on the item's first loud chunk.  A minimum does not depend on arrival
//                        order.  Every (direction, item) word has a 128-byte line of its own: atomics on words that share a
//                        line queue behind each other (measured: 0.55 ms for 64 items with packed words and an atomic per
//                        loud chunk, profiles/README.md round 31).
//   silence_cut_kernel   (column tile, item): start, end and new length from the two minima, the kept frames to the front
//                        of the output row, zeros behind them.
// Samples at or behind an item's length are never read: the appended zero frames exist only in n.
#include <math.h>

#include "kernels.h"

namespace t2 {

constexpr int kSilChunksPerGroup = 8;            // chunks a scan workgroup owns: two per wave
constexpr int kSilWordStride = 32;               // ints between two first-loud-chunk words: a 128-byte line each
constexpr int kSilCutSpan = 1024;                // output samples a cut workgroup writes: four per thread
constexpr int kSilNoneSilent = 0;                // R for a threshold of -inf: S < n * 0 never holds
constexpr int kSilAllSilent = 32769;             // R for a threshold above 0 dBFS: S <= n * 2^30 < n * 32769^2 always holds
// len(sound) of N frames: round(1000 * (float(N) / rate)), half to even on the double
__host__ __device__ inline int sil_len_ms(int N, int rate) { return (int)rint(1000.0 * ((double)N / (double)rate)); }
// the frame a millisecond maps to: int(ms * r), one double multiply, truncated
__host__ __device__ inline int sil_frame(int ms, double r) { return (int)((double)ms * r); }
struct SilPlan { int R, len_ms, chunks, groups; long out_width; size_t scratch_bytes; };

constexpr int kSilNone = 0x7f7f7f7f;             // "no loud chunk": what hipMemsetAsync(0x7f) leaves, above every chunk index

typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

struct SilScan {
    const void* x; const int* lengths; int* first;            // first [2][B] words kSilWordStride apart: forward, reversed
    long n; double r; unsigned long long R2;
    int B, rate, chunk_ms;
};

struct SilCut {
    const void* x; const int* lengths; const int* first; void* out; int* new_lengths; int* start_ms; int* end_ms;
    long n, W; double r; float scale;
    int B, rate, chunk_ms, R, leading_only;
};

// the item's own length, clamped to the row
__device__ __forceinline__ int sil_item_len(const int* lengths, long n, int b) {
    if (!lengths) return (int)n;
    const long l = lengths[b];
    return (int)(l < 0 ? 0 : (l > n ? n : l));
}

// a sample in int16 units: fp32 is clamped to the int16 range (NaN -> 0) and truncated toward zero, as astype('int16')
// does inside that range
__device__ __forceinline__ int sil_q(short v) { return v; }
__device__ __forceinline__ int sil_q(float v) {
    v = v == v ? v : 0.f;
    v = fminf(fmaxf(v, -32768.f), 32767.f);
    return (int)v;
}
__device__ __forceinline__ unsigned long long sil_sq(int q) { return (unsigned long long)((long long)q * q); }

__device__ __forceinline__ unsigned long long sil_sq16(const short* p) {
    const s16x8 v = *reinterpret_cast<const s16x8*>(p);
    unsigned long long s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += sil_sq(sil_q(v[i]));
    return s;
}
__device__ __forceinline__ unsigned long long sil_sq16(const float* p) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    unsigned long long s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += sil_sq(sil_q(v[i]));
    return s;
}

// Sum of squares of xb[lo .. hi) over the wave, in every lane.  16-byte loads on the address-aligned middle, single samples on
// the ragged head and tail: nothing outside [lo, hi) is read.
template <typename T>
__device__ __forceinline__ unsigned long long sil_wave_sumsq(const T* xb, int lo, int hi, int lane) {
    constexpr int G = 16 / (int)sizeof(T);
    unsigned long long s = 0;
    const int count = hi - lo;
    if (count > 0) {
        const int mis = (int)((reinterpret_cast<uintptr_t>(xb + lo) / sizeof(T)) & (G - 1));
        int head = (G - mis) & (G - 1);
        head = head < count ? head : count;
        const int groups = (count - head) / G;
        const int tail = count - head - groups * G;
        if (lane < head) s += sil_sq(sil_q(xb[lo + lane]));
        const T* body = xb + lo + head;
        for (int g = lane; g < groups; g += 64) s += sil_sq16(body + (size_t)g * G);
        if (lane < tail) s += sil_sq(sil_q(body[(size_t)groups * G + lane]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

template <typename T>
__global__ void __launch_bounds__(256) silence_scan_kernel(SilScan p) {
    __shared__ int seen, found[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, dir = blockIdx.z;
    const int N = sil_item_len(p.lengths, p.n, b);
    const int len_ms = sil_len_ms(N, p.rate);
    int* first = p.first + ((size_t)dir * p.B + b) * kSilWordStride;
    const int k0 = blockIdx.x * kSilChunksPerGroup;
    if ((long)k0 * p.chunk_ms >= len_ms) return;               // behind the item's last chunk (uniform over the workgroup)
    // One look at the item's word per workgroup: a group behind the minimum already there cannot lower it and skips its loads.
    // Whichever value the look returns, the minimum at the end is the same.
    if (threadIdx.x == 0) seen = __hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int cur = seen;
    if (k0 >= cur) return;
    const T* xb = static_cast<const T*>(p.x) + (size_t)b * p.n;
    int mine = kSilNone;                                       // this wave's first loud chunk
    for (int j = 0; j < kSilChunksPerGroup / 4; ++j) {
        const int k = k0 + wave + 4 * j;
        const long a_ms = (long)k * p.chunk_ms;
        if (a_ms >= len_ms || k >= cur) break;
        const int b_ms = (int)(a_ms + p.chunk_ms < len_ms ? a_ms + p.chunk_ms : len_ms);
        const int fa = sil_frame((int)a_ms, p.r), fb = sil_frame(b_ms, p.r);
        const int frames = fb > fa ? fb - fa : 0;              // appended zeros included
        int lo = fa < N ? fa : N, hi = fb < N ? fb : N;        // the part that is data
        if (hi < lo) hi = lo;
        if (dir) { const int t = N - hi; hi = N - lo; lo = t; }   // frame i of the reversed sound is frame N-1-i
        const unsigned long long S = sil_wave_sumsq(xb, lo, hi, lane);
        if (S >= (unsigned long long)frames * p.R2) {          // loud; the wave's later chunks lie behind this one
            mine = k;
            break;
        }
    }
    if (lane == 0) found[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {                                    // one atomic per workgroup, on a cache line of the item's own
        const int a = found[0] < found[1] ? found[0] : found[1], c = found[2] < found[3] ? found[2] : found[3];
        const int m = a < c ? a : c;
        if (m < cur) atomicMin(first, m);
    }
}

__device__ __forceinline__ void sil_put(short* o, int q, float) { *o = (short)q; }
__device__ __forceinline__ void sil_put(float* o, int q, float scale) { *o = __fmul_rn((float)q, scale); }
__device__ __forceinline__ void sil_put4(short* o, const int* q, float) {
    s16x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (short)q[i];
    *reinterpret_cast<s16x4*>(o) = v;
}
__device__ __forceinline__ void sil_put4(float* o, const int* q, float scale) {
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = __fmul_rn((float)q[i], scale);
    *reinterpret_cast<f32x4*>(o) = v;
}

template <typename Tin, typename Tout>
__global__ void __launch_bounds__(256) silence_cut_kernel(SilCut p) {
    const int b = blockIdx.y;
    const int N = sil_item_len(p.lengths, p.n, b);
    const int len_ms = sil_len_ms(N, p.rate);
    int s_ms = 0, e_ms = 0;                                    // nothing is silent under a threshold of -inf
    if (p.R != kSilNoneSilent) {
        const int ks = p.first[(size_t)b * kSilWordStride], ke = p.leading_only ? 0 : p.first[((size_t)p.B + b) * kSilWordStride];
        s_ms = ks == kSilNone ? -1 : ks * p.chunk_ms;          // chunk * k < len_ms: no overflow
        e_ms = p.leading_only || s_ms < 0 || ke == kSilNone ? -1 : ke * p.chunk_ms;   // the reference never looks for the end of a dropped item
    }
    if (p.leading_only) {
        if (blockIdx.x == 0 && threadIdx.x == 0) p.start_ms[b] = s_ms;
        return;
    }
    long fa = 0, keep = 0;
    if (s_ms >= 0 && e_ms >= 0) {                              // sound[start : len_ms - end]
        const int a = s_ms < len_ms ? s_ms : len_ms;
        int c = len_ms - e_ms;
        c = c < 0 ? 0 : c;
        fa = sil_frame(a, p.r);
        const long fb = sil_frame(c, p.r);
        keep = fb > fa ? fb - fa : 0;
        keep = keep < p.W ? keep : p.W;                        // never more than the row (the plan's width already covers it)
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        p.start_ms[b] = s_ms;
        p.end_ms[b] = e_ms;
        p.new_lengths[b] = (int)keep;
    }
    if (!p.out) return;
    const Tin* xb = static_cast<const Tin*>(p.x) + (size_t)b * p.n;
    Tout* ob = static_cast<Tout*>(p.out) + (size_t)b * p.W;
    // four outputs per thread, grouped so that a full group is one aligned vector store whatever the row's own alignment
    const int mis = (int)((reinterpret_cast<uintptr_t>(ob) / sizeof(Tout)) & 3);
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4 - mis;
    if (j0 >= p.W) return;
    int q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long j = j0 + i;
        q[i] = (j >= 0 && j < keep && fa + j < N) ? sil_q(xb[fa + j]) : 0;   // frames past N are the appended zeros
    }
    if (j0 >= 0 && j0 + 4 <= p.W) {
        sil_put4(ob + j0, q, p.scale);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (j0 + i >= 0 && j0 + i < p.W) sil_put(ob + j0 + i, q[i], p.scale);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------
static bool sil_below(int rms, double thr) { return 20.0 * log10((double)rms / 32768.0) < thr; }

// the smallest rms in 1..32768 whose level is not below thr
static int sil_threshold_rms(double thr) {
    if (isinf(thr) && thr < 0) return kSilNoneSilent;
    if (sil_below(32768, thr)) return kSilAllSilent;
    if (!sil_below(1, thr)) return 1;
    int lo = 1, hi = 32768;                                    // below(lo), not below(hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (sil_below(mid, thr)) lo = mid; else hi = mid;
    }
    return hi;
}

static int silence_plan(int rate, int chunk_ms, double thr, long n, int B, SilPlan* out) {   // validates; no device
    T2_REQUIRE(out, "silence: null plan");
    T2_REQUIRE(rate >= 4000 && rate <= 1000000, "silence: sample_rate=%d outside 4000..1000000", rate);
    T2_REQUIRE(chunk_ms >= 1 && chunk_ms <= 1000000, "silence: chunk_ms=%d outside 1..1000000", chunk_ms);
    T2_REQUIRE(thr == thr, "silence: threshold_db is NaN");
    T2_REQUIRE(n >= 0, "silence: n=%ld samples per row is negative", n);
    T2_REQUIRE(n <= INT32_MAX / 2, "silence: n=%ld samples per row exceed the %d that 32-bit frame indices take", n, INT32_MAX / 2);
    T2_REQUIRE(B >= 1 && B <= 65535, "silence: B=%d outside 1..65535", B);
    SilPlan p;
    const double r = rate / 1000.0;
    p.R = sil_threshold_rms(thr);
    p.len_ms = sil_len_ms((int)n, rate);
    p.chunks = (int)(((long)p.len_ms + chunk_ms - 1) / chunk_ms);
    p.groups = (p.chunks + kSilChunksPerGroup - 1) / kSilChunksPerGroup;
    p.out_width = n + (int)(0.5 * r) + 1;
    p.scratch_bytes = (size_t)2 * B * kSilWordStride * sizeof(int);
    *out = p;
    return 0;
}

template <typename Tin>
static void sil_launch_cut(const SilCut& c, int out_float, dim3 grid, hipStream_t s) {
    if (out_float) hipLaunchKernelGGL((silence_cut_kernel<Tin, float>), grid, dim3(256), 0, s, c);
    else hipLaunchKernelGGL((silence_cut_kernel<Tin, short>), grid, dim3(256), 0, s, c);
}

// x [B, n] int16 or fp32 (x_float) -> out [B, out_width] int16 or fp32 (out_float: int16 * scale), zero from new_lengths[b] on.
// lengths [B] int32 nullable.  start_ms / end_ms / new_lengths [B] int32.  leading_only: only start_ms is written (forward scan).
static int silence_trim(const t2_silence_args& a, hipStream_t s) {
    SilPlan pl;
    T2_TRY_RC(silence_plan(a.sample_rate, a.chunk_ms, a.threshold_db, a.n, a.B, &pl));
    T2_REQUIRE(a.x || a.n == 0, "silence: null input");
    T2_REQUIRE(a.start_ms, "silence: null start_ms");
    T2_REQUIRE(a.leading_only || (a.out && a.new_lengths && a.end_ms), "silence: null out, new_lengths or end_ms");
    T2_REQUIRE(a.scratch && a.scratch_bytes >= pl.scratch_bytes, "silence: %zu bytes of scratch needed, got %zu", pl.scratch_bytes,
               a.scratch ? a.scratch_bytes : (size_t)0);
    T2_REQUIRE(reinterpret_cast<uintptr_t>(a.scratch) % sizeof(int) == 0, "silence: scratch is not aligned to 4 bytes");
    T2_REQUIRE(reinterpret_cast<uintptr_t>(a.x) % (a.x_float ? 4 : 2) == 0, "silence: input is not aligned to its element size");
    T2_REQUIRE(a.leading_only || reinterpret_cast<uintptr_t>(a.out) % (a.out_float ? 4 : 2) == 0, "silence: output is not aligned to its element size");
    const double r = a.sample_rate / 1000.0;
    int* first = static_cast<int*>(a.scratch);
    if (pl.R != kSilNoneSilent) {
        T2_CHECK_HIP(hipMemsetAsync(first, 0x7f, pl.scratch_bytes, s));
        if (pl.groups > 0) {
            SilScan p;
            p.x = a.x; p.lengths = a.lengths; p.first = first; p.n = a.n; p.r = r; p.R2 = (unsigned long long)pl.R * pl.R;
            p.B = a.B; p.rate = a.sample_rate; p.chunk_ms = a.chunk_ms;
            const dim3 grid((unsigned)pl.groups, (unsigned)a.B, a.leading_only ? 1u : 2u);
            if (a.x_float) hipLaunchKernelGGL(silence_scan_kernel<float>, grid, dim3(256), 0, s, p);
            else hipLaunchKernelGGL(silence_scan_kernel<short>, grid, dim3(256), 0, s, p);
            T2_LAUNCH_CHECK();
        }
    }
    SilCut c;
    c.x = a.x; c.lengths = a.lengths; c.first = first; c.out = a.leading_only ? nullptr : a.out;
    c.new_lengths = a.new_lengths; c.start_ms = a.start_ms; c.end_ms = a.end_ms;
    c.n = a.n; c.W = pl.out_width; c.r = r; c.scale = a.scale;
    c.B = a.B; c.rate = a.sample_rate; c.chunk_ms = a.chunk_ms; c.R = pl.R; c.leading_only = a.leading_only != 0;
    const dim3 grid(a.leading_only ? 1u : (unsigned)((pl.out_width + 3 + kSilCutSpan - 1) / kSilCutSpan), (unsigned)a.B);
    if (a.x_float) sil_launch_cut<float>(c, a.out_float, grid, s);
    else sil_launch_cut<short>(c, a.out_float, grid, s);
    T2_LAUNCH_CHECK();
    return 0;
}

}  // namespace t2

// ---- C ABI (include/t2amd.h)
using namespace t2;

extern "C" {

int t2_silence_plan(int sample_rate, int chunk_ms, double threshold_db, long n, int B, t2_silence_plan_info* out) {
    T2_REQUIRE(out, "t2_silence_plan: null pointer");
    SilPlan p;
    T2_TRY_RC(silence_plan(sample_rate, chunk_ms, threshold_db, n, B, &p));
    out->R = p.R; out->len_ms = p.len_ms; out->chunks = p.chunks; out->chunks_per_group = kSilChunksPerGroup;
    out->scan_grid[0] = p.R == kSilNoneSilent ? 0 : p.groups; out->scan_grid[1] = B; out->scan_grid[2] = 2;
    out->cut_grid[0] = (int)((p.out_width + 3 + kSilCutSpan - 1) / kSilCutSpan); out->cut_grid[1] = B;
    out->block = 256; out->out_width = p.out_width; out->scratch_bytes = p.scratch_bytes;
    return 0;
}
int t2_silence_trim(const t2_silence_args* a, void* stream) {
    T2_REQUIRE(a, "t2_silence_trim: null arguments");
    return silence_trim(*a, (hipStream_t)stream);
}

}  // extern "C"
