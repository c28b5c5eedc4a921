// Soft-DTW (Cuturi & Blondel 2017) for checkpoint scoring: pairwise distances, the forward recurrence, its gradient
// and the gradient of the distances.  Replaces the two numba.cuda kernels of the reference's soft_dtw_cuda.py:34-111
// (and its host loops :185-239, which the reference falls back to above 1024 frames).
//
// The recurrence runs as a skewed wavefront, one workgroup per pair: thread t owns RPT consecutive rows and does
// column p - t of them at pass p, so the cell above its first row is what thread t - 1 finished one pass earlier.
// That one value per thread and pass travels by a lane shift inside a wave and through a double-buffered LDS slot
// per wave between waves: one workgroup barrier per pass, nothing crosses workgroups, nothing spins.
//
// Internal scratch (the distances the library computes itself, and R when a gradient is wanted) is laid out the way
// the wavefront walks it, [pair][pass][thread][row of the thread]: each pass reads / writes RPT adjacent floats per
// lane and adjacent lanes adjacent groups.  A caller's own D and the returned E are row-major [B,N,M].
//
// A cell is a fixed function of its three neighbours and D (contraction is off in the cell functions, the fused
// operations are written out), so the value does not depend on the partition: a pair inside a padded batch, alone,
// with or without the stored R, and from run to run gives the same bits.
#include "kernels.h"

namespace t2 {

constexpr int kSoftDtwMaxLen = 8192;             // frames per sequence: 1024 threads x 8 rows

constexpr int kSdtwMaxThreads = 1024;
constexpr int kSdtwMaxRpt = 8;                       // ladder 1, 2, 4, 8: N up to 8192
constexpr int kSdtwMaxWaves = kSdtwMaxThreads / kWave;
static_assert(kSdtwMaxThreads * kSdtwMaxRpt == kSoftDtwMaxLen, "the ladder covers exactly the advertised limit");

// The partition of one pair's recurrence, decided on the host (no device needed; t2amd.h t2_softdtw_plan_info has the fields)
static int softdtw_plan(int B, int N, int M, float gamma, int need_grad, t2_softdtw_plan_info* out) {
    T2_REQUIRE(out, "softdtw: null plan");
    T2_REQUIRE(B >= 1, "softdtw: B=%d must be at least 1", B);
    T2_REQUIRE(N >= 1 && M >= 1, "softdtw: N=%d and M=%d must be at least 1", N, M);
    T2_REQUIRE(N <= kSoftDtwMaxLen && M <= kSoftDtwMaxLen, "softdtw: N=%d, M=%d exceed the limit of %d frames per sequence", N, M, kSoftDtwMaxLen);
    T2_REQUIRE(gamma > 0.f, "softdtw: gamma=%g must be positive", (double)gamma);     // also refuses NaN
    int rpt = 1;
    while (rpt * kSdtwMaxThreads < N) rpt *= 2;
    const int owners = (N + rpt - 1) / rpt;                        // threads that own at least one row
    out->rows_per_thread = rpt;
    out->threads = (owners + kWave - 1) / kWave * kWave;
    out->passes = M + owners - 1;                                  // the last owner starts owners - 1 passes late
    out->d_floats = (size_t)B * out->passes * out->threads * rpt;
    out->r_floats = need_grad ? out->d_floats : 0;
    out->e_floats = need_grad ? (size_t)B * N * M : 0;
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// cells
// ------------------------------------------------------------------------------------------------------------------
// R[i,j] = D + softmin_gamma(diag, up, left), soft_dtw_cuda.py:66-72 term by term
__device__ __forceinline__ float sdtw_cell(float d, float diag, float up, float left, float gamma, float inv_gamma) {
#pragma clang fp contract(off)
    const float r0 = -diag * inv_gamma, r1 = -up * inv_gamma, r2 = -left * inv_gamma;
    const float rmax = fmaxf(fmaxf(r0, r1), r2);
    const float rsum = (expf(r0 - rmax) + expf(r1 - rmax)) + expf(r2 - rmax);
    const float softmin = -gamma * (logf(rsum) + rmax);
    return d + softmin;
}
// E[i,j] = E_down * a + E_right * b + E_diag * c, soft_dtw_cuda.py:105-108
__device__ __forceinline__ float sdtw_cell_bwd(float r, float r_down, float r_right, float r_diag, float d_down, float d_right,
                                               float d_diag, float e_down, float e_right, float e_diag, float inv_gamma) {
#pragma clang fp contract(off)
    const float a = expf(((r_down - r) - d_down) * inv_gamma);
    const float b = expf(((r_right - r) - d_right) * inv_gamma);
    const float c = expf(((r_diag - r) - d_diag) * inv_gamma);
    return (e_down * a + e_right * b) + e_diag * c;
}
__device__ __forceinline__ bool sdtw_out_of_band(int i, int j, float bandwidth) {     // 1-based i, j
    return bandwidth > 0.f && (float)abs(i - j) > bandwidth;
}
__device__ __forceinline__ float sdtw_neg_if_inf(float r) { return isinf(r) ? -INFINITY : r; }   // soft_dtw_cuda.py:100-101

template <int RPT> struct SdtwRows { float v[RPT]; };
template <int RPT> __device__ __forceinline__ SdtwRows<RPT> sdtw_load(const float* p) {
    SdtwRows<RPT> r;
    if constexpr (RPT == 1) r.v[0] = *p;
    else if constexpr (RPT == 2) { const float2 t = *reinterpret_cast<const float2*>(p); r.v[0] = t.x; r.v[1] = t.y; }
    else {
#pragma unroll
        for (int q = 0; q < RPT / 4; ++q) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p + 4 * q);
            r.v[4 * q] = t.x; r.v[4 * q + 1] = t.y; r.v[4 * q + 2] = t.z; r.v[4 * q + 3] = t.w;
        }
    }
    return r;
}
template <int RPT> __device__ __forceinline__ void sdtw_store(float* p, const SdtwRows<RPT>& r) {
    if constexpr (RPT == 1) *p = r.v[0];
    else if constexpr (RPT == 2) *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
    else {
#pragma unroll
        for (int q = 0; q < RPT / 4; ++q) {
            f32x4 t; t.x = r.v[4 * q]; t.y = r.v[4 * q + 1]; t.z = r.v[4 * q + 2]; t.w = r.v[4 * q + 3];
            *reinterpret_cast<f32x4*>(p + 4 * q) = t;
        }
    }
}

// D of the RPT rows of thread t at column J (0-based), for the pass p = J + t.  SKEW: the internal layout; otherwise the
// caller's row-major [N, M] plane, where rows / columns outside the matrix read as 0 (they are never used).
template <int RPT, bool SKEW>
__device__ __forceinline__ SdtwRows<RPT> sdtw_load_d(const float* Dp, int T, int N, int M, int t, int J) {
    if constexpr (SKEW) {
        return sdtw_load<RPT>(Dp + ((size_t)(J + t) * T + t) * RPT);
    } else {
        SdtwRows<RPT> r;
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const int i = t * RPT + k;
            r.v[k] = (i < N && J >= 0 && J < M) ? Dp[(size_t)i * M + J] : 0.f;
        }
        return r;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// distances: D[b,i,j] = sum_c (x[b,i,c] - y[b,j,c])^2, c ascending, one fused multiply-add per term; written in the
// internal layout of the partition (T threads, RPT rows each).  One thread per slot of the layout.
// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) softdtw_dist_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ Ds,
                                                          int N, int M, int d, int T, int rpt, int passes) {
    const int b = blockIdx.z, p = blockIdx.y;
    const int slot = blockIdx.x * 256 + threadIdx.x;              // t * rpt + k = the row
    if (slot >= T * rpt) return;
    const int i = slot, j = p - slot / rpt;
    float acc = 0.f;
    if (i < N && j >= 0 && j < M) {
        const float* xr = x + ((size_t)b * N + i) * d;
        const float* yr = y + ((size_t)b * M + j) * d;
        for (int c = 0; c < d; ++c) {
            const float df = xr[c] - yr[c];
            acc = fmaf(df, df, acc);
        }
    }
    Ds[((size_t)b * passes + p) * T * rpt + slot] = acc;
}

// ------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------
// value of thread t - 1 (forward) / t + 1 (backward) from the pass before.  `mine` is this thread's value of that pass;
// slot[par ^ 1] holds what the boundary lanes wrote before the last barrier.  In a kernel's first pass nothing has been
// written there yet: the boundary lanes read an uninitialised slot, and the value is never used (forward: a thread past
// the first wave has no column before pass 64, and takes its first diagonal from the border; backward: the thread below
// has not had a column yet either, so the caller's border values apply).
template <bool UP>
__device__ __forceinline__ float sdtw_neighbour(float mine, const float (*slot)[kSdtwMaxWaves], int par, int lane, int wave, int nwaves) {
    float v = UP ? __shfl_up(mine, 1, kWave) : __shfl_down(mine, 1, kWave);
    if (UP) { if (lane == 0 && wave > 0) v = slot[par ^ 1][wave - 1]; }
    else { if (lane == kWave - 1 && wave + 1 < nwaves) v = slot[par ^ 1][wave + 1]; }
    return v;
}

template <int RPT, bool SKEW, bool GRAD>
__global__ void __launch_bounds__(kSdtwMaxThreads) softdtw_fwd_kernel(const float* __restrict__ Dsrc, float* __restrict__ Rs, float* __restrict__ value,
                                                                     const int* __restrict__ xlen, const int* __restrict__ ylen,
                                                                     int N, int M, int T, int passes, float gamma, float bandwidth) {
    __shared__ float slot[2][kSdtwMaxWaves];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave, nwaves = T / kWave;
    const int n = xlen ? min(max(xlen[b], 0), N) : N, m = ylen ? min(max(ylen[b], 0), M) : M;
    if (n < 1 || m < 1) {                                           // an empty sequence: no path (uniform over the workgroup)
        if (t == 0) value[b] = INFINITY;
        return;
    }
    const float inv_gamma = 1.0f / gamma;
    const float* Dp = Dsrc + (SKEW ? (size_t)b * passes * T * RPT : (size_t)b * N * M);
    float* Rp = GRAD ? Rs + (size_t)b * passes * T * RPT : nullptr;
    const int last_pass = (m - 1) + (n - 1) / RPT;                  // the owner of row n does column m then
    const int i0 = t * RPT;                                         // 0-based first row

    SdtwRows<RPT> left;                                             // R[i, j-1] of my rows: column 0 of the padded grid
#pragma unroll
    for (int k = 0; k < RPT; ++k) left.v[k] = INFINITY;
    float up_prev = INFINITY;                                       // R[i0-1, j-1]
    float mine = INFINITY;                                          // my last row's value of the pass before
    SdtwRows<RPT> dcur = sdtw_load_d<RPT, SKEW>(Dp, T, N, M, t, 0 - t);

    for (int p = 0; p <= last_pass; ++p) {
        const int J = p - t, par = p & 1;
        SdtwRows<RPT> dnext = dcur;
        if (p < last_pass) dnext = sdtw_load_d<RPT, SKEW>(Dp, T, N, M, t, J + 1);    // on its way across the barrier
        float up = sdtw_neighbour<true>(mine, slot, par, lane, wave, nwaves);
        if (t == 0) up = INFINITY;                                  // row 0 of the padded grid
        if (J >= 0 && J < m && i0 < n) {
            float diag = J == 0 ? (t == 0 ? 0.f : INFINITY) : up_prev;
            float above = up;
#pragma unroll
            for (int k = 0; k < RPT; ++k) {
                const float l = left.v[k];
                float r = INFINITY;
                if (i0 + k < n && !sdtw_out_of_band(i0 + k + 1, J + 1, bandwidth))
                    r = sdtw_cell(dcur.v[k], diag, above, l, gamma, inv_gamma);
                diag = l; above = r; left.v[k] = r;
            }
            if constexpr (GRAD) sdtw_store<RPT>(Rp + ((size_t)p * T + t) * RPT, left);
            mine = left.v[RPT - 1];
        }
        up_prev = up;
        if (lane == kWave - 1) slot[par][wave] = mine;
        __syncthreads();
        dcur = dnext;
    }
    if (t == (n - 1) / RPT) {
        float v = left.v[0];
#pragma unroll
        for (int k = 1; k < RPT; ++k) if (k == (n - 1) % RPT) v = left.v[k];
        value[b] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// backward: the same wavefront from the last pass to the first over the stored R.  Thread t keeps column j+1 of its rows
// (R, D, E) in registers, reads column j of its rows and of row i+1 below them from the scratch, and gets E of row i+1
// from thread t + 1.  The padded grid's row n+1 and column m+1 are R = -inf, D = 0, E = 0, except the corner
// (n+1, m+1): R = R[n,m], E = 1 (soft_dtw_cuda.py:158-166).
// ------------------------------------------------------------------------------------------------------------------
template <int RPT, bool SKEW>
__global__ void __launch_bounds__(kSdtwMaxThreads) softdtw_bwd_kernel(const float* __restrict__ Dsrc, const float* __restrict__ Rs, float* __restrict__ E,
                                                                     const int* __restrict__ xlen, const int* __restrict__ ylen,
                                                                     int N, int M, int T, int passes, float gamma, float bandwidth) {
    __shared__ float slot[2][kSdtwMaxWaves];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave, nwaves = T / kWave;
    const int n = xlen ? min(max(xlen[b], 0), N) : N, m = ylen ? min(max(ylen[b], 0), M) : M;
    if (n < 1 || m < 1) return;                                     // E stays zero
    const float inv_gamma = 1.0f / gamma;
    const float* Dp = Dsrc + (SKEW ? (size_t)b * passes * T * RPT : (size_t)b * N * M);
    const float* Rp = Rs + (size_t)b * passes * T * RPT;
    float* Ep = E + (size_t)b * N * M;
    const int last_pass = (m - 1) + (n - 1) / RPT;
    const int i0 = t * RPT;
    const bool has_below = i0 + RPT < n;                            // row i0 + RPT (0-based) exists: thread t + 1 owns it
    const float r_end = Rp[((size_t)last_pass * T + (n - 1) / RPT) * RPT + (n - 1) % RPT];    // R[n,m], unconverted

    // column j+1: my rows, and the row below them
    SdtwRows<RPT> r_right, d_right, e_right;
#pragma unroll
    for (int k = 0; k < RPT; ++k) { r_right.v[k] = -INFINITY; d_right.v[k] = 0.f; e_right.v[k] = 0.f; }
    float rb_right = -INFINITY, db_right = 0.f, eb_right = 0.f;
    float mine = 0.f;                                               // E of my first row, of the pass before

    for (int p = last_pass; p >= 0; --p) {
        const int J = p - t, par = p & 1;
        const bool on = J >= 0 && J < m && i0 < n;
        SdtwRows<RPT> rc, dc;
        float rb = -INFINITY, db = 0.f;
        if (on) {
            rc = sdtw_load<RPT>(Rp + ((size_t)p * T + t) * RPT);
            dc = sdtw_load_d<RPT, SKEW>(Dp, T, N, M, t, J);
            if (has_below) {                                        // (i0 + RPT, J): thread t + 1 at pass p + 1, its row 0
                rb = sdtw_neg_if_inf(Rp[((size_t)(p + 1) * T + t + 1) * RPT]);
                db = SKEW ? Dp[((size_t)(p + 1) * T + t + 1) * RPT] : Dp[(size_t)(i0 + RPT) * M + J];
            }
        }
        float eb = sdtw_neighbour<false>(mine, slot, par, lane, wave, nwaves);
        if (!has_below) eb = 0.f;
        if (on) {
            // (a thread's first column is m: the initial values above are column m+1 of the padded grid)
            // neighbours of the row under consideration, walking up from my last row
            float r_down = rb, d_down = db, e_down = eb, r_diag = rb_right, d_diag = db_right, e_diag = eb_right;
            SdtwRows<RPT> e_new;
#pragma unroll
            for (int k = RPT - 1; k >= 0; --k) {
                const int i = i0 + k;                               // 0-based
                const float r = sdtw_neg_if_inf(rc.v[k]);
                float e = 0.f;
                if (i < n) {
                    if (i == n - 1) {                               // row n+1 of the padded grid
                        r_down = -INFINITY; d_down = 0.f; e_down = 0.f;
                        const bool corner = J == m - 1;
                        r_diag = corner ? r_end : -INFINITY; d_diag = 0.f; e_diag = corner ? 1.f : 0.f;
                    }
                    if (!sdtw_out_of_band(i + 1, J + 1, bandwidth))
                        e = sdtw_cell_bwd(r, r_down, r_right.v[k], r_diag, d_down, d_right.v[k], d_diag, e_down, e_right.v[k], e_diag, inv_gamma);
                    Ep[(size_t)i * M + J] = e;
                }
                // this row is "down" for the row above it, its column-(j+1) values are that row's diagonal
                r_diag = r_right.v[k]; d_diag = d_right.v[k]; e_diag = e_right.v[k];
                r_down = r; d_down = dc.v[k]; e_down = e;
                rc.v[k] = r; e_new.v[k] = e;
            }
            r_right = rc; d_right = dc; e_right = e_new;
            rb_right = rb; db_right = db; eb_right = eb;
            mine = e_new.v[0];
        }
        if (lane == 0) slot[par][wave] = mine;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------
// gradient of the distances: dX[b,i,c] = 2 sum_j G[b,i,j] (x[b,i,c] - y[b,j,c]), dY[b,j,c] = -2 sum_i G[b,i,j] (x - y),
// G = grad_out[b] * E, j resp. i ascending, one fused multiply-add per term: no atomics, one thread per output element.
// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) softdtw_dist_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ E,
                                                              const float* __restrict__ grad_out, const int* __restrict__ xlen, const int* __restrict__ ylen,
                                                              float* __restrict__ dX, float* __restrict__ dY, int N, int M, int d) {
    const int b = blockIdx.y;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nx = (size_t)N * d, ny = (size_t)M * d;
    if (idx >= nx + ny) return;
    const int n = xlen ? min(max(xlen[b], 0), N) : N, m = ylen ? min(max(ylen[b], 0), M) : M;
    const float g = grad_out[b];
    const float* Eb = E + (size_t)b * N * M;
    const float* xb = x + (size_t)b * nx;
    const float* yb = y + (size_t)b * ny;
    float acc = 0.f;
    if (idx < nx) {
        const int i = (int)(idx / d), c = (int)(idx % d);
        if (i < n) {
            const float xv = xb[idx];
            for (int j = 0; j < m; ++j) acc = fmaf(g * Eb[(size_t)i * M + j], xv - yb[(size_t)j * d + c], acc);
        }
        dX[(size_t)b * nx + idx] = 2.f * acc;
    } else {
        const size_t o = idx - nx;
        const int j = (int)(o / d), c = (int)(o % d);
        if (j < m) {
            const float yv = yb[o];
            for (int i = 0; i < n; ++i) acc = fmaf(g * Eb[(size_t)i * M + j], yv - xb[(size_t)i * d + c], acc);   // -(x - y), exactly
        }
        dY[(size_t)b * ny + o] = 2.f * acc;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// host: every call takes its argument struct of t2amd.h
// ------------------------------------------------------------------------------------------------------------------
static int softdtw_dist(const t2_softdtw_dist_args& a, hipStream_t s) {
    t2_softdtw_plan_info pl;
    T2_TRY_RC(softdtw_plan(a.B, a.N, a.M, 1.f, 0, &pl));
    T2_REQUIRE(a.d >= 1, "softdtw: feature dimension d=%d must be at least 1", a.d);
    T2_REQUIRE(a.x && a.y && a.Ds, "softdtw_dist: null pointer");
    T2_REQUIRE(a.B <= 65535, "softdtw_dist: B=%d exceeds the grid limit of 65535 pairs", a.B);     // passes <= 8192 + 1023
    const int slots = pl.threads * pl.rows_per_thread;
    dim3 grid((slots + 255) / 256, pl.passes, a.B);
    hipLaunchKernelGGL(softdtw_dist_kernel, grid, dim3(256), 0, s, a.x, a.y, a.Ds, a.N, a.M, a.d, pl.threads, pl.rows_per_thread, pl.passes);
    T2_LAUNCH_CHECK();
    return 0;
}

template <class Args>   // t2_softdtw_fwd_args or t2_softdtw_bwd_args
static int softdtw_check(const Args& a, const char* who) {
    T2_REQUIRE((a.D != nullptr) != (a.Ds != nullptr), "%s: exactly one of D (row-major) and Ds (from softdtw_dist) must be given", who);
    T2_REQUIRE(a.bandwidth >= 0.f, "%s: bandwidth=%g must not be negative (0 = off)", who, (double)a.bandwidth);
    T2_REQUIRE((a.x_lengths == nullptr) == (a.y_lengths == nullptr), "%s: give both length arrays or neither", who);
    return 0;
}

template <int RPT>
static void softdtw_fwd_launch(const t2_softdtw_fwd_args& a, const t2_softdtw_plan_info& pl, hipStream_t s) {
    const bool skew = a.Ds != nullptr, grad = a.R != nullptr;
    const float* src = skew ? a.Ds : a.D;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(a.B), dim3(pl.threads), 0, s, src, a.R, a.value, a.x_lengths, a.y_lengths,
                           a.N, a.M, pl.threads, pl.passes, a.gamma, a.bandwidth);
    };
    if (skew) { if (grad) go(softdtw_fwd_kernel<RPT, true, true>); else go(softdtw_fwd_kernel<RPT, true, false>); }
    else      { if (grad) go(softdtw_fwd_kernel<RPT, false, true>); else go(softdtw_fwd_kernel<RPT, false, false>); }
}

// value[b] = R[n_b, m_b]; R != null stores the whole R (r_floats) for softdtw_bwd
static int softdtw_fwd(const t2_softdtw_fwd_args& a, hipStream_t s) {
    t2_softdtw_plan_info pl;
    T2_TRY_RC(softdtw_plan(a.B, a.N, a.M, a.gamma, a.R != nullptr, &pl));
    T2_TRY_RC(softdtw_check(a, "softdtw_forward"));
    T2_REQUIRE(a.value, "softdtw_forward: null output");
    switch (pl.rows_per_thread) {
        case 1: softdtw_fwd_launch<1>(a, pl, s); break;
        case 2: softdtw_fwd_launch<2>(a, pl, s); break;
        case 4: softdtw_fwd_launch<4>(a, pl, s); break;
        default: softdtw_fwd_launch<8>(a, pl, s); break;
    }
    T2_LAUNCH_CHECK();
    return 0;
}

template <int RPT>
static void softdtw_bwd_launch(const t2_softdtw_bwd_args& a, const t2_softdtw_plan_info& pl, hipStream_t s) {
    if (a.Ds)
        hipLaunchKernelGGL((softdtw_bwd_kernel<RPT, true>), dim3(a.B), dim3(pl.threads), 0, s, a.Ds, a.R, a.E, a.x_lengths, a.y_lengths,
                           a.N, a.M, pl.threads, pl.passes, a.gamma, a.bandwidth);
    else
        hipLaunchKernelGGL((softdtw_bwd_kernel<RPT, false>), dim3(a.B), dim3(pl.threads), 0, s, a.D, a.R, a.E, a.x_lengths, a.y_lengths,
                           a.N, a.M, pl.threads, pl.passes, a.gamma, a.bandwidth);
}

// E [B,N,M], zeroed here first
static int softdtw_bwd(const t2_softdtw_bwd_args& a, hipStream_t s) {
    t2_softdtw_plan_info pl;
    T2_TRY_RC(softdtw_plan(a.B, a.N, a.M, a.gamma, 1, &pl));
    T2_TRY_RC(softdtw_check(a, "softdtw_backward"));
    T2_REQUIRE(a.R && a.E, "softdtw_backward: R (stored by the forward call) and E must be given");
    T2_CHECK_HIP(hipMemsetAsync(a.E, 0, pl.e_floats * sizeof(float), s));     // padding and skipped pairs stay exact zeros
    switch (pl.rows_per_thread) {
        case 1: softdtw_bwd_launch<1>(a, pl, s); break;
        case 2: softdtw_bwd_launch<2>(a, pl, s); break;
        case 4: softdtw_bwd_launch<4>(a, pl, s); break;
        default: softdtw_bwd_launch<8>(a, pl, s); break;
    }
    T2_LAUNCH_CHECK();
    return 0;
}

static int softdtw_dist_bwd(const t2_softdtw_dist_bwd_args& a, hipStream_t s) {
    t2_softdtw_plan_info pl;
    T2_TRY_RC(softdtw_plan(a.B, a.N, a.M, 1.f, 1, &pl));
    T2_REQUIRE(a.d >= 1, "softdtw: feature dimension d=%d must be at least 1", a.d);
    T2_REQUIRE(a.x && a.y && a.E && a.grad_out && a.dX && a.dY, "softdtw_dist_backward: null pointer");
    T2_REQUIRE((a.x_lengths == nullptr) == (a.y_lengths == nullptr), "softdtw_dist_backward: give both length arrays or neither");
    T2_REQUIRE(a.B <= 65535, "softdtw_dist_backward: B=%d exceeds the grid limit of 65535 pairs", a.B);
    const size_t total = ((size_t)a.N + a.M) * a.d;
    dim3 grid((unsigned)((total + 255) / 256), a.B);
    hipLaunchKernelGGL(softdtw_dist_bwd_kernel, grid, dim3(256), 0, s, a.x, a.y, a.E, a.grad_out, a.x_lengths, a.y_lengths, a.dX, a.dY, a.N, a.M, a.d);
    T2_LAUNCH_CHECK();
    return 0;
}

}  // namespace t2

// ---- C ABI (include/t2amd.h)
using namespace t2;

extern "C" {

int t2_softdtw_plan(int B, int N, int M, float gamma, int need_grad, t2_softdtw_plan_info* out) {
    t2_softdtw_plan_info p;
    T2_TRY_RC(softdtw_plan(B, N, M, gamma, need_grad, &p));
    T2_REQUIRE(out, "t2_softdtw_plan: null output");
    *out = p;
    return 0;
}
int t2_softdtw_dist(const t2_softdtw_dist_args* a, void* stream) {
    T2_REQUIRE(a, "t2_softdtw_dist: null arguments");
    return softdtw_dist(*a, (hipStream_t)stream);
}
int t2_softdtw_forward(const t2_softdtw_fwd_args* a, void* stream) {
    T2_REQUIRE(a, "t2_softdtw_forward: null arguments");
    return softdtw_fwd(*a, (hipStream_t)stream);
}
int t2_softdtw_backward(const t2_softdtw_bwd_args* a, void* stream) {
    T2_REQUIRE(a, "t2_softdtw_backward: null arguments");
    return softdtw_bwd(*a, (hipStream_t)stream);
}
int t2_softdtw_dist_backward(const t2_softdtw_dist_bwd_args* a, void* stream) {
    T2_REQUIRE(a, "t2_softdtw_dist_backward: null arguments");
    return softdtw_dist_bwd(*a, (hipStream_t)stream);
}

}  // extern "C"
