// One attention step for both decoder streams (phone / sub-word) in one launch:
// one workgroup per (batch item, stream).
//
//   SMA     StepwiseMonotonicAttention.forward   (attention.py:374-398)
//           e_j = v . tanh(q + pm_j) ; mask -> -inf ; (+ noise*std in training) ; p = sigmoid(e)
//           a_t[j] = a_{t-1}[j] p_j + a_{t-1}[j-1] (1 - p_{j-1})   ; ctx = a_t . memory
//   LSA     LocationSensitiveAttention.forward   (attention.py:64-85, LocationLayer :7-23)
//           e_j = v . tanh(q + dense(conv([w_prev; w_cum]))_j + pm_j) ; mask ; softmax ; ctx = w . memory
//
// The processed-memory rows (A floats) are read 16 B per lane by groups of 16 lanes per
// position j and reduced with wave shuffles; the encoder memory rows (E floats) are read
// 16 B per lane, fully coalesced, once per step.  Positions whose weight is exactly 0 are
// skipped in the context sum (SMA alignments are sparse early on; 0*x contributes nothing).
//
// This file: the SMA / LSA forward kernel, the SMA backward kernel and the two dispatch functions.  The LSA backward
// kernels, GMM and DCA live in attention_lsa_bwd.hip, attention_gmm.hip and attention_dca.hip.
#include "attention_common.h"

#ifdef T2_STAMPS
__device__ unsigned long long t2_stamps_attn[32];
#define T2_ASTAMP(o, i)                                                                          \
    do {                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        if (blockIdx.x == 7 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) t2_stamps_attn[(o) + (i)] = __builtin_amdgcn_s_memrealtime(); \
        __builtin_amdgcn_sched_barrier(0);                                                       \
    } while (0)
extern "C" int t2_debug_read_stamps_attn(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(t2_stamps_attn), sizeof(unsigned long long) * n);
}
#else
#define T2_ASTAMP(o, i)
#endif

namespace t2 {

namespace {


__global__ __launch_bounds__(NT) void attention_step_fwd_kernel(AttnStepDesc d) {
    const AttnStream& st = d.st[blockIdx.y];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tin = st.Tin, A = d.A, E = d.E, F = d.F, Kc = d.Kc;
    const int Tp = (Tin + 3) & ~3;

    T2_ASTAMP(0, 0);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* q = smem;                 // [A]
    float* vs = q + A;               // [A]
    float* e = vs + A;               // [Tp]
    float* ap = e + Tp;              // [Tp]
    float* an = ap + Tp;             // [Tp]
    float* red = an + Tp;            // [4*NT]  (query partial groups: (NT/(A/4)) * A floats)
    float* cred = red + 4 * NT;      // [nh*E]
    const int nd = E / 4, nh = NT / nd;
    float* lsa = cred + nh * E;      // LSA only: convw[F*2*Kc] dense[A*(F+1)] loc[Tin*(F+1)] wpad[2][Tin+Kc-1]

    // Processed-memory rows of the first 2 x NT/16 positions (2 x 64 channels per lane) are requested now: they do
    // not depend on the query, and the kernel is a chain of dependent L2/MALL round trips
    constexpr int PFJ = 2, PFA = 2;
    f32x4 pmv[PFJ][PFA];
    {
        const int gid = tid >> 4, sub = tid & 15;
#pragma unroll
        for (int i = 0; i < PFJ; ++i)
#pragma unroll
            for (int k = 0; k < PFA; ++k)
                pmv[i][k] = *reinterpret_cast<const f32x4*>(st.pm + ((long)b * Tin + min(gid + i * (NT / 16), Tin - 1)) * A + min(sub * 4 + 64 * k, A - 4));
    }

    // ---- query: direct, or ordered sum of the partials emitted by lstm_step_fwd
    if (st.qpart) {
        // groups of A/4 lanes read one partial row (16 B per lane); NT/(A/4) rows in flight per pass
        const int a4n = A / 4, ng = NT / a4n;
        const int pg = tid / a4n, a4 = (tid % a4n) * 4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* p = st.qpart + (long)b * A + a4;
        const long ps = (long)d.B * A;
#pragma unroll 4
        for (int i = pg; i < st.nparts; i += ng) acc += *reinterpret_cast<const f32x4*>(p + (long)i * ps);
        *reinterpret_cast<f32x4*>(red + pg * A + a4) = acc;
        __syncthreads();
        if (tid < A) {
            float sum = 0.f;
            const int used = st.nparts < ng ? st.nparts : ng;
            for (int h2 = 0; h2 < used; ++h2) sum += red[h2 * A + tid];
            q[tid] = sum;
            if (st.q_out) st.q_out[(long)b * st.ldq_out + tid] = sum;
        }
    } else {
        for (int a = tid; a < A; a += NT) q[a] = st.query[(long)b * st.ldq + a];
    }
    for (int a = tid; a < A; a += NT) vs[a] = st.v[a];

    // previous alignment / weights
    for (int j = tid; j < Tin; j += NT)
        ap[j] = st.a_prev ? st.a_prev[(long)b * st.lda_prev + j] : ((d.kind == AttnKind::SMA && j == 0) ? 1.f : 0.f);

    float* loc = nullptr; float* dense = nullptr; float* paS = nullptr;
    const int F1 = F + 1, PA = A + 8;            // PA % 16 == 8: the two row-halves of an MFMA tile store to disjoint banks
    if (d.kind == AttnKind::LSA) {
        float* convw = lsa;
        dense = convw + F * 2 * Kc;
        loc = dense + A * F1;
        float* wpad = loc + ((Tin * F1 + 3) & ~3);
        const int pad = (Kc - 1) / 2, Tw = Tin + Kc - 1, TwP = (Tw + 4 + 3) & ~3;
        if (d.lsa_pa) paS = wpad + 2 * TwP;
        for (int i = tid; i < F * 2 * Kc; i += NT) convw[i] = st.loc_conv[i];
        for (int i = tid; i < A * F1; i += NT) dense[i] = (i % F1) < F ? st.loc_dense[(i / F1) * F + (i % F1)] : 0.f;
        for (int i = tid; i < 2 * TwP; i += NT) {
            const int c = i / TwP, j = i % TwP - pad;
            float v = 0.f;
            if (j >= 0 && j < Tin) v = c == 0 ? (st.a_prev ? st.a_prev[(long)b * st.lda_prev + j] : 0.f)
                                              : (st.wcum_prev ? st.wcum_prev[(long)b * st.ldwcum_prev + j] : 0.f);
            wpad[i] = v;
        }
        __syncthreads();
        // location conv: loc[j][f] = sum_c sum_k convw[f][c][k] * wcat[c][j + k - pad]; one thread per (f, 4 positions):
        // the sliding window lives in registers, 2 LDS reads per 4 MACs
        const int nj4 = (Tin + 3) / 4;
        for (int i = tid; i < nj4 * F; i += NT) {
            const int f = i % F, j0 = (i / F) * 4;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            for (int c = 0; c < 2; ++c) {
                const float* w = convw + (f * 2 + c) * Kc;
                const float* x = wpad + c * TwP + j0;
                float x0 = x[0], x1 = x[1], x2 = x[2];
                for (int k = 0; k < Kc; ++k) {
                    const float x3 = x[k + 3], wk = w[k];
                    a0 += wk * x0; a1 += wk * x1; a2 += wk * x2; a3 += wk * x3;
                    x0 = x1; x1 = x2; x2 = x3;
                }
            }
            loc[j0 * F1 + f] = a0;
            if (j0 + 1 < Tin) loc[(j0 + 1) * F1 + f] = a1;
            if (j0 + 2 < Tin) loc[(j0 + 2) * F1 + f] = a2;
            if (j0 + 3 < Tin) loc[(j0 + 3) * F1 + f] = a3;
        }
        for (int j = tid; j < Tin; j += NT) loc[j * F1 + F] = 0.f;      // pad column (K rounded up to even for the MFMA)
        if (paS) {
            // location features through the dense layer on the matrix cores: pa[j][a] = sum_f loc[j][f] * Wd[a][f]
            // (exact fp32 fma chains, v_mfma_f32_32x32x2_f32), one 32x32 tile per wave
            __syncthreads();
            const int wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
            const int njt = (Tin + 31) / 32, nat = A / 32, Ke = (F + 1) & ~1;
            for (int tile = wave; tile < njt * nat; tile += NT / 64) {
                const int jt = tile / nat, at = tile % nat;
                const float* lr = loc + min(jt * 32 + r, Tin - 1) * F1 + h;
                const float* dr = dense + (at * 32 + r) * F1 + h;
                f32x16 acc;
#pragma unroll
                for (int e2 = 0; e2 < 16; ++e2) acc[e2] = 0.f;
                for (int kk = 0; kk < Ke; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lr[kk], dr[kk], acc, 0, 0, 0);
#pragma unroll
                for (int e2 = 0; e2 < 16; ++e2) {
                    const int row = jt * 32 + (e2 & 3) + 8 * (e2 >> 2) + 4 * h;
                    if (row < Tin) paS[row * PA + at * 32 + r] = acc[e2];
                }
            }
        }
    }
    __syncthreads();

    T2_ASTAMP(0, 1);
    // ---- energies: 16 lanes per position j
    {
        const int gid = tid >> 4, sub = tid & 15;
        auto chunk = [&](int j, int a, const f32x4 pv) {      // 4 channels of position j
            float part = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float u = q[a + c] + pv[c];
                if (d.kind == AttnKind::LSA) {
                    if (paS) u += paS[j * PA + a + c];
                    else {
                        float pa = 0.f;
                        const float* dr = dense + (a + c) * F1;
                        const float* lr = loc + j * F1;
                        for (int f = 0; f < F; ++f) pa += dr[f] * lr[f];
                        u += pa;
                    }
                }
                part += vs[a + c] * tanhf(u);
            }
            return part;
        };
        auto finish = [&](int j, float sum) {
            sum += __shfl_xor(sum, 8, 64); sum += __shfl_xor(sum, 4, 64);
            sum += __shfl_xor(sum, 2, 64); sum += __shfl_xor(sum, 1, 64);
            if (sub == 0 && j < Tin) e[j] = sum;
        };
#pragma unroll
        for (int i = 0; i < PFJ; ++i) {                       // prefetched positions (whole 16-lane groups stay converged)
            const int j = gid + i * (NT / 16);
            if (j < Tp) {
                float sum = 0.f;
                if (j < Tin) {
#pragma unroll
                    for (int k = 0; k < PFA; ++k) if (sub * 4 + 64 * k < A) sum += chunk(j, sub * 4 + 64 * k, pmv[i][k]);
                    const float* pmr = st.pm + ((long)b * Tin + j) * A;
                    for (int a = sub * 4 + 64 * PFA; a < A; a += 64) sum += chunk(j, a, *reinterpret_cast<const f32x4*>(pmr + a));
                }
                finish(j, sum);
            }
        }
        for (int j = gid + PFJ * (NT / 16); j < Tp; j += NT / 16) {
            float sum = 0.f;
            if (j < Tin) {
                const float* pmr = st.pm + ((long)b * Tin + j) * A;
                for (int a = sub * 4; a < A; a += 64) sum += chunk(j, a, *reinterpret_cast<const f32x4*>(pmr + a));
            }
            finish(j, sum);
        }
    }
    __syncthreads();

    T2_ASTAMP(0, 2);
    int len = st.lengths ? st.lengths[b] : Tin;
    if (d.max_pos > 0) len = min(len, d.max_pos);
    if (d.kind == AttnKind::SMA) {
        const RngKey key = rng_key(d.seed, st.site_noise);
        for (int j = tid; j < Tin; j += NT) {
            float ev = e[j];
            if (j >= len) ev = st.mask_value;
            if (d.noise_std > 0.f) ev += d.noise_std * rng_normal(key, st.idx_base + (uint32_t)b * st.idx_bstride + (uint32_t)j);
            const float p = sigmoidf_(ev);
            e[j] = p;
            if (st.p_out) st.p_out[(long)b * st.ldp_out + j] = p;
        }
        __syncthreads();
        for (int j = tid; j < Tin; j += NT) {
            float a = ap[j] * e[j];
            if (j > 0) a += ap[j - 1] * (1.0f - e[j - 1]);
            an[j] = a;
            st.a_out[(long)b * st.lda_out + j] = a;
        }
    } else {
        float mx = -INFINITY;
        for (int j = tid; j < Tin; j += NT) {
            float ev = e[j];
            if (j >= len) ev = st.mask_value;
            e[j] = ev;
            mx = fmaxf(mx, ev);
        }
        mx = block_reduce(mx, red, true);
        float sum = 0.f;
        for (int j = tid; j < Tin; j += NT) { const float x = expf(e[j] - mx); e[j] = x; sum += x; }
        sum = block_reduce(sum, red, false);
        const float inv = 1.0f / sum;
        for (int j = tid; j < Tin; j += NT) {
            const float w = e[j] * inv;
            an[j] = w;
            st.a_out[(long)b * st.lda_out + j] = w;
            if (st.wcum_out)
                st.wcum_out[(long)b * st.ldwcum_out + j] = (st.wcum_prev ? st.wcum_prev[(long)b * st.ldwcum_prev + j] : 0.f) + w;
        }
    }
    __syncthreads();

    T2_ASTAMP(0, 3);
    // ---- context: nh groups of nd lanes, each lane 4 channels; group h takes j = jlo+h, jlo+h+nh, ...
    // Only the band [jlo, jhi) of non-zero weights is read (an SMA alignment is a narrow band that
    // starts one-hot; exact zeros contribute nothing), with no branch inside the unrolled loop.
    {
        int lo = Tin, hi = 0;
        for (int j = tid; j < Tin; j += NT) if (an[j] != 0.f) { lo = min(lo, j); hi = max(hi, j + 1); }
        lo = -(int)block_reduce(-(float)lo, red, true);
        hi = (int)block_reduce((float)hi, red, true);
        const int h = tid / nd, dd = (tid % nd) * 4;
        if (h < nh) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const float* mp = st.memory + (long)b * Tin * E + dd;
#pragma unroll 8
            for (int j = lo + h; j < hi; j += nh) {
                const f32x4 mv = *reinterpret_cast<const f32x4*>(mp + (long)j * E);
                acc += an[j] * mv;
            }
            *reinterpret_cast<f32x4*>(cred + h * E + dd) = acc;
        }
        __syncthreads();
        T2_ASTAMP(0, 4);
        for (int c = tid; c < E; c += NT) {
            float sum = 0.f;
            for (int h2 = 0; h2 < nh; ++h2) sum += cred[h2 * E + c];
            st.ctx1[(long)b * st.ldctx1 + c] = sum;
            if (st.ctx2) st.ctx2[(long)b * st.ldctx2 + c] = sum;
            if (st.ctx16) st.ctx16[(long)b * st.ldctx16 + c] = (__bf16)sum;
            if (st.ctx16b) st.ctx16b[(long)b * st.ldctx16b + c] = (__bf16)sum;
        }
    }
    T2_ASTAMP(0, 5);
}


// ---------------------------------------------------------------------------------------------
// Backward of one StepwiseMonotonicAttention step (reverse time), one workgroup per (b, stream).
//   dctx   = direct sources + recurrent partials                      (saved: feeds d(memory) GEMM)
//   g_j    = dctx . memory_j + dalign_j + carry_j                     total gradient on a_t[j]
//   dp_j   = a_{t-1}[j] (g_j - g_{j+1}) ;  de_j = dp_j p_j (1 - p_j)
//   u_jk   = tanh(q_k + pm_jk) ;  dpre_jk = de_j v_k (1 - u_jk^2)
//   dq_k   = sum_j dpre_jk ; dv_k += sum_j de_j u_jk ; dpm_jk += dpre_jk
//   carry_out_j = g_j p_j + g_{j+1} (1 - p_j)                         gradient on a_{t-1}[j]
// ---------------------------------------------------------------------------------------------

// The memory positions of an item can be split over d.nsplit workgroups (blockIdx.z): each takes a contiguous range
// [jb, je), recomputes the (cheap) total ctx gradient, needs one extra g value at je for the recurrence, and emits its
// own partial of dq / dv (consumers add the partials).  With B*2 = 128 workgroups the kernel was bound by what one CU
// can pull from L2/MALL (~0.36 MB per item); two workgroups per item use all 256 CUs.
template <int MAXI>
__global__ __launch_bounds__(NTB) void attention_step_bwd_kernel(AttnBwdDesc d) {
    const AttnBwdStream& st = d.st[blockIdx.y];
    const int b = blockIdx.x, tid = threadIdx.x, split = blockIdx.z;
    const int Tin = st.Tin, A = d.A, E = d.E;
    const int chunk = (((Tin + d.nsplit - 1) / d.nsplit) + 3) & ~3;
    const int jb = min(split * chunk, Tin), je = min(jb + chunk, Tin), len = je - jb;
    const int ng = je < Tin ? len + 1 : len;          // g values computed here: positions [jb, jb + ng)
    const int Tp = chunk + 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* dctx = smem;              // [E]
    float* q = dctx + E;             // [A]
    float* vs = q + A;               // [A]
    float* g = vs + A;               // [Tp]  g[jl] = g_{jb+jl}; g[len] = g_{je} (0 past the end)
    float* de = g + Tp;              // [Tp]
    float* ps = de + Tp;             // [Tp]
    float* red = ps + Tp;            // [NT/16][A] x 2 (dq, dv partials of the NT/16 position groups)

    T2_ASTAMP(8, 0);
    // the first batch of memory rows of the g pass (4 positions x 2 x 256 channels per wave) is requested before the
    // ctx gradient is assembled: the rows do not depend on it
    constexpr int GU = 4, GC = 2;
    f32x4 mpre[GC][GU];
    {
        const int wave = tid >> 6, lane = tid & 63;
        const int ngp = max((je < Tin ? je - jb + 1 : je - jb), 1);
#pragma unroll
        for (int cc = 0; cc < GC; ++cc)
#pragma unroll
            for (int u = 0; u < GU; ++u)
                mpre[cc][u] = *reinterpret_cast<const f32x4*>(st.memory + ((long)b * Tin + min(jb + min(wave + u * (NTB / 64), ngp - 1), Tin - 1)) * E + min(lane * 4 + 256 * cc, E - 4));
    }

    for (int c = tid; c < E; c += NTB) {
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) if (st.dctx[i]) v += st.dctx[i][(long)b * st.lddctx[i] + c];
        if (st.part && !d.first) {
            const float* p = st.part + (long)b * st.ldpart + st.part_col + c;
            float pv[8];                              // all K-split partials requested at once (nparts <= 8)
#pragma unroll
            for (int z = 0; z < 8; ++z) pv[z] = z < st.nparts ? p[(long)z * st.part_stride] : 0.f;
            float acc = 0.f;
#pragma unroll
            for (int z = 0; z < 8; ++z) acc += pv[z];
            v += acc;
        }
        dctx[c] = v;
        if (split == 0) st.dctx_out[(long)b * st.lddctx_out + c] = v;
    }
    for (int a = tid; a < A; a += NTB) { q[a] = st.q[(long)b * st.ldq + a]; vs[a] = st.v[a]; }
    for (int jl = tid; jl < len; jl += NTB) ps[jl] = st.p[(long)b * st.ldp + jb + jl];
    if (tid == 0) g[len] = 0.f;
    __syncthreads();
    if (len == 0) {                                   // (only when Tin is tiny) nothing to do but the partial outputs
        for (int a = tid; a < A; a += NTB) {
            st.dq_out[(long)b * st.lddq_out + split * A + a] = 0.f;
            float* dvp = st.dv_acc + ((long)split * d.B + b) * A + a;
            if (d.first) *dvp = 0.f;
        }
        return;
    }

    T2_ASTAMP(8, 1);
    // g_j: one wave per position, lanes stride the E channels 16 B at a time; 4 positions are in
    // flight per wave so that the row loads overlap instead of serialising on L2 latency
    {
        const int wave = tid >> 6, lane = tid & 63;
        constexpr int NWV = NTB / 64, U = 4;
        static_assert(U == GU, "prefetch shape");
        for (int j0 = wave; j0 < ng; j0 += NWV * U) {
            float sum[U] = {0.f, 0.f, 0.f, 0.f};
            int cc = 0;
            for (int c = lane * 4; c < E; c += 256, ++cc) {
                const f32x4 dc = *reinterpret_cast<const f32x4*>(dctx + c);
                f32x4 mv[U];
                const bool pre = j0 == wave && cc < GC;      // wave-uniform
#pragma unroll
                for (int u = 0; u < U; ++u) {           // clamp instead of branching: the U loads issue back to back
                    const int j = jb + min(j0 + u * NWV, ng - 1);
                    if (pre) mv[u] = cc == 0 ? mpre[0][u] : mpre[1][u];
                    else mv[u] = *reinterpret_cast<const f32x4*>(st.memory + ((long)b * Tin + j) * E + c);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) sum[u] += mv[u][0] * dc[0] + mv[u][1] * dc[1] + mv[u][2] * dc[2] + mv[u][3] * dc[3];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int jl = j0 + u * NWV;
                const float tot = wave_sum(sum[u]);
                if (lane == 0 && jl < ng) {
                    const int j = jb + jl;
                    float gsum = tot;
                    if (st.dalign) gsum += st.dalign[(long)b * st.lddalign + j];
                    if (!d.first) gsum += st.carry[(long)b * Tin + j];
                    g[jl] = gsum;
                }
            }
        }
    }
    __syncthreads();
    T2_ASTAMP(8, 2);
    // carry is read at position je too, which the next split's workgroup updates: the new carry therefore goes to a
    // second buffer (carry / carry_out swap roles every step)
    for (int jl = tid; jl < len; jl += NTB) {
        const int j = jb + jl;
        const float ap = st.a_prev ? st.a_prev[(long)b * st.lda_prev + j] : (j == 0 ? 1.f : 0.f);
        const float p = ps[jl];
        const float gj = g[jl], gn = g[jl + 1];
        de[jl] = ap * (gj - gn) * p * (1.0f - p);
        st.carry_out[(long)b * Tin + j] = gj * p + gn * (1.0f - p);
    }
    __syncthreads();

    T2_ASTAMP(8, 3);
    // energies backward: 16 lanes per position, each lane owns channels sub*4 + 64*i
    {
        const int gid = tid >> 4, sub = tid & 15;
        float dq[MAXI][4], dv[MAXI][4];
#pragma unroll
        for (int i = 0; i < MAXI; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) { dq[i][c] = 0.f; dv[i][c] = 0.f; }
        for (int jl = gid; jl < len; jl += NTB / 16) {
            const float dej = de[jl];
            const float* pmr = st.pm + ((long)b * Tin + jb + jl) * A;
            float* dpr = st.dpm_acc + ((long)b * Tin + jb + jl) * A;
#pragma unroll
            for (int i = 0; i < MAXI; ++i) {
                const int a = sub * 4 + 64 * i;
                if (a < A) {
                    const f32x4 pv = *reinterpret_cast<const f32x4*>(pmr + a);
                    f32x4 acc = d.first ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(dpr + a);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float u = tanhf(q[a + c] + pv[c]);
                        const float dpre = dej * vs[a + c] * (1.0f - u * u);
                        dq[i][c] += dpre;
                        dv[i][c] += dej * u;
                        acc[c] += dpre;
                    }
                    *reinterpret_cast<f32x4*>(dpr + a) = acc;
                }
            }
        }
        T2_ASTAMP(8, 4);
        float* rq = red;
        float* rv = red + (NTB / 16) * A;
#pragma unroll
        for (int i = 0; i < MAXI; ++i) {
            const int a = sub * 4 + 64 * i;
            if (a < A) {
#pragma unroll
                for (int c = 0; c < 4; ++c) { rq[gid * A + a + c] = dq[i][c]; rv[gid * A + a + c] = dv[i][c]; }
            }
        }
        __syncthreads();
        for (int a = tid; a < A; a += NTB) {
            float sq = 0.f, sv = 0.f;
            for (int k = 0; k < NTB / 16; ++k) { sq += rq[k * A + a]; sv += rv[k * A + a]; }
            st.dq_out[(long)b * st.lddq_out + split * A + a] = sq;
            float* dvp = st.dv_acc + ((long)split * d.B + b) * A + a;
            *dvp = (d.first ? 0.f : *dvp) + sv;
        }
    }
    T2_ASTAMP(8, 5);
}
}  // namespace

// LDS bytes of attention_step_fwd_kernel for the longest memory Tmax (with_pa: the matrix-core tile of the LSA dense projection)
static size_t attention_fwd_smem(const AttnStepDesc& d, int Tmax, bool with_pa) {
    const int Tp = (Tmax + 3) & ~3;
    const int nh = NT / (d.E / 4);
    size_t n = 2 * d.A + 3 * Tp + 4 * NT + (size_t)nh * d.E;
    if (d.kind == AttnKind::LSA) {
        const int TwP = (Tmax + d.Kc - 1 + 4 + 3) & ~3;
        n += (size_t)d.F * 2 * d.Kc + (size_t)d.A * (d.F + 1) + (((size_t)Tmax * (d.F + 1) + 3) & ~(size_t)3) + 2 * (size_t)TwP;
        if (with_pa) n += (size_t)Tmax * (d.A + 8);
    }
    return n * sizeof(float);
}

int attention_step_fwd(const AttnStepDesc& din, hipStream_t s) {
    AttnStepDesc d = din;
    if (d.kind == AttnKind::DCA) {
        T2_REQUIRE(d.nstreams >= 1 && d.nstreams <= 2 && d.A % 4 == 0 && d.A <= 256 && NT % (d.A / 4) == 0 && d.E % 4 == 0 && NT % (d.E / 4) == 0,
                   "attention_step (DCA): A=%d E=%d unsupported", d.A, d.E);
        for (int i = 0; i < d.nstreams; ++i) {
            const DcaWeights& w = d.st[i].dca;
            T2_REQUIRE(d.st[i].qpart && w.bW && w.V && w.F && w.U && w.T && w.bT && w.v && w.P, "attention_step (DCA): missing weights");
        }
        return attention_dca_fwd_launch(d, attention_tmax(d.st, d.nstreams), s);
    }
    if (d.kind == AttnKind::GMM) {
        T2_REQUIRE(d.nstreams >= 1 && d.nstreams <= 2 && d.A % 4 == 0 && d.A <= 256 && NT % (d.A / 4) == 0 && d.E % 4 == 0 && NT % (d.E / 4) == 0,
                   "attention_step (GMM): A=%d E=%d unsupported", d.A, d.E);
        for (int i = 0; i < d.nstreams; ++i)
            T2_REQUIRE(d.st[i].qpart && d.st[i].gmm_b1 && d.st[i].gmm_w2 && d.st[i].gmm_b2 && d.st[i].mu_out, "attention_step (GMM): missing buffers");
        return attention_gmm_fwd_launch(d, attention_tmax(d.st, d.nstreams), s);
    }
    const bool lsa = d.kind == AttnKind::LSA;
    T2_REQUIRE(d.nstreams >= 1 && d.nstreams <= 2, "attention_step: nstreams=%d", d.nstreams);
    T2_REQUIRE(d.A % 4 == 0 && d.A <= 256 && NT % (d.A / 4) == 0, "attention_step: attention_dim %d must be a multiple of 4 dividing %d, <= 256", d.A, 4 * NT);
    T2_REQUIRE(d.E % 4 == 0 && d.E / 4 <= NT && NT % (d.E / 4) == 0, "attention_step: encoder dim %d unsupported", d.E);
    T2_REQUIRE(d.kind == AttnKind::SMA || (d.Kc % 2 == 1 && d.F >= 1), "attention_step: bad location layer F=%d Kc=%d", d.F, d.Kc);
    for (int i = 0; i < d.nstreams; ++i)
        T2_REQUIRE(((uintptr_t)d.st[i].pm & 15) == 0 && ((uintptr_t)d.st[i].memory & 15) == 0, "attention_step: pm/memory must be 16-byte aligned");
    const int Tmax = attention_tmax(d.st, d.nstreams);
    // LSA: the dense location projection runs on the matrix cores when its [T_in][A] tile fits in LDS beside the rest
    d.lsa_pa = lsa && d.A % 32 == 0 && attention_fwd_smem(d, Tmax, true) <= 160 * 1024;
    return attention_launch(attention_step_fwd_kernel, dim3(d.B, d.nstreams), NT, attention_fwd_smem(d, Tmax, d.lsa_pa), d, s, "attention_step");
}

int attention_step_bwd(const AttnBwdDesc& d, hipStream_t s) {
    T2_REQUIRE(d.nstreams >= 1 && d.nstreams <= 2, "attention_bwd: nstreams=%d", d.nstreams);
    T2_REQUIRE(d.A % 4 == 0 && d.A <= 256 && d.E % 4 == 0, "attention_bwd: A=%d E=%d unsupported", d.A, d.E);
    const int Tmax = attention_tmax(d.st, d.nstreams);
    if (d.kind == AttnKind::DCA) {
        for (int i = 0; i < d.nstreams; ++i) {
            const DcaWeights& w = d.st[i].dca;
            T2_REQUIRE(d.st[i].w && d.st[i].dca_acc && w.V && w.F && w.U && w.T && w.bT && w.v && w.P, "attention_bwd (DCA): missing buffers");
        }
        return attention_dca_bwd_launch(d, Tmax, s);
    }
    if (d.kind == AttnKind::GMM) {
        for (int i = 0; i < d.nstreams; ++i)
            T2_REQUIRE(d.st[i].w && d.st[i].gmm_w2 && d.st[i].gmm_b2 && d.st[i].mu && d.st[i].mu_carry && d.st[i].dw2_acc && d.st[i].db2_acc,
                       "attention_bwd (GMM): missing buffers");
        return attention_gmm_bwd_launch(d, Tmax, s);
    }
    if (d.kind == AttnKind::LSA) {
        T2_REQUIRE(d.Kc % 2 == 1 && d.F >= 1 && d.F <= 32, "attention_bwd (LSA): location layer F=%d (<= 32) Kc=%d (odd) unsupported", d.F, d.Kc);
        for (int i = 0; i < d.nstreams; ++i)
            T2_REQUIRE(d.st[i].w && d.st[i].carry_cum && d.st[i].dconv_acc && d.st[i].ddense_acc && d.st[i].loc_conv && d.st[i].loc_dense,
                       "attention_bwd (LSA): missing buffers");
        return attention_lsa_bwd_launch(d, Tmax, s);
    }
    T2_REQUIRE(d.nsplit >= 1 && d.nsplit <= 4, "attention_bwd: nsplit=%d", d.nsplit);
    for (int i = 0; i < d.nstreams; ++i) T2_REQUIRE(d.st[i].carry_out && d.st[i].carry_out != d.st[i].carry, "attention_bwd: carry_out must be a second buffer");
    const int chunk = (((Tmax + d.nsplit - 1) / d.nsplit) + 3) & ~3;
    const size_t smem = ((size_t)d.E + 2 * d.A + 3 * (size_t)(chunk + 4) + 2 * (NTB / 16) * (size_t)d.A) * sizeof(float);
    return attention_launch(d.A <= 128 ? attention_step_bwd_kernel<2> : attention_step_bwd_kernel<4>, dim3(d.B, d.nstreams, d.nsplit), NTB, smem, d, s,
                            "attention_bwd");
}

}  // namespace t2
