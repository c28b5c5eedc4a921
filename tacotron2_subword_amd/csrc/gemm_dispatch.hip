// The host side of gemm(): the process-wide settings and counters, the checks, the pure plan (plan_gemm), the executor that
// launches what the plan names (the kernel families' launchers: gemm_common.h), and the split-K reduce.
#include "gemm_common.h"
#include <cstdlib>
#include <algorithm>

namespace t2 {

using namespace gemm_detail;

static int g_precision = 0;       // 0: fp32 operands (parity path), 1: bf16 operands for large GEMMs, 2: split-bf16 (hi + lo) operands
// bf16 mode: stage fp32 operands as bf16 copies when both extents reach kStageMin (T2_GEMM_STAGE=0 switches it off)
static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v && *v ? atoi(v) : dflt; }
static int g_stage = env_int("T2_GEMM_STAGE", 1);
void set_gemm_staging(int on) { g_stage = on != 0; }
static int g_fold = env_int("T2_GEMM_FOLD", 1);
void set_gemm_fold(int on) { g_fold = on != 0; }
int get_gemm_fold() { return g_fold; }
constexpr int kStageMin = 256;
// split-bf16 mode: a product whose 2*M*N*K is below this many MFLOP runs the exact fp32 kernel instead: three staged terms
// and two staging launches cost 20 - 50 us whatever the shape, which the exact kernel beats up to about 2 GFLOP
// (break-even between 1.6 and 5.4 GFLOP: profiles/r05_split_threshold.txt).  set_gemm_split_min_mflop()
// changes it (tests of the kernels on small shapes set 0).
constexpr int kSplitMinMflopDefault = 2147;          // 2^31 FLOP
static double g_split_min_flop = 1e6 * kSplitMinMflopDefault;
void set_gemm_split_min_mflop(int mflop) { g_split_min_flop = 1e6 * (mflop < 0 ? kSplitMinMflopDefault : mflop); }
void set_precision(int p) { g_precision = p; }
int get_precision() { return g_precision; }
GemmEnv gemm_env_here() {
    static const int t256 = env_int("T2_GEMM_256", 1);
    return GemmEnv{g_precision, g_stage != 0, t256 != 0, g_split_min_flop};
}
// calls of gemm() by kernel family: exact fp32, converting bf16, bf16-source on single-bf16 operands, bf16-source on split operands
static uint64_t g_counts[4] = {0, 0, 0, 0};
void gemm_counts(uint64_t* out, int reset) {
    for (int i = 0; i < 4; ++i) { out[i] = g_counts[i]; if (reset) g_counts[i] = 0; }
}

namespace {

__global__ void splitk_reduce_kernel(GemmDesc d) {
    const long total = (long)d.batch * d.M * d.N;
    const RngKey key = rng_key(d.seed, d.site);
    with_col_map(d, [&](auto cmap) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        float acc = 0.f;                                   // partials requested 8 at a time, added in split order
        int s = 0;
        for (; s + 8 <= d.splitk; s += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = d.ws[(long)(s + j) * total + i];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += v[j];
        }
        if (s + 4 <= d.splitk) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = d.ws[(long)(s + j) * total + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += v[j];
            s += 4;
        }
        for (; s < d.splitk; ++s) acc += d.ws[(long)s * total + i];
        const int bz = (int)(i / ((long)d.M * d.N));
        const long rem = i - (long)bz * d.M * d.N;
        const int m = (int)(rem / d.N), n = (int)(rem % d.N);
        epilogue_store<decltype(cmap)::value>(d, d.C + (long)bz * d.bsC, m, n, acc, key);
    }
    });
}

inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

int check_gemm(const GemmDesc& d) {
    T2_REQUIRE(d.M > 0 && d.N > 0 && d.K > 0 && d.batch > 0, "gemm: bad shape M=%d N=%d K=%d batch=%d", d.M, d.N, d.K, d.batch);
    T2_REQUIRE(d.act >= ACT_NONE && d.act <= ACT_GELU, "gemm: unknown activation act=%d (0 none, 1 relu, 2 tanh, 3 gelu)", d.act);
    if (d.conv_a || d.conv_b) {
        T2_REQUIRE(d.conv_T > 0 && d.conv_C > 0 && d.conv_C % 4 == 0 && !(d.conv_a && d.conv_b), "gemm: bad implicit-conv operand (T=%d C=%d)", d.conv_T, d.conv_C);
        T2_REQUIRE(d.batch == 1, "gemm: implicit-conv operands need batch == 1");
        if (d.conv_a) T2_REQUIRE(d.K % d.conv_C == 0 && aligned16(d.A), "gemm: conv A operand: K=%d C=%d", d.K, d.conv_C);
        if (d.conv_b) T2_REQUIRE(d.N % d.conv_C == 0 && aligned16(d.B), "gemm: conv B operand: N=%d C=%d", d.N, d.conv_C);
    }
    T2_REQUIRE(d.conv_a || d.sam == 1 || d.sak == 1, "gemm: A needs one unit stride (sam=%ld sak=%ld)", d.sam, d.sak);
    T2_REQUIRE(d.conv_b || d.sbn == 1 || d.sbk == 1, "gemm: B needs one unit stride (sbn=%ld sbk=%ld)", d.sbn, d.sbk);
    T2_REQUIRE(d.ccol_mod >= 0 && d.ccol_mul >= 0 && (!d.ccol_mod || (d.N % d.ccol_mod == 0 && (long)d.ccol_mul * d.ccol_mod >= d.N && (long)d.ccol_mul * d.ccol_mod <= d.ldc)),
               "gemm: bad column map (N=%d mod=%d mul=%d)", d.N, d.ccol_mod, d.ccol_mul);
    T2_REQUIRE(!d.r1_m == !d.r1_n && (!d.r1_m || d.batch == 1), "gemm: the rank-1 addend needs both vectors and batch == 1");
    T2_REQUIRE(d.drop_p == 0.f || (d.batch == 1 && (long)d.M * d.N < (1l << 32)), "gemm: dropout epilogue needs batch==1 and M*N < 2^32");
    return 0;
}

// The split-K factor of a kernel family (`tiles` workgroups without it, kch 16-wide K-chunks), clamped by the scratch
int choose_splitk(const GemmDesc& d, bool tile256, long tiles, int kch, size_t ws_bytes) {
    if (!(d.ws && d.beta == 0.f)) return 1;
    int sp = 1;
    if (tile256) {
        // the 256-tile kernels: the factor that fills whole rounds of one workgroup per CU (a forced one leaves two K-tiles per split)
        const int nkt = kch / 4;
        if (d.splitk > 0) sp = std::min(d.splitk, std::max(1, nkt / 2));
        else if (tiles < 512) {
            double best = 0.0;
            for (int c = 1; c <= 16; ++c) {
                if (c > 1 && nkt / c < 16) break;
                const long wgs = tiles * c, rounds = (wgs + 255) / 256;
                const double eff = (double)wgs / (256.0 * rounds);
                if (eff > best * 1.05) { best = eff; sp = c; }
            }
        }
    } else if (d.splitk > 0) sp = d.splitk;
    // fewer than two tile-waves over the 256 CUs and a long K: split so that every CU holds several workgroups
    // (a lone 128x128 workgroup per CU cannot cover its own operand latency)
    else if (tiles < 512 && kch >= 64) sp = std::min((int)((1024 + tiles - 1) / tiles), kch / 16);
    const size_t per = (size_t)d.batch * d.M * d.N * sizeof(float);
    if ((size_t)sp * per > ws_bytes) sp = (int)(ws_bytes / per);
    return std::max(sp, 1);
}

int run_gemm(const GemmDesc& d, const GemmPlan& p, hipStream_t s) {
    // the descriptor as the kernels take it: the plan's K / conv_C / splitk, the partials behind the staged copies, the
    // implied strides of an implicit-conv operand and the default dropout row stride filled in
    GemmK g{};
    g.d = d;
    g.kchunks = p.kchunks; g.avec = p.avec; g.bvec = p.bvec;
    if (d.conv_a) { g.d.sam = 0; g.d.sak = 1; }
    if (d.conv_b) { g.d.sbk = 0; g.d.sbn = 1; }
    if (d.drop_mstride == 0) g.d.drop_mstride = (uint32_t)d.N;
    g.d.K = p.K; g.d.conv_C = p.conv_C; g.d.splitk = p.splitk;
    const size_t staged = p.a.bytes + p.b.bytes;
    if (staged) { g.d.ws = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(d.ws) + staged); g.d.ws_bytes = d.ws_bytes - staged; }
    const int tile = p.kernel == GemmKernel::f32_64 ? 64 : p.kernel >= GemmKernel::src256 ? 256 : 128;
    const dim3 grid((d.N + tile - 1) / tile, (d.M + tile - 1) / tile, d.batch * p.splitk);
    if (gemm_reads_bf16_copies(p.kernel)) {
        // both operands as bf16 copies: the caller's, or staged in front of the split-K scratch
        __bf16* a16 = reinterpret_cast<__bf16*>(d.ws), * b16 = reinterpret_cast<__bf16*>(reinterpret_cast<unsigned char*>(d.ws) + p.a.bytes);
        if (p.a.src == GemmSrc::staged) T2_TRY_RC(stage_planned(d.A, p.a, p.split, a16, s));
        if (p.b.src == GemmSrc::staged) T2_TRY_RC(stage_planned(d.B, p.b, p.split, b16, s));
        const __bf16* pa = p.a.src == GemmSrc::caller ? d.A16 : a16, * pb = p.b.src == GemmSrc::caller ? d.B16 : b16;
        T2_TRY_RC(launch_gemm_bf16src(g, p.kernel, pa, p.a.ld, pb, p.b.ld, grid, s));
    } else if (p.kernel == GemmKernel::bf16conv) {
        T2_TRY_RC(launch_gemm_bf16conv(g, grid, s));
    } else {
        T2_TRY_RC(launch_gemm_f32(g, p.kernel, grid, s));
    }
    if (p.splitk > 1) {
        const long total = (long)d.batch * d.M * d.N;
        int blocks = (int)((total + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, s, g.d);
        T2_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

const char* gemm_plan_name(const GemmPlan& p) {
    static const char* const names[] = {"f32_64", "f32_128", "bf16conv", "src128", "src256", "src256km", "x3src128", "x3src256", "x3src256km"};
    return names[(int)p.kernel + (p.split ? 3 : 0)];
}

GemmPlan plan_gemm(const GemmDesc& d) { return plan_gemm(d, gemm_env_here()); }

GemmPlan plan_gemm(const GemmDesc& d, const GemmEnv& e) {
    GemmPlan p{};
    const bool conv_any = d.conv_a || d.conv_b;
    const bool akc = d.conv_a || d.sak == 1, bkc = !d.conv_b && d.sbk == 1;   // K is the contiguous stride (conv: A's frames are rows, B's are k-rows)
    const long lda = d.conv_a ? d.conv_C : akc ? d.sam : d.sak;               // leading dimension of the fp32 operand (conv: of the frames)
    const long ldb = d.conv_b ? d.conv_C : bkc ? d.sbn : d.sbk;
    p.avec = aligned16(d.A) && d.bsA % 4 == 0 && lda % 4 == 0;
    p.bvec = aligned16(d.B) && d.bsB % 4 == 0 && ldb % 4 == 0;
    p.K = d.K; p.conv_C = d.conv_C;

    // bf16-operand mode: large GEMMs only (both extents >= 64), conv operands need C % 8 == 0
    const bool large = !d.fp32_only && d.M >= 64 && d.N >= 64 && d.K >= 64 && (!conv_any || d.conv_C % 8 == 0);
    const bool use_bf16 = e.precision == 1 && large;
    // split-bf16 mode: only the bf16-source kernels, on operands staged as hi / lo parts (K' = 3K, see the staging casts of gemm.hip);
    // whatever does not qualify for them below runs exactly what mode 0 runs.  Single-bf16 copies from the caller are not
    // used; split16 marks copies that are already in the split layout of this product (t2_prof_gemm).
    const bool want_split = e.precision == 2 && large && 2.0 * d.M * d.N * d.K >= e.split_min_flop;
    const int kmul = want_split ? 3 : 1;
    const bool copies = e.precision != 2 || (want_split && d.split16);
    bool a_caller = copies && d.A16, b_caller = copies && d.B16;
    // 256 x 256 tiles (gemm_bf16src256_kernel) when the staged operands are whole 256-tiles and K splits into an even
    // number of 64-wide K-tiles.  Its k-major variant reads both operands as they lie in memory when BOTH are k-major
    // (the weight-gradient products): they are staged by the plain cast, [K][M] and [K][N]; an implicit-conv B operand
    // is then the bf16 copy of the frames [K][C] alone.  A bf16 copy the caller hands over in the layout the product
    // does not take is ignored (the fp32 operand is staged instead).
    const bool shape256 = e.tiles256 && d.M % 256 == 0 && d.N % 256 == 0 && d.K >= 128;
    const long ld_km = std::max(std::max((long)d.M, a_caller && d.a16_kmajor ? d.lda16 : 0l), std::max((long)(d.conv_b ? d.conv_C : d.N), b_caller && d.b16_kmajor ? d.ldb16 : 0l));
    const bool km = shape256 && !akc && !bkc && !d.conv_a && (!d.conv_b || d.conv_C % 256 == 0) && (long)d.K * kmul * ld_km * 2 < (1l << 31);
    a_caller = a_caller && (d.a16_kmajor != 0) == km;
    b_caller = b_caller && (d.b16_kmajor != 0) == km;
    // (split: the k-major conv_b copies are three whole stacks of the frames, so the stack height must keep k % conv_T)
    // conv_a: a caller copy of A is the bf16 frames [M][conv_C], exactly what gemm() would stage (any other pitch is ignored);
    // the kernel's buffer resource spans M * conv_C elements and relies on rows outside it reading zero.  Split copies of a
    // conv_a product have a layout of their own (3C channels per tap): with them the product stays on the exact kernel
    a_caller = a_caller && (!d.conv_a || d.lda16 == d.conv_C);
    const bool conv_ok = !conv_any || (d.conv_a && d.conv_C % 64 == 0 && (!want_split || (!a_caller && !b_caller))) ||
                         (d.conv_b && km && (!want_split || d.K % d.conv_T == 0));
    // bf16-source kernels: both operands staged as bf16 in front of the split-K scratch (or handed over by the caller);
    // pays when each staged element is reused by many tiles, i.e. when both extents are large
    bool staged = false;
    size_t ws_bytes = d.ws_bytes;                           // what is left for the split-K partials
    if ((use_bf16 || want_split) && e.stage && conv_ok && d.batch == 1 && d.M % 128 == 0 && d.N % 128 == 0 && d.K % 64 == 0) {
        // implicit-conv operands: only the frames [rows][C] are staged (the kernel shifts rows per tap)
        const size_t a_elems = d.conv_a ? (size_t)d.M * d.conv_C : (size_t)d.M * d.K;
        const size_t b_elems = d.conv_b ? (size_t)d.K * d.conv_C : (size_t)d.N * d.K;
        const size_t need_a = a_caller ? 0 : round256(kmul * a_elems * sizeof(__bf16));
        const size_t need_b = b_caller ? 0 : round256(kmul * b_elems * sizeof(__bf16));
        const bool big = (a_caller || d.N >= kStageMin) && (b_caller || d.M >= kStageMin);
        const bool ok_src = (a_caller ? aligned16(d.A16) && d.lda16 % 8 == 0 : p.avec != 0) && (b_caller ? aligned16(d.B16) && d.ldb16 % 8 == 0 : p.bvec != 0);
        if (big && ok_src && (need_a + need_b == 0 || (d.ws && aligned16(d.ws) && d.ws_bytes >= need_a + need_b))) {
            staged = true;
            p.a.bytes = need_a; p.b.bytes = need_b;
            ws_bytes -= need_a + need_b;
        }
    }
    // split operands: the product is the bf16-source kernels' K' = 3K one (conv_a: 3C channels per tap)
    p.split = want_split && staged;
    if (p.split) { p.K = 3 * d.K; if (d.conv_a) p.conv_C = 3 * d.conv_C; }
    const int kch = (p.K + BK - 1) / BK;
    int splitk;
    if (staged) {
        const bool use256 = shape256 && (!d.conv_a || (long)d.M * p.conv_C * 2 < (1l << 31));
        p.kernel = !use256 ? GemmKernel::src128 : km ? GemmKernel::src256km : GemmKernel::src256;    // (km implies use256)
        const int lo_grp = !p.split ? 0 : d.conv_b ? d.K : 64;   // split k-major copies: K-tile interleave, or whole stacks next to conv_b
        const int lo = p.split ? 1 : 0;                           // lo slot of a split copy: 1 for A, 2 for B
        if (a_caller) p.a = {GemmSrc::caller, d.lda16};
        else if (d.conv_a) p.a = {GemmSrc::staged, p.conv_C, true, lda, d.M, d.conv_C, lo, 0, p.a.bytes};
        else if (km) p.a = {GemmSrc::staged, d.M, true, lda, d.K, d.M, lo, lo_grp, p.a.bytes};         // the k-major copies are [K][rows]
        else p.a = {GemmSrc::staged, p.K, akc, lda, d.M, d.K, lo, 0, p.a.bytes};
        if (b_caller) p.b = {GemmSrc::caller, d.ldb16};
        else if (d.conv_b) p.b = {GemmSrc::staged, d.conv_C, true, ldb, d.K, d.conv_C, 2 * lo, lo_grp, p.b.bytes};
        else if (km) p.b = {GemmSrc::staged, d.N, true, ldb, d.K, d.N, 2 * lo, lo_grp, p.b.bytes};
        else p.b = {GemmSrc::staged, p.K, bkc, ldb, d.N, d.K, 2 * lo, 0, p.b.bytes};
        splitk = use256 ? choose_splitk(d, true, (long)(d.M / 256) * (d.N / 256), kch, ws_bytes) : choose_splitk(d, false, (long)(d.M / 128) * (d.N / 128), kch, ws_bytes);
    } else {
        // 128x128 tiles whenever both extents allow it (4 MFMAs per 4 LDS fragment reads); a grid that
        // would not fill the chip is completed by split-K when scratch is available, else by 64x64 tiles.
        const bool can_split = d.ws && d.beta == 0.f && kch >= 64;
        const long tiles128 = (long)((d.M + 127) / 128) * ((d.N + 127) / 128) * d.batch;
        const bool small = !use_bf16 && ((d.M <= 64 || d.N <= 64) || (tiles128 < 256 && !can_split));
        p.kernel = use_bf16 ? GemmKernel::bf16conv : small ? GemmKernel::f32_64 : GemmKernel::f32_128;
        splitk = choose_splitk(d, false, small ? (long)((d.M + 63) / 64) * ((d.N + 63) / 64) * d.batch : tiles128, kch, ws_bytes);
    }
    const int round = p.kernel >= GemmKernel::bf16conv ? 3 : 0;                 // bf16 kernels: whole 64-wide chunks per split
    p.kchunks = ((kch + splitk - 1) / splitk + round) & ~round;
    p.splitk = (kch + p.kchunks - 1) / p.kchunks;                               // drop empty splits
    if (p.kernel >= GemmKernel::src256 && p.splitk > 1 && kch - (p.splitk - 1) * p.kchunks < 8) {   // the 256-tile kernel needs two K-tiles in every split
        p.kchunks = ((kch + p.splitk - 2) / (p.splitk - 1) + 3) & ~3;
        p.splitk = (kch + p.kchunks - 1) / p.kchunks;
    }
    return p;
}

int gemm_plan(const GemmDesc& d, GemmPlan* out) {
    T2_TRY_RC(check_gemm(d));
    *out = plan_gemm(d);
    T2_REQUIRE((long)d.batch * out->splitk <= 65535, "gemm: batch*splitk too large (%d*%d)", d.batch, out->splitk);
    return 0;
}

bool gemm_handoff(const GemmDesc& plain, const GemmDesc& offered, GemmPlan* plan) {
    const GemmPlan p0 = plan_gemm(plain);
    if (plan) *plan = p0;
    if (g_precision != 1 || !gemm_reads_bf16_copies(p0.kernel) || !(offered.A16 || offered.B16)) return false;
    if ((offered.A16 && p0.a.src != GemmSrc::staged) || (offered.B16 && p0.b.src != GemmSrc::staged)) return false;
    const GemmPlan p1 = plan_gemm(offered);
    if (p1.kernel != p0.kernel || p1.split != p0.split || p1.splitk != p0.splitk || p1.kchunks != p0.kchunks) return false;
    if ((offered.A16 && p1.a.src != GemmSrc::caller) || (offered.B16 && p1.b.src != GemmSrc::caller)) return false;
    if (plan) *plan = p1;
    return true;
}

int gemm(const GemmDesc& d, hipStream_t s) {
    GemmPlan p;
    T2_TRY_RC(gemm_plan(d, &p));
    static const int g_log = env_int("T2_GEMM_LOG", 0);      // dev: one line per product (shape, kernel, split, which operands get staged)
    if (g_log)
        fprintf(stderr, "t2gemm M=%d N=%d K=%d batch=%d %s%s kernel=%s splitk=%d stageA=%d stageB=%d convA=%d convB=%d beta=%g\n", d.M, d.N, d.K, d.batch,
                d.conv_a || d.sak == 1 ? "A[m][k]" : "A[k][m]", !d.conv_b && d.sbk == 1 ? " B[n][k]" : " B[k][n]", gemm_plan_name(p),
                p.splitk, p.a.src == GemmSrc::staged, p.b.src == GemmSrc::staged, d.conv_a, d.conv_b, (double)d.beta);
    ++g_counts[p.split ? 3 : gemm_reads_bf16_copies(p.kernel) ? 2 : p.kernel == GemmKernel::bf16conv ? 1 : 0];
    return run_gemm(d, p, s);
}

}  // namespace t2
