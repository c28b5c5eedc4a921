// C ABI (include/t2amd.h) of the GEMM layer, the conv / BatchNorm layers, the LSTM sequences, the chain plans and the small
// element-wise calls: thin wrappers over the launchers of kernels.h; and the process-wide host state (error string, profiler,
// side stream, status block, switches; driver.h) that the decoder drivers in decoder.hip share.  The other families keep
// their entry points at the end of their own files.
// No device allocation, no synchronisation except where the header says so.
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <sys/file.h>
#include <unistd.h>
#include <stdlib.h>
#include <string.h>

#include "kernels.h"
#include "chain_plan.h"
#include "driver.h"

static thread_local char g_err[512] = "";

void t2_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#include <algorithm>
#include <mutex>
#include <vector>

using namespace t2;

namespace t2 {
// ---------------------------------------------------------------------------------------------
// Optional in-situ kernel timing (bench.py's roofline figures): when enabled, the drivers bracket
// the per-step kernel launches with HIP events on the launch stream.  Off by default.
// ---------------------------------------------------------------------------------------------
struct Prof {
    bool on = false;
    std::vector<hipEvent_t> ev;
    std::vector<int> kind;
    size_t used = 0;
};
static Prof g_prof;

ProfScope::ProfScope(int kind, hipStream_t st) : s(st), on(g_prof.on && g_prof.used + 2 <= g_prof.ev.size()) {
    if (on) { g_prof.kind[g_prof.used / 2] = kind; (void)hipEventRecord(g_prof.ev[g_prof.used], s); }
}
ProfScope::~ProfScope() {
    if (on) { (void)hipEventRecord(g_prof.ev[g_prof.used + 1], s); g_prof.used += 2; }
}

// ---------------------------------------------------------------------------------------------
// Side stream for the decoder-LSTM recurrence.  Teacher-forced passes have two serial chains that only meet through
// hoisted GEMMs: (A) attention LSTMs + attention, (B) decoder LSTM.  Each per-step launch is bound by what ONE CU can
// pull from L2/MALL and leaves much of the chip idle (the attention step uses B*2 workgroups, the decoder-LSTM step
// H/8), so chain B runs on its own stream one chunk of steps behind (forward) / ahead of (backward) chain A.
// The caller's stream forks at the first chunk and joins before the entry point returns.
// ---------------------------------------------------------------------------------------------
static Side g_side[16];
int g_overlap = 1;
int g_chain = getenv("T2_CHAIN") ? atoi(getenv("T2_CHAIN")) : 1;   // persistent chain kernels (chain.hip)
int g_chain_bwd = getenv("T2_CHAIN_BWD") ? atoi(getenv("T2_CHAIN_BWD")) : 1;   // ... of the backward pass (chain_bwd.hip)
uint64_t g_step_counts[6] = {0, 0, 0, 0, 0, 0};
int counted(int rc, int base, int family) { if (rc == 0) ++g_step_counts[base + family]; return rc; }
uint64_t g_defer_counts[2] = {0, 0};
int g_dg_handoff = getenv("T2_DG_HANDOFF") ? atoi(getenv("T2_DG_HANDOFF")) != 0 : 1;   // backward chains leave dG as bf16 rows (chain_bwd.hip)
uint64_t g_dg_cast_counts[2] = {0, 0};
int g_split_steps = getenv("T2_SPLIT_STEPS") ? atoi(getenv("T2_SPLIT_STEPS")) != 0 : 0;   // split-bf16 recurrent steps (mode 2 only)
int side_get(Side** out) {
    int dev = 0;
    T2_CHECK_HIP(hipGetDevice(&dev));
    Side& sd = g_side[dev & 15];
    if (!sd.s) {
        // lowest priority: chain A (the caller's stream) is the critical path, the side chain has slack
        int least = 0, greatest = 0;
        T2_CHECK_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        T2_CHECK_HIP(hipStreamCreateWithPriority(&sd.s, hipStreamNonBlocking, least));
    }
    *out = &sd;
    return 0;
}
static int side_event(Side& sd, size_t i, hipEvent_t* out) {
    while (sd.ev.size() <= i) {
        hipEvent_t e;
        T2_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        sd.ev.push_back(e);
    }
    *out = sd.ev[i];
    return 0;
}
int stream_edge(Side& sd, size_t i, hipStream_t from, hipStream_t to) {
    hipEvent_t e;
    T2_TRY_RC(side_event(sd, i, &e));
    T2_CHECK_HIP(hipEventRecord(e, from));
    T2_CHECK_HIP(hipStreamWaitEvent(to, e, 0));
    return 0;
}

static StopPoll g_poll[16];
int stop_poll_get(StopPoll** out) {
    int dev = 0;
    T2_CHECK_HIP(hipGetDevice(&dev));
    StopPoll& p = g_poll[dev & 15];
    if (!p.host) {
        T2_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&p.host), 4 * sizeof(int32_t), hipHostMallocDefault));
        for (auto& e : p.ev) T2_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    *out = &p;
    return 0;
}
}  // namespace t2

// ---------------------------------------------------------------------------------------------
// Sticky status of the persistent kernels, one block per device in PAGE-LOCKED HOST memory that the device writes
// directly (chain_common.h report_abort) and reads in the optimizer (optim.hip): word 0 = code of the hand-off that
// timed out (0 = fine).  The host looks at it with a plain load — no copy, no event, no synchronisation — at every
// entry point of the Python layer and right after its own synchronisation points; nothing clears it but
// t2_chain_status_clear, so one aborted chain stops every later optimizer step until the caller has seen it.
// The same block carries this process's CLAIM on the device: a persistent grid needs every CU, so only one process per
// GPU may launch them (an flock on a per-device file; T2_CHAIN_FORCE=1 skips the test, e.g. for a child process whose
// parent holds the claim but is idle).
// ---------------------------------------------------------------------------------------------
struct StatusBlock { unsigned* host = nullptr; int claim = 0; };        // claim: 0 = not asked yet, 1 = held, -1 = another process holds it
static StatusBlock g_status[16];
static std::mutex g_status_mu;

namespace t2 {
unsigned* chain_sticky_words() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(g_status_mu);
    StatusBlock& b = g_status[dev & 15];
    if (!b.host) {
        void* p = nullptr;
        if (hipHostMalloc(&p, 64, hipHostMallocMapped) != hipSuccess) return nullptr;
        memset(p, 0, 64);
        b.host = static_cast<unsigned*>(p);
    }
    return b.host;
}
bool chain_device_claim() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lock(g_status_mu);
    StatusBlock& b = g_status[dev & 15];
    if (b.claim == 0) {
        b.claim = 1;
        const char* force = getenv("T2_CHAIN_FORCE");
        if (!(force && atoi(force) != 0)) {
            char bus[64] = "";
            if (hipDeviceGetPCIBusId(bus, sizeof(bus), dev) != hipSuccess) snprintf(bus, sizeof(bus), "dev%d", dev);
            for (char* c = bus; *c; ++c) if (*c == ':' || *c == '.' || *c == '/') *c = '_';
            char path[160];
            snprintf(path, sizeof(path), "/tmp/t2amd-persistent-%s.lock", bus);
            const int fd = open(path, O_CREAT | O_RDWR | O_CLOEXEC, 0666);
            if (fd >= 0 && flock(fd, LOCK_EX | LOCK_NB) != 0) {            // held by another process for as long as it lives
                close(fd);
                b.claim = -1;
                fprintf(stderr, "t2amd: another process runs persistent kernels on GPU %s: this process takes the per-step launch path "
                                "(one process per GPU is the contract; T2_CHAIN_FORCE=1 overrides)\n", bus);
            }                                                               // (fd stays open: the lock lives as long as the process)
        }
    }
    return b.claim > 0;
}
}  // namespace t2

__global__ void status_report_kernel(unsigned* sticky, unsigned code) {
    if (threadIdx.x == 0 && blockIdx.x == 0) __hip_atomic_store(sticky, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// tests: `workgroups` workgroups that each hold a CU's LDS (no persistent workgroup fits next to one) for `ticks` of the
// 100 MHz realtime counter — what a foreign kernel does to a persistent grid
__global__ __launch_bounds__(256) void occupy_kernel(unsigned long long ticks, unsigned* sink) {
    extern __shared__ unsigned hold[];
    hold[threadIdx.x] = threadIdx.x;
    // the highest vector and accumulation registers: each wave then owns a SIMD's whole register file (512 per lane), so
    // no wave of any other kernel — whatever its size — fits on a CU this workgroup sits on
    asm volatile("v_mov_b32 v255, 0\n\tv_accvgpr_write_b32 a255, 0" ::: "v255", "a255");
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
    if (hold[(threadIdx.x + 1) & 255] == 0xffffffffu) *sink = 1;            // (keeps the LDS allocation alive)
}

static size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

extern "C" {

const char* t2_last_error(void) { return g_err; }
int t2_version(void) { return T2_ABI_VERSION; }
int t2_chain_status(uint32_t* out_host) {
    T2_REQUIRE(out_host, "null argument");
    const unsigned* w = chain_sticky_words();
    T2_REQUIRE(w, "t2_chain_status: no status block");
    for (int i = 0; i < 4; ++i) out_host[i] = __atomic_load_n(w + i, __ATOMIC_RELAXED);
    return 0;
}
int t2_chain_status_clear(void) {
    unsigned* w = chain_sticky_words();
    T2_REQUIRE(w, "t2_chain_status_clear: no status block");
    for (int i = 0; i < 4; ++i) __atomic_store_n(w + i, 0u, __ATOMIC_RELAXED);
    return 0;
}
int t2_debug_report_abort(uint32_t code, void* stream) {
    unsigned* w = chain_sticky_words();
    T2_REQUIRE(w, "t2_debug_report_abort: no status block");
    hipLaunchKernelGGL(status_report_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, w, code);
    T2_LAUNCH_CHECK();
    return 0;
}
int t2_chain_claimed(void) { return chain_device_claim() ? 1 : 0; }
int t2_debug_occupy(int workgroups, int milliseconds, void* stream) {
    T2_REQUIRE(workgroups >= 1 && workgroups <= 256 && milliseconds >= 1 && milliseconds <= 5000, "t2_debug_occupy: 1..256 workgroups, 1..5000 ms");
    unsigned* w = chain_sticky_words();
    T2_REQUIRE(w, "t2_debug_occupy: no status block");
    const size_t smem = 96 * 1024;                                          // more than half a CU's LDS: one such workgroup per CU, no chain workgroup beside it
    T2_TRY_RC(t2_allow_dynamic_lds(reinterpret_cast<const void*>(occupy_kernel), smem));
    hipLaunchKernelGGL(occupy_kernel, dim3(workgroups), dim3(256), smem, (hipStream_t)stream, (unsigned long long)milliseconds * 100000ull, w + 8);
    T2_LAUNCH_CHECK();
    return 0;
}
int t2_set_precision(int mode) {
    T2_REQUIRE(mode >= 0 && mode <= 2, "t2_set_precision: mode must be 0 (fp32), 1 (bf16 operands) or 2 (split-bf16 large GEMMs), not %d", mode);
    set_precision(mode);
    return 0;
}
int t2_get_precision(void) { return get_precision(); }
int t2_set_gemm_split_min_mflop(int mflop) { set_gemm_split_min_mflop(mflop); return 0; }
int t2_gemm_counts(uint64_t* out_host, int reset) {
    T2_REQUIRE(out_host, "null argument");
    gemm_counts(out_host, reset);
    return 0;
}
int t2_set_split_steps(int on) { g_split_steps = on != 0; return 0; }
int t2_get_split_steps(void) { return g_split_steps; }
int t2_step_counts(uint64_t* out_host, int reset) {
    T2_REQUIRE(out_host, "null argument");
    for (int i = 0; i < 6; ++i) { out_host[i] = g_step_counts[i]; if (reset) g_step_counts[i] = 0; }
    return 0;
}
int t2_set_overlap(int on) { g_overlap = on != 0; return 0; }
int t2_set_chain(int on) { g_chain = on != 0; return 0; }
int t2_get_chain(void) { return g_chain; }
int t2_set_chain_bwd(int on) { g_chain_bwd = on != 0; return 0; }
int t2_set_gemm_staging(int on) { set_gemm_staging(on); return 0; }
int t2_set_gemm_fold(int on) { set_gemm_fold(on); return 0; }
int t2_set_bn_fuse(int on) { set_bn_fuse(on); return 0; }
int t2_get_bn_fuse(void) { return get_bn_fuse(); }
int t2_bn_fuse_counts(uint64_t* out_host, int reset) {
    T2_REQUIRE(out_host, "null argument");
    bn_fuse_counts(out_host, reset);
    return 0;
}
int t2_defer_counts(uint64_t* out_host, int reset) {
    T2_REQUIRE(out_host, "null argument");
    for (int i = 0; i < 2; ++i) { out_host[i] = g_defer_counts[i]; if (reset) g_defer_counts[i] = 0; }
    return 0;
}
int t2_set_dg_handoff(int on) { g_dg_handoff = on != 0; return 0; }
int t2_get_dg_handoff(void) { return g_dg_handoff; }
int t2_dg_handoff_counts(uint64_t* out_host, int reset) {
    T2_REQUIRE(out_host, "null argument");
    for (int i = 0; i < 2; ++i) { out_host[i] = g_dg_cast_counts[i]; if (reset) g_dg_cast_counts[i] = 0; }
    return 0;
}
int t2_stage_bf16(const float* src, long ld, void* dst, int rows, int K, void* stream) {
    T2_REQUIRE(src && dst, "null argument");
    return stage_bf16(src, true, ld, static_cast<__bf16*>(dst), rows, K, (hipStream_t)stream);
}
int t2_side_join(void* stream) {
    Side* side = nullptr;
    T2_TRY(side_get(&side));
    hipEvent_t e;
    T2_TRY(side_event(*side, 0, &e));          // slot 0 is free between calls: every call re-records its events before use
    T2_CHECK_HIP(hipEventRecord(e, side->s));
    T2_CHECK_HIP(hipStreamWaitEvent((hipStream_t)stream, e, 0));
    return 0;
}

int t2_conv_bn_forward(const t2_conv_bn_args* a, void* stream) {
    T2_REQUIRE(a, "null argument");
    const size_t nw = (size_t)a->Cout * a->Cin * a->K;
    T2_REQUIRE(a->ws_floats >= nw + 128 * (size_t)a->Cout, "t2_conv_bn_forward: workspace too small");
    ConvBnFwd f{};
    f.x = a->x; f.B = a->B; f.T = a->T; f.Cin = a->Cin; f.Cout = a->Cout; f.K = a->K;
    f.w = a->w; f.bias = a->bias; f.gamma = a->gamma; f.beta = a->beta; f.run_mean = a->run_mean; f.run_var = a->run_var;
    f.training = a->training; f.eps = a->eps; f.act = a->act; f.drop_p = a->drop_p; f.seed = a->seed; f.site = a->site;
    f.residual = a->residual; f.z = a->z; f.mean = a->mean; f.invstd = a->invstd; f.var = a->var; f.y = a->y;
    f.wperm = a->ws; f.scratch = a->ws + align4(nw);
    const size_t used = align4(nw) + 128 * (size_t)a->Cout;
    if (a->ws_floats > used) { f.gemm_ws = a->ws + used; f.gemm_ws_bytes = (a->ws_floats - used) * sizeof(float); }
    f.handoff = a->handoff; f.x16 = static_cast<const __bf16*>(a->x16); f.y16 = static_cast<__bf16*>(a->y16);
    return conv_bn_fwd(f, (hipStream_t)stream);
}

int t2_conv_bn_backward(const t2_conv_bn_bwd_args* a, void* stream) {
    T2_REQUIRE(a, "null argument");
    const size_t nw = align4((size_t)a->Cout * a->Cin * a->K), ndz = align4((size_t)a->B * a->T * a->Cout), nsc = 128 * (size_t)a->Cout;
    T2_REQUIRE(a->ws_floats >= nw + ndz + nsc, "t2_conv_bn_backward: workspace too small");
    ConvBnBwd f{};
    f.x = a->x; f.B = a->B; f.T = a->T; f.Cin = a->Cin; f.Cout = a->Cout; f.K = a->K;
    f.w = a->w; f.gamma = a->gamma; f.beta = a->beta; f.z = a->z; f.mean = a->mean; f.invstd = a->invstd;
    f.training = a->training; f.eps = a->eps; f.act = a->act; f.drop_p = a->drop_p; f.seed = a->seed; f.site = a->site;
    f.dy = a->dy; f.dw = a->dw; f.dbias = a->dbias; f.dgamma = a->dgamma; f.dbeta = a->dbeta;
    f.dx = a->dx; f.dx_accumulate = a->dx_accumulate;
    f.dz = a->ws; f.wperm = a->ws + ndz; f.scratch = a->ws + ndz + nw;
    f.gemm_ws = a->ws + ndz + nw + nsc; f.gemm_ws_bytes = (a->ws_floats - (ndz + nw + nsc)) * sizeof(float);
    f.handoff = a->handoff; f.x16 = static_cast<const __bf16*>(a->x16);
    return conv_bn_bwd(f, (hipStream_t)stream);
}

int t2_embedding_forward(const int64_t* ids, const float* table, float* out, int rows, int dim, void* stream) {
    return embedding_fwd(reinterpret_cast<const long*>(ids), table, out, rows, dim, (hipStream_t)stream);
}
int t2_embedding_backward(const int64_t* ids, const float* dout, float* dtable, int rows, int dim, int vocab, void* stream) {
    return embedding_bwd(reinterpret_cast<const long*>(ids), dout, dtable, rows, dim, vocab, (hipStream_t)stream);
}

int t2_lstm_seq_forward(const t2_lstm_seq_args* a, void* stream) {
    T2_REQUIRE(a && a->nstreams >= 1 && a->nstreams <= kMaxLstmStreams, "t2_lstm_seq_forward: bad nstreams");
    T2_REQUIRE(a->H % 64 == 0, "t2_lstm_seq_forward: H=%d must be a multiple of 64", a->H);
    const int B = a->B, T = a->T, H = a->H;
    // every step of both directions in one persistent launch (chain_enc.hip) when the shape is covered and the caller
    // gave exchange space; otherwise one launch per step
    ChainPlan plan{CHAIN_REFUSE_WORKSPACE};
    if (g_chain && a->ws && a->ws_floats) plan = plan_here(plan_enc_chain, enc_chain_shape(a->nstreams, B, H, 0, a->ws_floats * sizeof(float)));
    if (plan.refusal == CHAIN_OK) {
        EncChainDesc d{};
        d.ND = a->nstreams; d.B = B; d.T = T; d.H = H; d.lengths = a->lengths; d.ldh = a->ldh;
        for (int s = 0; s < a->nstreams; ++s) {
            d.pre[s] = a->pre[s]; d.w_hh[s] = a->w_hh[s]; d.reverse[s] = a->reverse[s];
            d.h[s] = a->h[s]; d.c[s] = a->c[s]; d.gates[s] = a->gates[s];
        }
        return enc_chain_fwd(d, plan, a->ws, a->ws_floats, (hipStream_t)stream);
    }
    for (int step = 0; step < T; ++step) {
        LstmStepDesc d{};
        d.nstreams = a->nstreams; d.B = B; d.H = H; d.drop_p = 0.f;
        for (int s = 0; s < a->nstreams; ++s) {
            LstmStream& st = d.st[s];
            const int t = a->reverse[s] ? T - 1 - step : step;
            const int tp = a->reverse[s] ? t + 1 : t - 1;            // time index processed in the previous step
            st.pre = a->pre[s] + (long)t * B * 4 * H; st.ldpre = 4 * H;
            if (step > 0) {
                st.seg[0] = LstmSeg{a->h[s] + (long)tp * B * a->ldh, a->ldh, a->w_hh[s], (long)H, H};
                st.nseg = 1;
                st.c_prev = a->c[s] + (long)tp * B * H; st.ldc_prev = H;
            }
            st.gates = a->gates[s] + (long)t * B * 4 * H; st.ldgates = 4 * H;
            st.c_out = a->c[s] + (long)t * B * H; st.ldc_out = H;
            st.h_out = a->h[s] + (long)t * B * a->ldh; st.ldh_out = a->ldh;
            st.lengths = a->lengths; st.t = t;
        }
        T2_TRY(lstm_step_fwd(d, (hipStream_t)stream));
    }
    return 0;
}

size_t t2_lstm_seq_chain_ws_floats(int nstreams, int B, int H, int backward) { return enc_chain_ws_floats(nstreams, B, H, backward); }

int t2_lstm_seq_backward(const t2_lstm_seq_bwd_args* a, void* stream) {
    T2_REQUIRE(a && a->nstreams >= 1 && a->nstreams <= kMaxLstmStreams, "t2_lstm_seq_backward: bad nstreams");
    const int B = a->B, T = a->T, H = a->H, ns = a->nstreams;
    const int ks = lstm_bwd_ksplit(4 * H);
    hipStream_t s = (hipStream_t)stream;
    float* dc = a->ws;                                        // [ns][B*H]
    float* part = dc + align4((size_t)ns * B * H);            // [ns][ks][B][H]
    float* gws = part + align4((size_t)ns * ks * B * H);
    T2_REQUIRE(a->ws_floats >= (size_t)(gws - a->ws), "t2_lstm_seq_backward: workspace too small");
    const size_t gws_bytes = (a->ws_floats - (size_t)(gws - a->ws)) * sizeof(float);
    ChainPlan plan{CHAIN_REFUSE_WORKSPACE};
    if (g_chain && g_chain_bwd && a->ws_floats) plan = plan_here(plan_enc_chain, enc_chain_shape(ns, B, H, 1, a->ws_floats * sizeof(float)));
    const bool chain = plan.refusal == CHAIN_OK;
    if (chain) {                                               // whole BPTT in one persistent launch (chain_enc.hip); its exchange space = this scratch
        EncChainBwdDesc d{};
        d.ND = ns; d.B = B; d.T = T; d.H = H; d.lddh = a->lddh;
        for (int i = 0; i < ns; ++i) {
            d.w_hh[i] = a->w_hh[i]; d.reverse[i] = a->reverse[i]; d.c[i] = a->c[i]; d.gates[i] = a->gates[i];
            d.dh[i] = a->dh[i]; d.dpre[i] = a->dpre[i];
        }
        T2_TRY(enc_chain_bwd(d, plan, a->ws, a->ws_floats, s));
    }
    for (int step = 0; step < (chain ? 0 : T); ++step) {      // reverse of the processing order
        LstmBwdPointDesc p{};
        p.nstreams = ns; p.B = B; p.H = H; p.drop_p = 0.f; p.first = step == 0;
        LstmBwdGemmDesc g{};
        g.nstreams = ns; g.B = B; g.H4 = 4 * H; g.KS = ks; g.NC = H;
        for (int i = 0; i < ns; ++i) {
            // processing order: forward dir t = 0..T-1, reverse dir t = T-1..0; BPTT visits it backwards
            const int t = a->reverse[i] ? step : T - 1 - step;
            const int tprev = a->reverse[i] ? t + 1 : t - 1;  // the step whose state entered step t
            const bool has_prev = a->reverse[i] ? (t + 1 < T) : (t > 0);
            LstmBwdStream& st = p.st[i];
            st.dh1 = a->dh[i] + (long)t * B * a->lddh; st.lddh1 = a->lddh;
            st.part = part + (size_t)i * ks * B * H; st.nparts = ks; st.part_stride = (long)B * H; st.ldpart = H; st.part_col = 0;
            st.gates = a->gates[i] + (long)t * B * 4 * H; st.ldgates = 4 * H;
            st.c_new = a->c[i] + (long)t * B * H; st.ldc_new = H;
            if (has_prev) { st.c_prev = a->c[i] + (long)tprev * B * H; st.ldc_prev = H; }
            st.dc_state = dc + (size_t)i * B * H;
            st.dg = a->dpre[i] + (long)t * B * 4 * H; st.lddg = 4 * H;
            g.st[i].dg = st.dg; g.st[i].lddg = 4 * H;
            g.st[i].seg[0] = LstmBwdSeg{a->w_hh[i], (long)H, H}; g.st[i].nseg = 1;
            g.st[i].part = part + (size_t)i * ks * B * H;
        }
        T2_TRY(lstm_bwd_pointwise(p, s));
        if (step + 1 < T) T2_TRY(lstm_bwd_gemm(g, s));
    }
    // d(W_hh) = sum_t dpre(t)^T . h(previous processed step)
    for (int i = 0; i < ns; ++i) {
        if (T < 2) { T2_TRY(fill_f32(a->dw_hh[i], 0.f, (size_t)4 * H * H, s)); continue; }
        GemmDesc w = gemm_desc();
        const long rowsB = (long)B;
        w.A = a->reverse[i] ? a->dpre[i] : a->dpre[i] + rowsB * 4 * H; w.sam = 1; w.sak = 4 * H;
        w.B = a->reverse[i] ? a->h[i] + rowsB * a->ldh : a->h[i]; w.sbk = a->ldh; w.sbn = 1;
        w.C = a->dw_hh[i]; w.ldc = H; w.M = 4 * H; w.N = H; w.K = (T - 1) * B;
        w.ws = gws; w.ws_bytes = gws_bytes;
        T2_TRY(gemm(w, s));
    }
    return 0;
}

static GemmDesc desc_of(const t2_gemm_args& a) {
    GemmDesc g = gemm_desc();
    g.A = a.A; g.B = a.B; g.C = a.C; g.M = a.M; g.N = a.N; g.K = a.K;
    g.sam = a.sam; g.sak = a.sak; g.sbn = a.sbn; g.sbk = a.sbk; g.ldc = a.ldc;
    g.batch = a.batch > 0 ? a.batch : 1; g.bsA = a.bsA; g.bsB = a.bsB; g.bsC = a.bsC;
    g.alpha = a.alpha; g.beta = a.beta; g.bias1 = a.bias; g.act = a.act;
    g.crow_mod = a.crow_mod; g.crow_mul = a.crow_mul;
    g.ws = a.ws; g.ws_bytes = a.ws_bytes; g.splitk = a.splitk;
    return g;
}
int t2_gemm_ex(const t2_gemm_args* a, void* stream) {
    T2_REQUIRE(a, "null argument");
    return gemm(desc_of(*a), (hipStream_t)stream);
}
static GemmDesc desc_of(const t2_gemm_args& a, const t2_gemm_plan_opts* o) {
    GemmDesc g = desc_of(a);
    if (o) {
        g.conv_a = o->conv_a; g.conv_b = o->conv_b; g.conv_T = o->conv_T; g.conv_C = o->conv_C; g.fp32_only = o->fp32_only;
        const __bf16* copy = reinterpret_cast<const __bf16*>(uintptr_t(256));          // only its alignment is looked at
        if (o->a16) { g.A16 = copy; g.lda16 = o->lda16; g.a16_kmajor = o->a16_kmajor; }
        if (o->b16) { g.B16 = copy; g.ldb16 = o->ldb16; g.b16_kmajor = o->b16_kmajor; }
        g.split16 = o->split16;
    }
    return g;
}
static t2_gemm_plan_info info_of(const GemmPlan& p) {
    return t2_gemm_plan_info{(int)p.kernel, gemm_plan_name(p), p.split, p.splitk, p.kchunks, (int)p.a.src, (int)p.b.src, p.a.bytes, p.b.bytes};
}
int t2_gemm_plan(const t2_gemm_args* a, const t2_gemm_plan_opts* o, t2_gemm_plan_info* out) {
    T2_REQUIRE(a && out, "null argument");
    GemmPlan p;
    T2_TRY(gemm_plan(desc_of(*a, o), &p));
    *out = info_of(p);
    return 0;
}
int t2_chain_plan(const t2_chain_shape* z, int direction, int cus, int claimed, int no_resident, t2_chain_plan_info* out) {
    T2_REQUIRE(z && out && (direction == T2_CHAIN_FORWARD || direction == T2_CHAIN_BACKWARD), "t2_chain_plan: null argument or bad direction");
    ChainShape c{};
    c.kind = z->kind; c.dec = z->dec; c.NS = z->NS; c.B = z->B; c.H = z->H; c.E = z->E; c.A = z->A; c.P = z->P; c.M = z->M; c.Hd = z->Hd; c.F = z->F; c.Kc = z->Kc;
    c.Tin[0] = z->Tin[0]; c.Tin[1] = z->Tin[1]; c.backward = direction; c.saved_tiles = z->saved_tiles != 0; c.ws_bytes = z->ws_floats * sizeof(float);
    const ChainEnv env{cus, claimed != 0, no_resident != 0};
    const ChainPlan p = z->kind == T2_CHAIN_ENC ? plan_enc_chain(c, env) : direction == T2_CHAIN_BACKWARD ? plan_chain_bwd(c, env) : plan_chain_fwd(c, env);
    t2_chain_plan_info o{};
    o.covered = p.refusal == CHAIN_OK; o.reason = p.refusal; o.reason_text = chain_refusal_text(p.refusal);
    if (o.covered) {
        // (a space too small for the plan is the executors' error, not a refusal: the layouts size it; encoder chains refuse it)
        T2_REQUIRE(p.ws_bytes >= p.total, "t2_chain_plan: exchange space too small (%zu bytes, the chain needs %zu)", p.ws_bytes, p.total);
        o.instance = p.instance; o.instance_name = chain_instance_name(p.instance); o.grid = p.grid; o.lds_bytes = p.lds_bytes;
        o.UT = p.UT; o.RT = p.RT; o.CS = p.CS; o.MT = p.MT; o.lds_Tc = p.lds_Tc; o.lds_Tin = p.lds_Tin; o.lds_Jp = p.lds_Jp; o.lds_Jm = p.lds_Jm;
        for (int s = 0; s < 2; ++s) { o.Jp[s] = p.Jp[s]; o.Jm[s] = p.Jm[s]; }
        o.q_bytes = p.q_bytes; o.total_bytes = p.total; o.ws_bytes = p.ws_bytes;
        static_assert(CHAIN_PARTS == T2_CHAIN_PARTS, "t2_chain_plan_info carries every part");
        for (int i = 0; i < CHAIN_PARTS; ++i) { o.part_off[i] = p.part[i].off; o.part_bytes[i] = p.part[i].bytes; o.part_name[i] = chain_part_name(i); }
        o.clear_off = p.clear.off; o.clear_bytes = p.clear.bytes;
        for (int w = 0; w < 3 && z->kind != T2_CHAIN_ENC && direction == T2_CHAIN_FORWARD; ++w) o.pass_clear_bytes[w] = chain_fwd_clear_range(p.ws_bytes, (ChainWsClear)w).bytes;
    }
    *out = o;
    return 0;
}
int t2_conv_handoff_plan(const t2_gemm_args* a, const t2_gemm_plan_opts* o, int* taken, t2_gemm_plan_info* out) {
    T2_REQUIRE(a && taken && out, "null argument");
    const GemmDesc offered = desc_of(*a, o);
    GemmDesc plain = offered;
    plain.A16 = plain.B16 = nullptr; plain.a16_kmajor = plain.b16_kmajor = 0; plain.lda16 = plain.ldb16 = 0;
    GemmPlan p;
    T2_TRY(gemm_plan(plain, &p));                       // the checks of gemm(), and its refusals
    *taken = gemm_handoff(plain, offered, &p);
    *out = info_of(p);
    return 0;
}
// bench.py's GEMM roofline figure: `reps` launches of one product bracketed by HIP events on the launch stream, once as
// t2_gemm_ex runs it (fp32 operands in, staging casts included) and once with both bf16 operand copies made beforehand,
// so that the second figure is the matrix kernel (+ its split-K reduce) alone.
static int time_gemm(const GemmDesc& g, int reps, float* ms, hipStream_t s) {
    hipEvent_t e0, e1;
    T2_CHECK_HIP(hipEventCreate(&e0)); T2_CHECK_HIP(hipEventCreate(&e1));
    int rc = gemm(g, s);                                                  // warm-up
    T2_CHECK_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < reps && rc == 0; ++i) rc = gemm(g, s);
    T2_CHECK_HIP(hipEventRecord(e1, s));
    T2_CHECK_HIP(hipEventSynchronize(e1));
    T2_CHECK_HIP(hipEventElapsedTime(ms, e0, e1));
    *ms /= reps;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return rc;
}
int t2_prof_gemm(const t2_gemm_args* a, int reps, float* ms_total, float* ms_kernel, void* stream) {
    T2_REQUIRE(a && reps > 0 && ms_total && ms_kernel, "t2_prof_gemm: bad arguments");
    T2_REQUIRE(get_precision() != 0 && a->M % 128 == 0 && a->N % 128 == 0 && a->K % 64 == 0 && (a->batch <= 1) && a->ws,
               "t2_prof_gemm: bf16 or split-bf16 mode, whole-tile shapes and scratch only");
    hipStream_t s = (hipStream_t)stream;
    GemmDesc g = desc_of(*a);
    GemmPlan p, q;
    T2_TRY(gemm_plan(g, &p));
    T2_REQUIRE(p.a.src == GemmSrc::staged && p.b.src == GemmSrc::staged, "t2_prof_gemm: refused, gemm() runs this product on kernel %s, which stages no bf16 copies", gemm_plan_name(p));
    T2_TRY(time_gemm(g, reps, ms_total, s));
    // the copies as the plan lays them out, made once in front of the scratch and handed over
    unsigned char* w8 = reinterpret_cast<unsigned char*>(a->ws);
    __bf16* a16 = reinterpret_cast<__bf16*>(w8); __bf16* b16 = reinterpret_cast<__bf16*>(w8 + p.a.bytes);
    T2_TRY(stage_planned(g.A, p.a, p.split, a16, s));
    T2_TRY(stage_planned(g.B, p.b, p.split, b16, s));
    g.A16 = a16; g.lda16 = p.a.ld; g.B16 = b16; g.ldb16 = p.b.ld;
    g.a16_kmajor = g.b16_kmajor = p.kernel == GemmKernel::src256km; g.split16 = p.split;
    g.ws = reinterpret_cast<float*>(w8 + p.a.bytes + p.b.bytes); g.ws_bytes = a->ws_bytes - p.a.bytes - p.b.bytes;
    T2_TRY(gemm_plan(g, &q));
    T2_REQUIRE(q.kernel == p.kernel && q.split == p.split && q.a.src == GemmSrc::caller && q.b.src == GemmSrc::caller,
               "t2_prof_gemm: refused, with both copies handed over gemm() would run kernel %s and not read both", gemm_plan_name(q));
    return time_gemm(g, reps, ms_kernel, s);
}
int t2_colsum(const float* x, long ld, int M, int N, float* out, float* scratch, void* stream) {
    return colsum(x, ld, M, N, out, nullptr, scratch, (hipStream_t)stream);
}
int t2_mask_btc(float* x, int B, int T, int C, const int32_t* lengths, float fill, void* stream) {
    T2_REQUIRE(lengths, "t2_mask_btc: lengths is null");
    return mask_btc(x, B, T, C, lengths, fill, (hipStream_t)stream);
}

int t2_prof_enable(int max_launches) {
    if (max_launches <= 0) { g_prof.on = false; return 0; }
    const size_t need = (size_t)max_launches * 2;
    while (g_prof.ev.size() < need) {
        hipEvent_t e;
        T2_CHECK_HIP(hipEventCreate(&e));
        g_prof.ev.push_back(e);
    }
    g_prof.kind.assign(g_prof.ev.size() / 2, 0);
    g_prof.used = 0;
    g_prof.on = true;
    return 0;
}

int t2_prof_collect(int n_kinds, double* total_ms_host, int* launches_host) {
    T2_REQUIRE(n_kinds >= PK_COUNT, "t2_prof_collect: need %d kinds", (int)PK_COUNT);
    g_prof.on = false;
    for (int i = 0; i < n_kinds; ++i) { total_ms_host[i] = 0.0; launches_host[i] = 0; }
    if (g_prof.used == 0) return 0;
    T2_CHECK_HIP(hipDeviceSynchronize());                // events live on two streams
    for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
        float ms = 0.f;
        T2_CHECK_HIP(hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]));
        total_ms_host[g_prof.kind[i / 2]] += ms;
        launches_host[g_prof.kind[i / 2]] += 1;
    }
    g_prof.used = 0;
    return 0;
}

int t2_finalize_bct(const float* in_btc, float* out_bct, int B, int T, int C, const int32_t* lengths, float fill, void* stream) {
    return transpose_btc_to_bct(in_btc, out_bct, B, T, C, lengths, fill, (hipStream_t)stream);
}
int t2_mask_bt(float* x, int B, int T, const int32_t* lengths, float fill, void* stream) {
    T2_REQUIRE(lengths, "t2_mask_bt: lengths is null");
    return mask_bt(x, B, T, lengths, fill, (hipStream_t)stream);
}

int t2_gemm(const float* A, const float* B, float* C, int M, int N, int K, long sam, long sak, long sbn, long sbk, long ldc,
            const float* bias, int act, float alpha, float beta, float* ws, size_t ws_bytes, int splitk, void* stream) {
    GemmDesc g = gemm_desc();
    g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K;
    g.sam = sam; g.sak = sak; g.sbn = sbn; g.sbk = sbk; g.ldc = ldc;
    g.bias1 = bias; g.act = act; g.alpha = alpha; g.beta = beta;
    g.ws = ws; g.ws_bytes = ws_bytes; g.splitk = splitk;
    return gemm(g, (hipStream_t)stream);
}
int t2_rng_keep_mask(uint64_t seed, uint32_t site, uint32_t n, float p, uint8_t* out, void* stream) {
    return rng_keep_mask(seed, site, n, p, out, (hipStream_t)stream);
}
int t2_rng_normal(uint64_t seed, uint32_t site, uint32_t n, float* out, void* stream) {
    return rng_normal(seed, site, n, out, (hipStream_t)stream);
}

}  // extern "C"
