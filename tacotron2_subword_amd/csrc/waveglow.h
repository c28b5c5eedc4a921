// What the three WaveGlow files share: waveglow_kernels.hip (the kernels, one host launcher per launch), waveglow_plan.hip (pure
// host: the tensor table, the layouts and carves, the weight-gradient descriptor, the three plans) and waveglow.hip (the pack
// drivers, the three flow drivers and the C ABI).
#pragma once
#include <vector>

#include "../../include/t2amd.h"
#include "kernels.h"

namespace t2 {

constexpr int kWgMaxD = 128;                      // dilation of layer 7
static_assert(T2_WAVEGLOW_MAX_LAYERS == 8 && (1 << (T2_WAVEGLOW_MAX_LAYERS - 1)) == kWgMaxD, "the deepest layer's dilation fits the slab");
enum { kWgGated = 0, kWgResSkip = 1, kWgUpsample = 2, kWgGateBwd = 3, kWgAccum = 4 };   // the last two: epilogues of the backward
constexpr int kWgUpK = 1024, kWgUpStride = 256, kWgUpTaps = kWgUpK / kWgUpStride;
constexpr int kWgGradTile = 128, kWgGradTL = 32, kWgGradMaxSeg = 5, kWgGradMaxSplit = 64;

// ---- arguments of the kernels the drivers fill in themselves (waveglow_kernels.hip says what each field is)
struct WgCouple {
    const float* out; const float* w_end; const float* b_end; const float* in; const float* winv; const float* z;
    float* dst; float* inter;
    int nc, n_half, n_early; long L; float in_scale, sigma;
};
struct WgTail {
    const float* out; const float* w_end; const float* b_end; const float* in; const float* wnext;
    float* dst; float* z; float* log_s; double* part_s; double* part_z;
    int nc, n_half, n_peel, G, zoff; long L;
};
struct WgTailBwd {
    const float* out; const float* w_end; const float* b_end; const float* in;        // kept by the forward: out, audio_in of this flow
    const float* wnext; const float* dnext;        // W_{k+1} [Cn][Cn] and d(audio_in_{k+1}) [B, Cn, L]; unused on the last flow
    const float* dz; const float* dlog_s;          // nullable: upstream gradients on z [B, G, L] and on log_s[k] [B, n_half, L]
    float* d_out; float* d_in;                     // [B, nc, L]; [B, C, L]: d(audio_in) but for W_start^T dx, which wg_start_bwd adds
    double* part;                                  // [B * blocks * 4 waves][C*nc + C + Cn*Cn]: dW_end, db_end, dW_{k+1}
    int nc, n_half, n_peel, G, zoff; long L;
};
struct WgGradSeg { const float* src; int C, Cbuf, shift, tile0, col0, vec; }; // src null: ones; Cbuf: channels per item of the buffer; vec: 16-byte loads
struct WgGradDst { float* dst; float* dst2; long rs, cs; };                 // element (m, ch) of a segment goes to dst[m*rs + ch*cs]
struct WgGrad {
    const float* a; float* part;
    WgGradSeg seg[kWgGradMaxSeg]; WgGradDst dst[kWgGradMaxSeg];
    int nseg, M, Mbuf, B, mtiles, ntiles, Ntot, nchunk, per, nsplit, avec; long L;
};

// ---- waveglow_plan.hip
int wg_check_common(const char* who, int B, long L);
int wg_check_nc(const char* who, int nc);
int wg_check_group(const char* who, int G);
int wg_check_half(const char* who, int n_half);
int wg_check_peel(const char* who, int n_peel, int C, int zoff, int G);
int wg_gated_check(int B, int nc, int n_cond, long L, int d);
size_t wg_packed_floats(int kind, int rows, int k0, int k1);
size_t wg_packed_t_floats(int rows, int k0, int taps, int k1);

// The folded tensors in t2_waveglow_pack's order, by name: the upsample's two, then per flow start, cond, in_layers[i],
// res_skip_layers[i], end and the 1x1 mix.  Every index into a tensor list or into the gradient offsets comes from here.
struct WgTensors {
    int nl, nf;
    int per_flow() const { return 7 + 4 * nl; }
    int count() const { return 2 + nf * per_flow(); }
    int up_w() const { return 0; }
    int up_b() const { return 1; }
    int start_w(int k) const { return 2 + k * per_flow(); }
    int start_b(int k) const { return start_w(k) + 1; }
    int cond_w(int k) const { return start_w(k) + 2; }
    int cond_b(int k) const { return start_w(k) + 3; }
    int in_w(int k, int i) const { return start_w(k) + 4 + 2 * i; }
    int in_b(int k, int i) const { return in_w(k, i) + 1; }
    int rs_w(int k, int i) const { return in_w(k, nl) + 2 * i; }
    int rs_b(int k, int i) const { return rs_w(k, i) + 1; }
    int end_w(int k) const { return rs_w(k, nl); }
    int end_b(int k) const { return end_w(k) + 1; }
    int mix(int k) const { return end_w(k) + 2; }
};

// the packed weights of both flow drivers, offsets in floats
struct WgFlow {
    int c, n_half, early;                          // channels of `audio` in this flow; early: sigma * z is prepended after it
    size_t start_w, start_b, cond_b, end_w, end_b, winv;
    size_t gated[T2_WAVEGLOW_MAX_LAYERS], in_b[T2_WAVEGLOW_MAX_LAYERS], rs[T2_WAVEGLOW_MAX_LAYERS], rs_b[T2_WAVEGLOW_MAX_LAYERS];
};
struct WgLayout { WgTensors tt; std::vector<WgFlow> flows; size_t up_w, up_b, total; int n_remaining, n_planes; };
int wg_layout(const t2_waveglow_config& c, WgLayout* out);                     // judges the configuration
size_t wg_tensor_floats(const t2_waveglow_config& c, const WgLayout& lay, int tensor);      // torch-layout element count of tensor tt.<name>

// the transposed packs of the backward, and where every tensor's gradient starts inside the arena (pack order)
struct WgBwdFlow { size_t conv_t[T2_WAVEGLOW_MAX_LAYERS], cond_t[T2_WAVEGLOW_MAX_LAYERS], rs_t[T2_WAVEGLOW_MAX_LAYERS]; };
struct WgBwdLayout { std::vector<WgBwdFlow> flows; size_t total; std::vector<size_t> grad; size_t grad_total; };
void wg_bwd_layout(const t2_waveglow_config& c, const WgLayout& lay, WgBwdLayout* out);

// What the training forward keeps for the backward, in floats from the start of `saved` (per = B * L rounded up to 4):
// spect [B, n_mel*G, L] once; per flow the mixed audio_in [B, c_k, L] and out [B, nc, L]; per flow and layer x_i, tanh(u_a),
// sigmoid(u_b), [B, nc, L] each.  The pre-mix audio of flow k > 0 is cat(a0, a1')[n_peel:] of flow k - 1, which the tail backward
// recomputes anyway; flow 0's is the regrouped audio itself.
struct WgSaved {
    size_t per, nc, nl, n_cond;
    std::vector<size_t> base, ch;
    size_t total;
    size_t ain(int k) const { return base[k]; }
    size_t out(int k) const { return base[k] + per * ch[k]; }
    size_t x(int k, int i) const { return out(k) + per * nc * (1 + 3 * (size_t)i); }
    size_t t(int k, int i) const { return x(k, i) + per * nc; }
    size_t g(int k, int i) const { return x(k, i) + 2 * per * nc; }
};
WgSaved wg_saved(const t2_waveglow_config& c, const WgLayout& lay, int B, long L);

// The workspaces, offsets in floats (a double takes two; every region starts on 16 bytes) and the total behind the last one.
// infer and forward share the front; the fp64 regions are empty for infer.
struct WgFlowWs { size_t spect, x, out, acts, bufs[2], part_s, part_z, item, sums, total; };
struct WgBwdWs { size_t dx, d_out, du, acts, d_spect, dbuf[2], gpart, tpart, total; };

// the plans: what the C ABI reports (info) and what the driver places its buffers by
struct WgInferPlan { t2_waveglow_plan_info info; WgFlowWs ws; };
struct WgForwardPlan { t2_waveglow_forward_info info; WgLayout lay; WgFlowWs ws; };
struct WgBackwardPlan { t2_waveglow_backward_info info; WgLayout lay; WgBwdLayout bl; WgSaved sv; WgBwdWs ws; };
int wg_plan(const t2_waveglow_config& c, const WgLayout& lay, int B, int T, WgInferPlan* out);
int wg_forward_plan(const t2_waveglow_config& c, int B, int T, long N, WgForwardPlan* out);
int wg_backward_plan(const t2_waveglow_config& c, int B, int T, long N, WgBackwardPlan* out);

// One weight-gradient launch: rows M of `a` against the columns `taps` shifts of x (x_ch channels each, d apart), n_cond channels
// of spect (0: none) and a row of ones (the bias gradient).  The three the backward runs: conv + cond of a layer, a half of
// res_skip, start.
struct WgGradSite { int M, x_ch, taps, n_cond; };
inline WgGradSite wg_site_conv(int nc, int n_cond) { return {2 * nc, nc, 3, n_cond}; }
inline WgGradSite wg_site_res_skip(int nc) { return {nc, nc, 1, 0}; }
inline WgGradSite wg_site_start(int nc, int n_half) { return {nc, n_half, 1, 0}; }
struct WgGradOut { float* dw_x; float* dw_spect; float* db; float* db2; };      // [M][x_ch][taps], [M][n_cond], [M] and, nullable, [M] once more
size_t wg_grad_part_floats(const WgGradSite& g, int B, long L);                 // the partial planes of one launch
WgGrad wg_grad_desc(const WgGradSite& g, const float* a, int a_rows, const float* x, int x_rows, int d, const float* spect, const WgGradOut& out, int B,
                    long L, float* part);

// ---- waveglow_kernels.hip: one launch each
int wg_pack(int kind, const float* w0, const float* w1, float* out, int rows, int k0, int k1, hipStream_t s);
int wg_pack_conv_t(const float* w_in, float* out, int nc, hipStream_t s);
int wg_pack_cond_t(const float* w_cond_i, float* out, int nc, int n_cond, hipStream_t s);
int wg_pack_rs_t(const float* w_rs, float* out, int nc, int last, hipStream_t s);
int wg_gated(int B, int nc, int n_cond, long L, int d, int raw, const float* x, const float* spect, const float* packed, const float* b_in,
             const float* b_cond, float* y, hipStream_t s, float* keep_t = nullptr, float* keep_g = nullptr);
int wg_res_skip(int B, int nc, long L, int first, int last, const float* acts, const float* packed, const float* bias, float* x, float* out, hipStream_t s,
                const float* x_from = nullptr);
int wg_upsample(int B, int n_mel, int T, int G, long n_samples, const float* mel, const float* packed, const float* bias, float* spect, hipStream_t s);
int wg_start(int B, int nc, int ctot, int n_half, long L, float scale, const float* audio, const float* w, const float* bias, float* x, hipStream_t s);
int wg_couple(int B, const WgCouple& p, hipStream_t s);
int wg_head(int B, int G, long N, const float* audio, const float* w, float* dst, hipStream_t s);
int wg_tail(int B, const WgTail& p, hipStream_t s);
int wg_logdet(const float* w, int c, int n, float* out, hipStream_t s);
int wg_nll_item(int n_flows, int B, int nblk, long L, int G, float sigma, const double* part_s, const double* part_z, const float* logdet_w, double* sums,
                double* item, float* nll_item, hipStream_t s);
int wg_nll_loss(int n_flows, int B, long L, const double* item, const float* logdet_w, float* logdet, float* loss, hipStream_t s);
int wg_wgrad(const WgGrad& p, hipStream_t s);
int wg_wgrad_reduce(const WgGrad& p, hipStream_t s);
int wg_gate_bwd(int B, int nc, long L, int last, const float* dx, const float* d_out, const float* packed_t, const float* t, const float* g, float* du,
                float* acts, hipStream_t s);
int wg_data_bwd(int B, int rows, int nc, long L, int taps, int d, int first, const float* du, const float* packed_t, float* y, hipStream_t s);
int wg_tail_bwd(int B, const WgTailBwd& p, hipStream_t s);
int wg_finish(const double* part, size_t nslots, size_t stride, float* d0, int n0, float* d1, int n1, float* d2, int n2, hipStream_t s);
int wg_head_bwd(int B, int G, long N, const float* d_in, const float* audio, double* part, float* dw, hipStream_t s);      // the partials and their wg_finish
int wg_start_bwd(int B, int nc, int ctot, int n_half, long L, const float* dx, const float* w, float* d_in, hipStream_t s);
int wg_up_bwd(int B, int n_mel, int T, int G, long n_samples, const float* mel, const float* d_spect, float* dw, float* db, hipStream_t s);      // weight, then bias

}  // namespace t2
