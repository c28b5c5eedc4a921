// WaveGlow (Prenger et al. 2018), both directions of the flow.  Inference, mel spectrogram -> waveform, replaces the reference's
// glow.py: WaveGlow.infer (:251-293), WN.forward (:153-175), Invertible1x1Conv.forward(reverse=True) (:88-97).  Analysis,
// waveform -> z with log_s, log det W and the negative log-likelihood (values only, no gradient), replaces WaveGlow.forward
// (:207-249), Invertible1x1Conv.forward (:98-102) and WaveGlowLoss (:48-59): the WN is the same in both directions, so it runs
// the same upsample / start / gated conv / res_skip kernels, with a head kernel (regroup + W_0), one tail kernel per flow (end,
// exp(s) * a1 + b, the early-output split, the next flow's W, fp64 partial sums of s and z^2) and two small kernels that finish
// the sums in a fixed order.  log |det W_k| comes from an fp64 LU, once per set of weights.
//
// Training (waveglow/train.py:125-137): the forward direction with the activations the backward reads kept in a caller-owned
// buffer (per flow audio_in and out, per layer x_i, tanh(u_a), sigmoid(u_b)), and the backward.
//
// Here: the drivers and the C ABI.  A driver takes its plan, checks the pointers, places its buffers from the plan's carve and
// runs the launch sequence, every launch through WG_RUN.  The kernels and their launchers are in waveglow_kernels.hip; the tensor
// table, the layouts, the carves, the weight-gradient descriptor and the plans in waveglow_plan.hip.
#include "waveglow.h"

namespace t2 {

static int wg_copy(float* dst, const float* src, size_t n, hipStream_t s) {
    T2_CHECK_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

static int wg_pack_model(const t2_waveglow_config& c, const float* const* t, int n, float* packed, hipStream_t s) {
    WgLayout L;
    T2_TRY_RC(wg_layout(c, &L));
    const WgTensors& tt = L.tt;
    T2_REQUIRE(t && packed, "t2_waveglow_pack: null pointer");
    T2_REQUIRE(n == tt.count(), "t2_waveglow_pack: %d tensors given, the configuration has %d", n, tt.count());
    for (int i = 0; i < n; ++i) T2_REQUIRE(t[i], "t2_waveglow_pack: tensor %d is null", i);
    const int nc = c.n_channels, n_cond = c.n_mel_channels * c.n_group;
    auto copy = [&](size_t dst, int tensor) { return wg_copy(packed + dst, t[tensor], wg_tensor_floats(c, L, tensor), s); };
    T2_TRY_RC(wg_pack(kWgUpsample, t[tt.up_w()], nullptr, packed + L.up_w, c.n_mel_channels, c.n_mel_channels, 0, s));
    T2_TRY_RC(copy(L.up_b, tt.up_b()));
    for (int k = 0; k < c.n_flows; ++k) {
        const WgFlow& f = L.flows[k];
        T2_TRY_RC(copy(f.start_w, tt.start_w(k)));
        T2_TRY_RC(copy(f.start_b, tt.start_b(k)));
        T2_TRY_RC(copy(f.cond_b, tt.cond_b(k)));
        for (int i = 0; i < c.n_layers; ++i) {
            T2_TRY_RC(wg_pack(kWgGated, t[tt.in_w(k, i)], t[tt.cond_w(k)] + (size_t)2 * nc * i * n_cond, packed + f.gated[i], nc, nc, n_cond, s));
            T2_TRY_RC(copy(f.in_b[i], tt.in_b(k, i)));
        }
        for (int i = 0; i < c.n_layers; ++i) {
            T2_TRY_RC(wg_pack(kWgResSkip, t[tt.rs_w(k, i)], nullptr, packed + f.rs[i], i < c.n_layers - 1 ? 2 * nc : nc, nc, 0, s));
            T2_TRY_RC(copy(f.rs_b[i], tt.rs_b(k, i)));
        }
        T2_TRY_RC(copy(f.end_w, tt.end_w(k)));
        T2_TRY_RC(copy(f.end_b, tt.end_b(k)));
        T2_TRY_RC(copy(f.winv, tt.mix(k)));
    }
    return 0;
}

static int wg_pack_backward(const t2_waveglow_config& c, const float* const* t, int n, float* packed, hipStream_t s) {
    WgLayout lay;
    WgBwdLayout bl;
    T2_TRY_RC(wg_layout(c, &lay));
    wg_bwd_layout(c, lay, &bl);
    const WgTensors& tt = lay.tt;
    T2_REQUIRE(t && packed, "t2_waveglow_pack_backward: null pointer");
    T2_REQUIRE(n == tt.count(), "t2_waveglow_pack_backward: %d tensors given, the configuration has %d", n, tt.count());
    for (int i = 0; i < n; ++i) T2_REQUIRE(t[i], "t2_waveglow_pack_backward: tensor %d is null", i);
    const int nc = c.n_channels, n_cond = c.n_mel_channels * c.n_group, nl = c.n_layers;
    for (int k = 0; k < c.n_flows; ++k)
        for (int i = 0; i < nl; ++i) {
            T2_TRY_RC(wg_pack_conv_t(t[tt.in_w(k, i)], packed + bl.flows[k].conv_t[i], nc, s));
            T2_TRY_RC(wg_pack_cond_t(t[tt.cond_w(k)] + (size_t)2 * nc * i * n_cond, packed + bl.flows[k].cond_t[i], nc, n_cond, s));
            T2_TRY_RC(wg_pack_rs_t(t[tt.rs_w(k, i)], packed + bl.flows[k].rs_t[i], nc, i == nl - 1, s));
        }
    return 0;
}

static int wg_logdet_model(const t2_waveglow_config& c, const float* packed, float* logdet, hipStream_t s) {
    WgLayout lay;
    T2_TRY_RC(wg_layout(c, &lay));
    T2_REQUIRE(packed && logdet, "t2_waveglow_logdet: null pointer");
    for (int k = 0; k < c.n_flows; ++k) T2_TRY_RC(wg_logdet(packed + lay.flows[k].winv, lay.flows[k].c, 1, logdet + k, s));
    return 0;
}

// kernel_ms_host: an event in front of (mark) and behind (timed) every launch, added up per kernel kind at the end (finish)
struct WgTimer {
    double* ms; int n_kinds; hipStream_t s; const char* who;
    std::vector<hipEvent_t> ev;
    std::vector<int> kinds;
    void mark() {
        if (ms) {
            hipEvent_t e;
            if (hipEventCreate(&e) == hipSuccess && hipEventRecord(e, s) == hipSuccess) ev.push_back(e);
        }
    }
    int timed(int kind, int r) {
        if (ms && r == 0) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess || hipEventRecord(e, s) != hipSuccess) { t2_set_error("%s: event failed", who); return -2; }
            ev.push_back(e); kinds.push_back(kind);
        }
        return r;
    }
    int finish(int rc) {
        if (ms) {
            for (int i = 0; i < n_kinds; ++i) ms[i] = 0.0;
            if (rc == 0 && hipStreamSynchronize(s) != hipSuccess) { t2_set_error("%s: synchronising for the kernel times failed", who); rc = -2; }
            for (size_t i = 0; rc == 0 && i + 1 < ev.size() && i / 2 < kinds.size(); i += 2) {
                float t = 0.f;
                if (hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess) ms[kinds[i / 2]] += t;
            }
            for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        }
        return rc;
    }
};
#define WG_RUN(kind, call)                      \
    do {                                        \
        tm.mark();                              \
        rc = tm.timed(kind, call);              \
        if (rc != 0) goto done;                 \
    } while (0)

static int wg_infer(const t2_waveglow_config& c, const t2_waveglow_infer_args& a, hipStream_t s) {
    WgLayout lay;
    WgInferPlan pl;
    T2_TRY_RC(wg_layout(c, &lay));
    T2_REQUIRE(a.n_mel == c.n_mel_channels, "t2_waveglow_infer: the mel has %d channels, the model takes %d", a.n_mel, c.n_mel_channels);
    T2_TRY_RC(wg_plan(c, lay, a.B, a.T, &pl));
    T2_REQUIRE(a.packed && a.mel && a.workspace && a.audio && a.noise_host, "t2_waveglow_infer: null pointer");
    T2_REQUIRE(a.n_noise == lay.n_planes, "t2_waveglow_infer: %d noise planes given, the model draws %d", a.n_noise, lay.n_planes);
    for (int i = 0; i < a.n_noise; ++i) T2_REQUIRE(a.noise_host[i], "t2_waveglow_infer: noise plane %d is null", i);
    const int B = a.B, nc = c.n_channels, G = c.n_group, n_cond = c.n_mel_channels * G;
    const long L = pl.info.L;
    const WgFlowWs& ws = pl.ws;
    float* spect = a.workspace + ws.spect; float* x = a.workspace + ws.x; float* out = a.workspace + ws.out; float* acts = a.workspace + ws.acts;
    float* bufs[2] = {a.workspace + ws.bufs[0], a.workspace + ws.bufs[1]};

    WgTimer tm{a.kernel_ms_host, T2_WAVEGLOW_KERNELS, s, "t2_waveglow_infer"};
    int rc = 0;
    {
        WG_RUN(0, wg_upsample(B, c.n_mel_channels, a.T, G, (long)a.T * kWgUpStride, a.mel, a.packed + lay.up_w, a.packed + lay.up_b,
                              spect, s));
        const float* src = a.noise_host[0];
        float scale = a.sigma;
        int plane = 1, cur = 0;
        for (int k = c.n_flows - 1; k >= 0; --k) {
            const WgFlow& f = lay.flows[k];
            WG_RUN(1, wg_start(B, nc, f.c, f.n_half, L, scale, src, a.packed + f.start_w, a.packed + f.start_b, x, s));
            for (int i = 0; i < c.n_layers; ++i) {
                WG_RUN(2, wg_gated(B, nc, n_cond, L, 1 << i, 0, x, spect, a.packed + f.gated[i], a.packed + f.in_b[i],
                                   a.packed + f.cond_b + (size_t)2 * nc * i, acts, s));
                WG_RUN(3, wg_res_skip(B, nc, L, i == 0, i == c.n_layers - 1, acts, a.packed + f.rs[i], a.packed + f.rs_b[i], x, out, s));
            }
            WgCouple p{out, a.packed + f.end_w, a.packed + f.end_b, src, a.packed + f.winv, f.early ? a.noise_host[plane] : nullptr,
                       k == 0 ? a.flow_audio : bufs[cur], k == 0 ? a.audio : nullptr, nc, f.n_half, f.early ? c.n_early_size : 0, L, scale, a.sigma};
            if (f.early) ++plane;
            WG_RUN(4, wg_couple(B, p, s));
            src = bufs[cur]; cur ^= 1; scale = 1.f;
        }
        if (a.spect) rc = wg_copy(a.spect, spect, (size_t)B * n_cond * L, s);
    }
done:
    return tm.finish(rc);
}

// saved: null for analyze / nll; the training forward's buffer of wg_saved(..).total floats otherwise: the same launches in the
// same order on the same packed weights, with the activations the backward reads left in `saved` instead of the workspace.
static int wg_forward(const t2_waveglow_config& c, const t2_waveglow_forward_args& a, hipStream_t s, float* saved = nullptr) {
    WgForwardPlan pl;
    T2_TRY_RC(wg_forward_plan(c, a.B, a.T, a.n_samples, &pl));      // judges the configuration first
    T2_REQUIRE(a.n_mel == c.n_mel_channels, "t2_waveglow_forward: the mel has %d channels, the model takes %d", a.n_mel, c.n_mel_channels);
    const bool want_sums = a.sums || a.nll_item || a.loss;
    T2_REQUIRE(a.packed && a.mel && a.audio && a.workspace && (a.z || want_sums), "t2_waveglow_forward: null pointer");
    T2_REQUIRE(a.logdet_w || !(want_sums || a.logdet), "t2_waveglow_forward: logdet_w is null, but a sum or logdet is asked for");
    T2_REQUIRE(!want_sums || a.sigma > 0.f, "t2_waveglow_forward: sigma=%g must be positive", (double)a.sigma);
    for (int k = 0; a.log_s_host && k < c.n_flows; ++k) T2_REQUIRE(a.log_s_host[k], "t2_waveglow_forward: log_s pointer %d is null", k);
    const WgLayout& lay = pl.lay;
    const int B = a.B, nc = c.n_channels, G = c.n_group, n_cond = c.n_mel_channels * G, nblk = (int)pl.info.n_blocks;
    const long L = pl.info.L;
    const WgFlowWs& ws = pl.ws;
    float* spect = a.workspace + ws.spect; float* x = a.workspace + ws.x; float* out = a.workspace + ws.out; float* acts = a.workspace + ws.acts;
    float* bufs[2] = {a.workspace + ws.bufs[0], a.workspace + ws.bufs[1]};
    double* part = reinterpret_cast<double*>(a.workspace + ws.part_s);
    double* part_z = reinterpret_cast<double*>(a.workspace + ws.part_z);
    double* item = reinterpret_cast<double*>(a.workspace + ws.item);
    double* sums = a.sums ? a.sums : reinterpret_cast<double*>(a.workspace + ws.sums);

    WgSaved sv;
    if (saved) { sv = wg_saved(c, lay, B, L); spect = saved; }

    WgTimer tm{a.kernel_ms_host, T2_WAVEGLOW_FORWARD_KERNELS, s, "t2_waveglow_forward"};
    int rc = 0;
    {
        WG_RUN(0, wg_upsample(B, c.n_mel_channels, a.T, G, L * G, a.mel, a.packed + lay.up_w, a.packed + lay.up_b, spect, s));
        if (saved) bufs[0] = saved + sv.ain(0);
        WG_RUN(4, wg_head(B, G, a.n_samples, a.audio, a.packed + lay.flows[0].winv, bufs[0], s));
        int cur = 0, zoff = 0;
        for (int k = 0; k < c.n_flows; ++k) {
            const WgFlow& f = lay.flows[k];
            const WgFlow* next = k + 1 < c.n_flows ? &lay.flows[k + 1] : nullptr;
            if (saved) { x = saved + sv.x(k, 0); out = saved + sv.out(k); if (next) bufs[cur ^ 1] = saved + sv.ain(k + 1); }
            WG_RUN(1, wg_start(B, nc, f.c, f.n_half, L, 1.f, bufs[cur], a.packed + f.start_w, a.packed + f.start_b, x, s));
            for (int i = 0; i < c.n_layers; ++i) {
                const bool last = i == c.n_layers - 1;
                float* xi = saved ? saved + sv.x(k, i) : x;                        // kept: layer i reads x_i and writes x_{i+1}
                float* xn = saved && !last ? saved + sv.x(k, i + 1) : xi;
                WG_RUN(2, wg_gated(B, nc, n_cond, L, 1 << i, 0, xi, spect, a.packed + f.gated[i], a.packed + f.in_b[i],
                                   a.packed + f.cond_b + (size_t)2 * nc * i, acts, s, saved ? saved + sv.t(k, i) : nullptr,
                                   saved ? saved + sv.g(k, i) : nullptr));
                WG_RUN(3, wg_res_skip(B, nc, L, i == 0, last, acts, a.packed + f.rs[i], a.packed + f.rs_b[i], xn, out, s, xi));
            }
            WgTail p{out, a.packed + f.end_w, a.packed + f.end_b, bufs[cur], next ? a.packed + next->winv : nullptr,
                     next ? bufs[cur ^ 1] : nullptr, a.z, a.log_s_host ? a.log_s_host[k] : nullptr,
                     want_sums ? part + (size_t)k * B * nblk : nullptr, want_sums ? part_z + (size_t)k * B * nblk : nullptr,
                     nc, f.n_half, next ? f.c - next->c : f.c, G, zoff, L};
            WG_RUN(5, wg_tail(B, p, s));
            zoff += p.n_peel; cur ^= 1;
        }
        if (want_sums) WG_RUN(6, wg_nll_item(c.n_flows, B, nblk, L, G, a.sigma, part, part_z, a.logdet_w, sums, item, a.nll_item, s));
        if (a.logdet || a.loss) WG_RUN(6, wg_nll_loss(c.n_flows, B, L, item, a.logdet_w, a.logdet, a.loss, s));
    }
done:
    return tm.finish(rc);
}

// the backward of the forward direction: gradients of every folded tensor from dz and the dlog_s[k]
static int wg_backward(const t2_waveglow_config& c, const t2_waveglow_backward_args& a, hipStream_t s) {
    WgBackwardPlan pl;
    T2_TRY_RC(wg_backward_plan(c, a.B, a.T, a.n_samples, &pl));
    T2_REQUIRE(a.n_mel == c.n_mel_channels, "t2_waveglow_backward: the mel has %d channels, the model takes %d", a.n_mel, c.n_mel_channels);
    T2_REQUIRE(a.packed && a.packed_bwd && a.saved && a.mel && a.audio && a.workspace && a.grad, "t2_waveglow_backward: null pointer");
    const WgLayout& lay = pl.lay;
    const WgTensors& tt = lay.tt;
    const WgSaved& sv = pl.sv;
    const WgBwdWs& ws = pl.ws;
    const int B = a.B, nc = c.n_channels, G = c.n_group, n_cond = c.n_mel_channels * G, nl = c.n_layers, nf = c.n_flows;
    const long L = pl.info.L;
    float* dx = a.workspace + ws.dx; float* d_out = a.workspace + ws.d_out; float* du = a.workspace + ws.du; float* acts = a.workspace + ws.acts;
    float* d_spect = a.workspace + ws.d_spect;
    float* dbuf[2] = {a.workspace + ws.dbuf[0], a.workspace + ws.dbuf[1]};
    float* gpart = a.workspace + ws.gpart;
    double* tpart = reinterpret_cast<double*>(a.workspace + ws.tpart);
    const float* spect = a.saved;
    auto grad = [&](int tensor) { return a.grad + pl.bl.grad[tensor]; };
    std::vector<int> zoff(nf, 0);
    for (int k = 0, z = 0; k < nf; ++k) { zoff[k] = z; z += k + 1 < nf ? lay.flows[k].c - lay.flows[k + 1].c : lay.flows[k].c; }

    WgTimer tm{a.kernel_ms_host, T2_WAVEGLOW_BACKWARD_KERNELS, s, "t2_waveglow_backward"};
    int rc = 0;
    {
        for (int k = nf - 1; k >= 0; --k) {
            const WgFlow& f = lay.flows[k];
            const WgBwdFlow& bf = pl.bl.flows[k];
            const WgFlow* next = k + 1 < nf ? &lay.flows[k + 1] : nullptr;
            const int Cn = next ? next->c : 0;
            float* d_in = dbuf[k & 1];
            WgTailBwd tp{a.saved + sv.out(k), a.packed + f.end_w, a.packed + f.end_b, a.saved + sv.ain(k), next ? a.packed + next->winv : nullptr,
                         next ? dbuf[(k + 1) & 1] : nullptr, a.dz, a.dlog_s_host ? a.dlog_s_host[k] : nullptr, d_out, d_in, tpart,
                         nc, f.n_half, next ? f.c - next->c : f.c, G, zoff[k], L};
            WG_RUN(0, wg_tail_bwd(B, tp, s));
            WG_RUN(0, wg_finish(tpart, pl.info.n_slots, (size_t)f.c * nc + f.c + Cn * Cn, grad(tt.end_w(k)), f.c * nc, grad(tt.end_b(k)), f.c,
                                next ? grad(tt.mix(k + 1)) : nullptr, Cn * Cn, s));
            for (int i = nl - 1; i >= 0; --i) {
                const bool last = i == nl - 1;
                WG_RUN(1, wg_gate_bwd(B, nc, L, last, dx, d_out, a.packed_bwd + bf.rs_t[i], a.saved + sv.t(k, i), a.saved + sv.g(k, i), du, acts, s));
                for (int half = last ? 1 : 0; half < 2; ++half) {        // rows [:nc] of res_skip take dx, rows [nc:] (all, on the last layer) d_out
                    const size_t row0 = half && !last ? nc : 0;
                    const WgGrad gp = wg_grad_desc(wg_site_res_skip(nc), half ? d_out : dx, nc, acts, nc, 0, nullptr,
                                                   WgGradOut{grad(tt.rs_w(k, i)) + row0 * nc, nullptr, grad(tt.rs_b(k, i)) + row0, nullptr}, B, L, gpart);
                    WG_RUN(4, wg_wgrad(gp, s));
                    WG_RUN(5, wg_wgrad_reduce(gp, s));
                }
                {
                    const WgGradOut to{grad(tt.in_w(k, i)), grad(tt.cond_w(k)) + (size_t)2 * nc * i * n_cond, grad(tt.in_b(k, i)), grad(tt.cond_b(k)) + (size_t)2 * nc * i};
                    const WgGrad gp = wg_grad_desc(wg_site_conv(nc, n_cond), du, 2 * nc, a.saved + sv.x(k, i), nc, 1 << i, spect, to, B, L, gpart);
                    WG_RUN(4, wg_wgrad(gp, s));
                    WG_RUN(5, wg_wgrad_reduce(gp, s));
                }
                WG_RUN(2, wg_data_bwd(B, nc, nc, L, 3, 1 << i, last, du, a.packed_bwd + bf.conv_t[i], dx, s));
                WG_RUN(3, wg_data_bwd(B, n_cond, nc, L, 1, 0, k == nf - 1 && last, du, a.packed_bwd + bf.cond_t[i], d_spect, s));
            }
            WG_RUN(6, wg_start_bwd(B, nc, f.c, f.n_half, L, dx, a.packed + f.start_w, d_in, s));
            {
                const WgGrad gp = wg_grad_desc(wg_site_start(nc, f.n_half), dx, nc, a.saved + sv.ain(k), f.c, 0, nullptr,
                                               WgGradOut{grad(tt.start_w(k)), nullptr, grad(tt.start_b(k)), nullptr}, B, L, gpart);
                WG_RUN(4, wg_wgrad(gp, s));
                WG_RUN(5, wg_wgrad_reduce(gp, s));
            }
        }
        WG_RUN(0, wg_head_bwd(B, G, a.n_samples, dbuf[0], a.audio, tpart, grad(tt.mix(0)), s));
        WG_RUN(7, wg_up_bwd(B, c.n_mel_channels, a.T, G, L * G, a.mel, d_spect, grad(tt.up_w()), grad(tt.up_b()), s));
    }
done:
    return tm.finish(rc);
}
#undef WG_RUN

}  // namespace t2

// ---- C ABI (include/t2amd.h)
using namespace t2;
static_assert(T2_VOCODER_TIME_TILE == kVocTT, "t2amd.h mirrors the time tile");

extern "C" {

int t2_waveglow_plan(const t2_waveglow_config* cfg, int B, int T, t2_waveglow_plan_info* out) {
    T2_REQUIRE(cfg && out, "t2_waveglow_plan: null pointer");
    WgLayout lay;
    WgInferPlan pl;
    T2_TRY_RC(wg_layout(*cfg, &lay));
    T2_TRY_RC(wg_plan(*cfg, lay, B, T, &pl));
    *out = pl.info;
    return 0;
}
int t2_waveglow_pack(const t2_waveglow_config* cfg, const float* const* tensors_host, int n_tensors, float* packed, void* stream) {
    T2_REQUIRE(cfg, "t2_waveglow_pack: null configuration");
    return wg_pack_model(*cfg, tensors_host, n_tensors, packed, (hipStream_t)stream);
}
int t2_waveglow_infer(const t2_waveglow_config* cfg, const t2_waveglow_infer_args* a, void* stream) {
    T2_REQUIRE(cfg && a, "t2_waveglow_infer: null pointer");
    return wg_infer(*cfg, *a, (hipStream_t)stream);
}
size_t t2_waveglow_packed_floats(int kind, int rows, int k0, int k1) {
    return kind >= kWgGated && kind <= kWgUpsample && rows > 0 && k0 > 0 && k1 >= 0 ? wg_packed_floats(kind, rows, k0, k1) : 0;
}
int t2_waveglow_gated_conv(const t2_waveglow_gated_args* a, void* stream) {
    T2_REQUIRE(a, "t2_waveglow_gated_conv: null arguments");
    T2_TRY_RC(wg_gated_check(a->B, a->nc, a->n_cond, a->L, a->d));
    T2_REQUIRE(a->w_in && a->w_cond && a->packed_ws, "t2_waveglow_gated_conv: null weights or packing scratch");
    T2_TRY_RC(wg_pack(kWgGated, a->w_in, a->w_cond, a->packed_ws, a->nc, a->nc, a->n_cond, (hipStream_t)stream));
    return wg_gated(a->B, a->nc, a->n_cond, a->L, a->d, a->raw, a->x, a->spect, a->packed_ws, a->b_in, a->b_cond, a->y, (hipStream_t)stream);
}
int t2_waveglow_res_skip(const t2_waveglow_res_skip_args* a, void* stream) {
    T2_REQUIRE(a, "t2_waveglow_res_skip: null arguments");
    T2_TRY_RC(wg_check_nc("waveglow res_skip", a->nc));
    T2_REQUIRE(a->w && a->packed_ws, "t2_waveglow_res_skip: null weights or packing scratch");
    T2_TRY_RC(wg_pack(kWgResSkip, a->w, nullptr, a->packed_ws, a->last ? a->nc : 2 * a->nc, a->nc, 0, (hipStream_t)stream));
    return wg_res_skip(a->B, a->nc, a->L, a->first, a->last, a->acts, a->packed_ws, a->bias, a->x, a->out, (hipStream_t)stream);
}
int t2_waveglow_upsample(const t2_waveglow_upsample_args* a, void* stream) {
    T2_REQUIRE(a, "t2_waveglow_upsample: null arguments");
    T2_REQUIRE(a->n_mel >= 1 && a->n_mel <= 512, "waveglow upsample: n_mel_channels=%d outside 1..512", a->n_mel);
    T2_REQUIRE(a->w && a->packed_ws, "t2_waveglow_upsample: null weights or packing scratch");
    T2_TRY_RC(wg_pack(kWgUpsample, a->w, nullptr, a->packed_ws, a->n_mel, a->n_mel, 0, (hipStream_t)stream));
    return wg_upsample(a->B, a->n_mel, a->T, a->n_group, (long)a->T * kWgUpStride, a->mel, a->packed_ws, a->bias, a->spect, (hipStream_t)stream);
}
int t2_waveglow_couple(const t2_waveglow_couple_args* a, void* stream) {
    T2_REQUIRE(a, "t2_waveglow_couple: null arguments");
    return wg_couple(a->B, WgCouple{a->out, a->w_end, a->b_end, a->audio_in, a->w_inverse, a->z, a->audio_out, a->audio_interleaved, a->nc, a->n_half,
                                    a->n_early, (long)a->L, a->in_scale, a->sigma}, (hipStream_t)stream);
}
int t2_waveglow_forward_plan(const t2_waveglow_config* cfg, int B, int T, long n_samples, t2_waveglow_forward_info* out) {
    T2_REQUIRE(cfg && out, "t2_waveglow_forward_plan: null pointer");
    WgForwardPlan pl;
    T2_TRY_RC(wg_forward_plan(*cfg, B, T, n_samples, &pl));
    *out = pl.info;
    return 0;
}
int t2_waveglow_forward(const t2_waveglow_config* cfg, const t2_waveglow_forward_args* a, void* stream) {
    T2_REQUIRE(cfg && a, "t2_waveglow_forward: null pointer");
    return wg_forward(*cfg, *a, (hipStream_t)stream);
}
int t2_waveglow_logdet(const t2_waveglow_config* cfg, const float* packed, float* logdet, void* stream) {
    T2_REQUIRE(cfg, "t2_waveglow_logdet: null configuration");
    return wg_logdet_model(*cfg, packed, logdet, (hipStream_t)stream);
}
int t2_waveglow_logdet_matrices(const float* w, int c, int n, float* out, void* stream) { return wg_logdet(w, c, n, out, (hipStream_t)stream); }
int t2_waveglow_head(const t2_waveglow_head_args* a, void* stream) {
    T2_REQUIRE(a, "t2_waveglow_head: null arguments");
    return wg_head(a->B, a->n_group, a->n_samples, a->audio, a->w, a->audio_out, (hipStream_t)stream);
}
int t2_waveglow_tail(const t2_waveglow_tail_args* a, void* stream) {
    T2_REQUIRE(a, "t2_waveglow_tail: null arguments");
    T2_REQUIRE(!a->part_s == !a->part_z, "t2_waveglow_tail: part_s and part_z go together");
    return wg_tail(a->B, WgTail{a->out, a->w_end, a->b_end, a->audio_in, a->w_next, a->audio_out, a->z, a->log_s, a->part_s, a->part_z, a->nc, a->n_half,
                                a->n_peel, a->n_group, a->z_offset, (long)a->L}, (hipStream_t)stream);
}

int t2_waveglow_backward_plan(const t2_waveglow_config* cfg, int B, int T, long n_samples, t2_waveglow_backward_info* out) {
    T2_REQUIRE(cfg && out, "t2_waveglow_backward_plan: null pointer");
    WgBackwardPlan pl;
    T2_TRY_RC(wg_backward_plan(*cfg, B, T, n_samples, &pl));
    *out = pl.info;
    return 0;
}
int t2_waveglow_grad_offsets(const t2_waveglow_config* cfg, size_t* offsets_host, int n_tensors) {
    T2_REQUIRE(cfg && offsets_host, "t2_waveglow_grad_offsets: null pointer");
    WgLayout lay;
    WgBwdLayout bl;
    T2_TRY_RC(wg_layout(*cfg, &lay));
    wg_bwd_layout(*cfg, lay, &bl);
    T2_REQUIRE(n_tensors == lay.tt.count(), "t2_waveglow_grad_offsets: room for %d tensors, the configuration has %d", n_tensors, lay.tt.count());
    for (int i = 0; i < n_tensors; ++i) offsets_host[i] = bl.grad[i];
    return 0;
}
int t2_waveglow_pack_backward(const t2_waveglow_config* cfg, const float* const* tensors_host, int n_tensors, float* packed_bwd, void* stream) {
    T2_REQUIRE(cfg, "t2_waveglow_pack_backward: null configuration");
    return wg_pack_backward(*cfg, tensors_host, n_tensors, packed_bwd, (hipStream_t)stream);
}
int t2_waveglow_train_forward(const t2_waveglow_config* cfg, const t2_waveglow_train_forward_args* a, void* stream) {
    T2_REQUIRE(cfg && a && a->saved, "t2_waveglow_train_forward: null pointer");
    return wg_forward(*cfg, a->fwd, (hipStream_t)stream, a->saved);
}
int t2_waveglow_backward(const t2_waveglow_config* cfg, const t2_waveglow_backward_args* a, void* stream) {
    T2_REQUIRE(cfg && a, "t2_waveglow_backward: null pointer");
    return wg_backward(*cfg, *a, (hipStream_t)stream);
}
size_t t2_waveglow_weight_grad_ws_floats(int M, int nc, int n_cond, int taps, int B, int L) {
    if (M < 1 || nc < 1 || n_cond < 0 || (taps != 1 && taps != 3) || B < 1 || L < 1) return 0;
    return wg_grad_part_floats(WgGradSite{M, nc, taps, n_cond}, B, L);
}
int t2_waveglow_weight_grad(const t2_waveglow_weight_grad_args* a, void* stream) {
    const char* who = "waveglow weight gradient";
    T2_REQUIRE(a, "t2_waveglow_weight_grad: null arguments");
    T2_TRY_RC(wg_check_common(who, a->B, a->L));
    T2_REQUIRE(a->M >= 1 && a->M <= 1024 && a->nc >= 1 && a->nc <= 512 && a->n_cond >= 0, "%s: M=%d, nc=%d, n_cond=%d", who, a->M, a->nc, a->n_cond);
    T2_REQUIRE((a->taps == 1 && a->d == 0) || (a->taps == 3 && a->d >= 1 && a->d <= kWgMaxD), "%s: taps=%d, d=%d", who, a->taps, a->d);
    T2_REQUIRE(a->a && a->x && a->dw_x && a->db && a->workspace && (a->n_cond == 0 || (a->spect && a->dw_spect)), "%s: null pointer", who);
    T2_REQUIRE((a->a_rows == 0 || a->a_rows >= a->M) && (a->x_rows == 0 || a->x_rows >= a->nc), "%s: a_rows=%d, x_rows=%d are fewer than M=%d, nc=%d", who,
               a->a_rows, a->x_rows, a->M, a->nc);
    const WgGrad gp = wg_grad_desc(WgGradSite{a->M, a->nc, a->taps, a->n_cond}, a->a, a->a_rows ? a->a_rows : a->M, a->x, a->x_rows ? a->x_rows : a->nc, a->d,
                                   a->spect, WgGradOut{a->dw_x, a->dw_spect, a->db, a->db2}, a->B, a->L, a->workspace);
    T2_TRY_RC(wg_wgrad(gp, (hipStream_t)stream));
    return wg_wgrad_reduce(gp, (hipStream_t)stream);
}
int t2_waveglow_gate_backward(const t2_waveglow_gate_backward_args* a, void* stream) {
    T2_REQUIRE(a, "t2_waveglow_gate_backward: null arguments");
    T2_TRY_RC(wg_check_nc("waveglow gate backward", a->nc));
    T2_REQUIRE(a->w_rs && a->packed_ws, "t2_waveglow_gate_backward: null weights or packing scratch");
    T2_TRY_RC(wg_pack_rs_t(a->w_rs, a->packed_ws, a->nc, a->last, (hipStream_t)stream));
    return wg_gate_bwd(a->B, a->nc, a->L, a->last, a->dx, a->d_out, a->packed_ws, a->t, a->g, a->du, a->acts, (hipStream_t)stream);
}
int t2_waveglow_conv_backward(const t2_waveglow_conv_backward_args* a, void* stream) {
    T2_REQUIRE(a, "t2_waveglow_conv_backward: null arguments");
    T2_TRY_RC(wg_check_nc("waveglow conv backward", a->nc));
    T2_REQUIRE(a->n_cond >= 8 && a->n_cond % 8 == 0, "waveglow conv backward: %d conditioning channels, must be a positive multiple of 8", a->n_cond);
    T2_REQUIRE(a->w_in && a->w_cond && a->packed_ws, "t2_waveglow_conv_backward: null weights or packing scratch");
    float* pc = a->packed_ws + wg_packed_t_floats(a->nc, 2 * a->nc, 3, 0);
    T2_TRY_RC(wg_pack_conv_t(a->w_in, a->packed_ws, a->nc, (hipStream_t)stream));
    T2_TRY_RC(wg_pack_cond_t(a->w_cond, pc, a->nc, a->n_cond, (hipStream_t)stream));
    T2_TRY_RC(wg_data_bwd(a->B, a->nc, a->nc, a->L, 3, a->d, a->first_dx, a->du, a->packed_ws, a->dx, (hipStream_t)stream));
    return wg_data_bwd(a->B, a->n_cond, a->nc, a->L, 1, 0, a->first_spect, a->du, pc, a->d_spect, (hipStream_t)stream);
}
size_t t2_waveglow_conv_backward_packed_floats(int nc, int n_cond) {
    return nc > 0 && n_cond > 0 ? wg_packed_t_floats(nc, 2 * nc, 3, 0) + wg_packed_t_floats(n_cond, 2 * nc, 1, 0) : 0;
}
int t2_waveglow_tail_backward(const t2_waveglow_tail_backward_args* a, void* stream) {
    T2_REQUIRE(a, "t2_waveglow_tail_backward: null arguments");
    T2_REQUIRE(a->dw_end && a->db_end, "t2_waveglow_tail_backward: null pointer");
    const int C = 2 * a->n_half, Cn = C - a->n_peel;
    T2_TRY_RC(wg_tail_bwd(a->B, WgTailBwd{a->out, a->w_end, a->b_end, a->audio_in, a->w_next, a->d_next, a->dz, a->dlog_s, a->d_out, a->d_in, a->part, a->nc,
                                         a->n_half, a->n_peel, a->n_group, a->z_offset, (long)a->L}, (hipStream_t)stream));
    T2_REQUIRE(Cn == 0 || a->dw_next, "t2_waveglow_tail_backward: dw_next is null");
    return wg_finish(a->part, (size_t)a->B * ((a->L + 255) / 256) * 4, (size_t)C * a->nc + C + Cn * Cn, a->dw_end, C * a->nc, a->db_end, C, a->dw_next, Cn * Cn,
                     (hipStream_t)stream);
}
int t2_waveglow_start_backward(const t2_waveglow_start_backward_args* a, void* stream) {
    const char* who = "waveglow start backward";
    T2_REQUIRE(a, "t2_waveglow_start_backward: null arguments");
    T2_TRY_RC(wg_check_common(who, a->B, a->L));
    T2_TRY_RC(wg_check_nc(who, a->nc));
    T2_REQUIRE(a->n_half >= 1 && a->n_half <= 4 && a->c >= 2 * a->n_half && a->c <= 8, "%s: n_half=%d outside 1..4 or c=%d outside 2*n_half..8", who, a->n_half, a->c);
    T2_REQUIRE(a->dx && a->w_start && a->audio_in && a->d_in && a->dw_start && a->db_start && a->workspace, "%s: null pointer", who);
    T2_TRY_RC(wg_start_bwd(a->B, a->nc, a->c, a->n_half, a->L, a->dx, a->w_start, a->d_in, (hipStream_t)stream));
    const WgGrad gp = wg_grad_desc(wg_site_start(a->nc, a->n_half), a->dx, a->nc, a->audio_in, a->c, 0, nullptr, WgGradOut{a->dw_start, nullptr, a->db_start, nullptr},
                                   a->B, a->L, a->workspace);
    T2_TRY_RC(wg_wgrad(gp, (hipStream_t)stream));
    return wg_wgrad_reduce(gp, (hipStream_t)stream);
}
int t2_waveglow_head_backward(const t2_waveglow_head_backward_args* a, void* stream) {
    const char* who = "waveglow head backward";
    T2_REQUIRE(a, "t2_waveglow_head_backward: null arguments");
    T2_REQUIRE(a->n_group >= 2 && a->n_group <= 8 && a->n_group % 2 == 0, "%s: n_group=%d is not even and from 2 to 8", who, a->n_group);
    T2_REQUIRE(a->n_samples >= a->n_group, "%s: n_samples=%ld is shorter than one group of %d", who, a->n_samples, a->n_group);
    T2_TRY_RC(wg_check_common(who, a->B, a->n_samples / a->n_group));
    T2_REQUIRE(a->d_in && a->audio && a->part && a->dw, "%s: null pointer", who);
    return wg_head_bwd(a->B, a->n_group, a->n_samples, a->d_in, a->audio, a->part, a->dw, (hipStream_t)stream);
}
int t2_waveglow_upsample_backward(const t2_waveglow_upsample_backward_args* a, void* stream) {
    T2_REQUIRE(a, "t2_waveglow_upsample_backward: null arguments");
    return wg_up_bwd(a->B, a->n_mel, a->T, a->n_group, a->n_samples, a->mel, a->d_spect, a->dw, a->db, (hipStream_t)stream);
}

}  // extern "C"
