"""Dev tool: times of the HiFi-GAN multi-period discriminator on the GPU (``MultiPeriodDiscriminator``, csrc/vocoder_disc.hip) with
seeded weight-normed weights at the training shape of scripts/time_hifigan_train.py, B = 16 segments of 8192 samples, real and
generated together = 32 items per period discriminator:

  python scripts/time_hifigan_mpd.py [--shape 16x8192] [--warmup 3] [--reps 10] [--no-kernels]

From HIP events around --reps calls after --warmup calls:
  the steps       the discriminator step (y, y_hat.detach(): discriminator_loss, all parameter gradients), the generator step with
                  the gradient to y_hat only (feature_loss + generator_loss, parameters frozen) and as the reference's loop runs
                  it (the parameters' gradients too), and the forward alone under no_grad.  Real and generated audio run as one batch, so the
                  generator step also computes the real half's data gradients, which nobody reads: that work is in its figures.  Every figure of a path with a gradient
                  includes folding the weight norm and packing the forward and data-gradient weights, which happen on every call;
  per kernel kind unless --no-kernels, per period through the C entry points on the step's own shapes: the two packs, the forward
                  (six launches), the backward with the audio's gradient only (conv_post's and the four GEMM data gradients, the
                  audio's gather) and with everything; the weight gradients (six launches with their reduces) are the difference.
                  Useful FLOPs (2 * Cin * Cout * taps * output positions * items, per kind) as a share of the 157.3 TFLOP/s
                  fp32-matrix peak.
A run without a GPU fails."""
import argparse, ctypes as C, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="16x8192")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--no-kernels", action="store_true")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import hifigan_disc_ref as R
from tacotron2_subword_amd import _lib as L
from tacotron2_subword_amd.hifigan_infer.hifigan_model import MultiPeriodDiscriminator, discriminator_loss, feature_loss, generator_loss

assert torch.cuda.is_available(), "time_hifigan_mpd.py measures on the GPU: none found"
PEAK = 157.3e12
N = L.HIFIGAN_MPD_LAYERS


def event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def forward_flops(plan):
    return sum(2.0 * plan.C[i] * plan.C[i + 1] * (5 if i < 5 else 3) * plan.H[i + 1] * plan.period * plan.B for i in range(N))


def line(label, ms, fl):
    print(f"    {label:58s} {ms:9.3f} ms  {fl / 1e9:9.1f} GFLOP  {fl / (ms * 1e-3) / 1e12:6.2f} TFLOP/s = {100 * fl / (ms * 1e-3) / PEAK:5.2f} % of fp32-matrix peak",
          flush=True)


def kernel_report(mpd, B2, T):
    lib, dev, tot = L.lib(), "cuda", {}
    for d, disc in enumerate(mpd.discriminators):
        p = disc.period
        plan = L.hifigan_mpd_plan(p, B2, T)
        layers = list(disc.convs) + [disc.conv_post]
        with torch.no_grad():
            ws = [torch._weight_norm(l.weight_v, l.weight_g, 0).contiguous() for l in layers]
        wp, bp = (C.c_void_p * N)(*[L.ptr(w) for w in ws]), (C.c_void_p * N)(*[L.ptr(l.bias.detach()) for l in layers])
        packed, packed_bwd = torch.empty(plan.packed_bytes // 4, device=dev), torch.empty(plan.packed_bwd_bytes // 4, device=dev)
        audio = R.make_audio(B2, T, 40 + d).cuda()
        fmaps = [torch.empty(B2, plan.C[i + 1], plan.H[i + 1], p, device=dev) for i in range(N)]
        g = [torch.randn_like(f) for f in fmaps]
        wsp, arena, d_audio = torch.empty(plan.workspace_bytes // 4, device=dev), torch.empty(plan.grad_floats, device=dev), torch.empty_like(audio)
        fa = L.HifiganMpdFwdArgs(p, B2, T, L.ptr(packed), L.ptr(audio), (C.c_void_p * N)(*[L.ptr(f) for f in fmaps]))

        def bwd_args(grads, dx):
            return L.HifiganMpdBwdArgs(p, B2, T, L.ptr(packed), L.ptr(packed_bwd), L.ptr(audio), (C.c_void_p * N)(*[L.ptr(f) for f in fmaps]),
                                       (C.c_void_p * N)(*[L.ptr(x) for x in g]), L.ptr(wsp), L.ptr(grads), L.ptr(dx))
        b_x, b_all = bwd_args(None, d_audio), bwd_args(arena, d_audio)
        ms = {"pack (forward)": event_ms(lambda: L.check(lib.t2_hifigan_mpd_pack(wp, bp, L.ptr(packed), L.stream())), a.warmup, a.reps),
              "pack (data gradient)": event_ms(lambda: L.check(lib.t2_hifigan_mpd_pack_backward(wp, L.ptr(packed_bwd), L.stream())), a.warmup, a.reps),
              "forward": event_ms(lambda: L.check(lib.t2_hifigan_mpd_forward(C.byref(fa), L.stream())), a.warmup, a.reps),
              "data gradients": event_ms(lambda: L.check(lib.t2_hifigan_mpd_backward(C.byref(b_x), L.stream())), a.warmup, a.reps)}
        ms["weight gradients + reduces (difference)"] = event_ms(lambda: L.check(lib.t2_hifigan_mpd_backward(C.byref(b_all), L.stream())), a.warmup, a.reps) - ms["data gradients"]
        fl = forward_flops(plan)
        print(f"  period {p}: rows {list(plan.H)}, 128-column tiles per item {list(plan.tiles)}, weight-gradient runs {list(plan.splits)}, "
              f"backward scratch {plan.workspace_bytes / 2 ** 20:.1f} MiB")
        for k, v in ms.items():
            line(k, v, 0.0 if k.startswith("pack") else fl)
            t = tot.setdefault(k, [0.0, 0.0])
            t[0] += v; t[1] += 0.0 if k.startswith("pack") else fl
        del packed, packed_bwd, fmaps, g, wsp, arena
        torch.cuda.empty_cache()
    print("  all five periods:")
    for k, (v, fl) in tot.items():
        line(k, v, fl)


B, T = (int(v) for v in a.shape.split("x"))
mpd = MultiPeriodDiscriminator()
mpd.load_state_dict(R.make_state_dict(1))
mpd = mpd.cuda()
y, y_hat = R.make_audio(B, T, 2).cuda(), R.make_audio(B, T, 3).cuda()
fl = sum(forward_flops(L.hifigan_mpd_plan(p, 2 * B, T)) for p in R.PERIODS)


def set_grad(on):
    for p in mpd.parameters():
        p.requires_grad_(on)


def d_step():
    mpd.zero_grad(set_to_none=True)
    discriminator_loss(*mpd(y, y_hat.detach())[:2])[0].backward()


def g_step():
    mpd.zero_grad(set_to_none=True)
    h = y_hat.detach().requires_grad_(True)
    _, y_d_gs, fmap_rs, fmap_gs = mpd(y, h)
    (feature_loss(fmap_rs, fmap_gs) + generator_loss(y_d_gs)[0]).backward()


def infer():
    with torch.no_grad():
        mpd(y, y_hat)


print(f"multi-period discriminator, B = {B} x {T} samples (2B = {2 * B} items per period), fp32, weight-normed; {a.warmup} warm-up + {a.reps} timed calls per figure")
print("  the steps (FLOPs: forward x 1, x 3 with every gradient, x 2 with the data gradients only):")
line("forward alone (no_grad)", event_ms(infer, a.warmup, a.reps), fl)
line("discriminator step (all parameter gradients)", event_ms(d_step, a.warmup, a.reps), 3 * fl)
line("generator step as the reference runs it (parameters too)", event_ms(g_step, a.warmup, a.reps), 3 * fl)
set_grad(False)
line("generator step, gradient to y_hat only", event_ms(g_step, a.warmup, a.reps), 2 * fl)
set_grad(True)
if not a.no_kernels:
    kernel_report(mpd, 2 * B, T)
