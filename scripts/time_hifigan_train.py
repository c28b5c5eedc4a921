"""Dev tool: times of one HiFi-GAN generator training iteration on the GPU (``Generator.trainable()``, csrc/vocoder_bwd.hip),
config_v1 with seeded weight-normed weights, at the published training shape B = 16, 32 frames (segment 8192) and for one
400-frame item:

  python scripts/time_hifigan_train.py [--shapes 16x32 1x400] [--warmup 3] [--reps 10] [--no-torch] [--no-kernels]

Per shape, from HIP events around --reps calls after --warmup calls:
  the iteration   forward (kept activations), 45 * L1(mel(y_hat), mel(y)), backward, FusedAdam step -- and its parts: the
                  inference forward under no_grad (cached packs), the training forward alone (it folds the weight norm and packs
                  the forward and data-gradient weights on every call, as a training loop needs: that work is inside every figure
                  of the training path), forward + loss + backward, the optimizer step;
                  the tape's size from the plan; forward + backward FLOPs (3 x the forward's useful FLOPs, time_hifigan.py's
                  count) as a share of the 157.3 TFLOP/s fp32-matrix peak;
  per kernel      unless --no-kernels: every launch of the backward's list through its unit entry point on random data of
                  the layer's shape (the data gradient's entry point packs its weights first, which the generator does once per
                  training forward for all layers: the figure includes that pack), summed per kind, with the kind's useful FLOPs and share of peak;
  torch           unless --no-torch: the same iteration through the tests' functional restatement on torch's conv1d /
                  conv_transpose1d with autograd and torch.optim.Adam on the same GPU, if those ops run here.
A run without a GPU fails."""
import argparse, ctypes as C, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["16x32", "1x400"])
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--no-kernels", action="store_true")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import torch.nn.functional as F
import hifigan_ref as R
from tacotron2_subword_amd import _lib as L
from tacotron2_subword_amd.hifigan_infer import Generator
from tacotron2_subword_amd.optim import FusedAdam
from tacotron2_subword_amd.utils import mel_spectrogram_from_audio

assert torch.cuda.is_available(), "time_hifigan_train.py measures on the GPU: none found"
PEAK = 157.3e12
V1 = R.load_config(os.path.join(ROOT, "tests", "golden", "hifigan_config_v1.json"))


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


def layer_lengths(h, T):
    """{layer name: its input length}."""
    rate, stage_len = 1, [T]
    for u in h["upsample_rates"]:
        rate *= u
        stage_len.append(T * rate)
    nk, out = len(h["resblock_kernel_sizes"]), {}
    for name, kind, *_ in R.layer_names(h):
        if name == "conv_pre":
            out[name] = T
        elif kind == "convT":
            out[name] = stage_len[int(name.split(".")[1])]
        elif name == "conv_post":
            out[name] = stage_len[-1]
        else:
            out[name] = stage_len[int(name.split(".")[1]) // nk + 1]
    return out


def forward_flops(h, B, T):
    n = layer_lengths(h, T)
    return sum(2.0 * cin * cout * k * n[name] * B for name, _, cin, cout, k, _ in R.layer_names(h))


def kernel_report(h, B, T):
    lens, lib = layer_lengths(h, T), L.lib()
    kinds = {}
    for name, kind, cin, cout, k, du in R.layer_names(h):
        n, u, d = lens[name], (du if kind == "convT" else 0), (1 if kind == "convT" else du)
        fl = 2.0 * cin * cout * k * n * B
        if name == "conv_post":
            x, w = torch.randn(B, cin, n, device="cuda"), torch.randn(cin, 7, device="cuda")
            audio, da = torch.rand(B, n, device="cuda") - 0.5, torch.randn(B, n, device="cuda")
            dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty(1, device="cuda")
            part = torch.empty(lib.t2_vocoder_post_part_doubles(B, cin, n), device="cuda", dtype=torch.float64)
            args = L.VocoderPostBwdArgs(B, cin, n, L.ptr(x), L.ptr(w), L.ptr(audio), L.ptr(da), L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(part), 1.0)
            ms = event_ms(lambda: L.check(lib.t2_vocoder_post_backward(C.byref(args), L.stream())), a.warmup, a.reps)
            t = kinds.setdefault("conv_post backward", [0.0, 0.0])
            t[0] += ms; t[1] += 2 * fl
            continue
        x, dy = torch.randn(B, cin, n, device="cuda"), torch.randn(B, cout, n * max(u, 1), device="cuda")
        w = torch.randn((cin, cout, k) if u else (cout, cin, k), device="cuda")
        dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty(cout, device="cuda")
        packed = torch.empty(lib.t2_vocoder_dgrad_packed_floats(cin, cout, k, u), device="cuda")
        part = torch.empty(lib.t2_vocoder_wgrad_part_floats(B, cin, cout, n, k, d, u), device="cuda")
        da = L.VocoderDgradArgs(B, cin, cout, n, k, d, u, L.ptr(dy), L.ptr(w), L.ptr(x), None, L.ptr(dx), L.ptr(packed), 0.1, 0, 1.0)
        wa = L.VocoderWgradArgs(B, cin, cout, n, k, d, u, L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(db), L.ptr(part), 0.1)
        fn = lib.t2_vocoder_conv_transpose1d_dgrad if u else lib.t2_vocoder_conv1d_dgrad
        tag = "ConvTranspose1d" if u else "Conv1d"
        for label, call in ((f"{tag} data gradient (+ pack)", lambda: L.check(fn(C.byref(da), L.stream()))),
                            (f"{tag} weight gradient + reduce", lambda: L.check(lib.t2_vocoder_wgrad(C.byref(wa), L.stream())))):
            ms = event_ms(call, a.warmup, a.reps)
            t = kinds.setdefault(label, [0.0, 0.0])
            t[0] += ms; t[1] += fl
    total = sum(v[0] for v in kinds.values())
    print(f"  per kernel kind, every launch of the backward's list on its own (sum {total:9.3f} ms):")
    for label, (ms, fl) in kinds.items():
        print(f"    {label:40s} {ms:9.3f} ms  {100 * ms / total:5.1f} %  {fl / 1e9:9.1f} GFLOP  {fl / (ms * 1e-3) / 1e12:6.2f} TFLOP/s = "
              f"{100 * fl / (ms * 1e-3) / PEAK:5.2f} % of fp32-matrix peak", flush=True)


def torch_iteration(sd, h, mel, target):
    """The same iteration on torch's ops: weight norm, convs and autograd are torch's, the log-mel is this project's."""
    p = {k: v.clone().cuda().requires_grad_(True) for k, v in sd.items()}
    specs = {s[0]: s for s in R.layer_names(h)}
    opt = torch.optim.Adam(list(p.values()), lr=2e-4, betas=(0.8, 0.99))

    def layer(name, x):
        v, g = p[name + ".weight_v"], p[name + ".weight_g"]
        return R._apply(specs[name], x, torch._weight_norm(v, g, 0), p[name + ".bias"])

    def it():
        opt.zero_grad(set_to_none=True)
        y_hat, _ = R._walk(h, mel, layer)
        (F.l1_loss(mel_spectrogram_from_audio(y_hat.squeeze(1), differentiable=True), target) * 45).backward()
        opt.step()
    return it


sd = R.calibrate(R.make_state_dict(V1, 1), V1, R.make_mel(1, 8, 2))
for shape in a.shapes:
    B, T = (int(v) for v in shape.split("x"))
    gen = Generator(V1)
    gen.load_state_dict(sd)
    gen = gen.cuda().trainable()
    opt = FusedAdam(gen.parameters(), lr=2e-4, betas=(0.8, 0.99))
    mel = R.make_mel(B, T, 3).cuda()
    with torch.no_grad():
        target = mel_spectrogram_from_audio(torch.tanh(torch.randn(B, T * 256, device="cuda")) * 0.5)
    plan = L.hifigan_train_plan(gen._cfg, B, T)

    def fwd_bwd():
        gen.zero_grad(set_to_none=True)
        y_hat = gen(mel)
        (F.l1_loss(mel_spectrogram_from_audio(y_hat.squeeze(1), differentiable=True), target) * 45).backward()

    def iteration():
        fwd_bwd()
        opt.step()

    def infer():
        with torch.no_grad():
            gen(mel)
    ms_it = event_ms(iteration, a.warmup, a.reps)
    ms_fb = event_ms(fwd_bwd, a.warmup, a.reps)
    ms_f = event_ms(lambda: gen(mel), a.warmup, a.reps)
    ms_i = event_ms(infer, a.warmup, a.reps)
    fwd_bwd()
    ms_o = event_ms(opt.step, a.warmup, a.reps)
    fl = 3 * forward_flops(V1, B, T)
    print(f"config_v1, B = {B}, T = {T} frames ({T * 256} samples), fp32, weight-normed; {a.warmup} warm-up + {a.reps} timed calls per figure; "
          f"tape {plan.tape_bytes / 2 ** 20:.1f} MiB, backward scratch {plan.workspace_bytes / 2 ** 20:.1f} MiB")
    print(f"  iteration (forward, mel-L1, backward, FusedAdam) {ms_it:9.3f} ms   {fl / 1e9:8.1f} GFLOP forward + backward  "
          f"{fl / (ms_it * 1e-3) / 1e12:6.2f} TFLOP/s = {100 * fl / (ms_it * 1e-3) / PEAK:5.2f} % of fp32-matrix peak")
    print(f"  inference forward (no_grad) {ms_i:9.3f} ms | training forward {ms_f:9.3f} ms | forward + loss + backward {ms_fb:9.3f} ms "
          f"= {ms_fb / ms_i:.2f} x inference | FusedAdam step {ms_o:9.3f} ms", flush=True)
    if not a.no_kernels:
        kernel_report(V1, B, T)
    if not a.no_torch:
        try:
            tms = event_ms(torch_iteration(sd, V1, mel, target), a.warmup, a.reps)
            print(f"  the same iteration on torch's conv1d / conv_transpose1d, autograd and Adam {tms:9.3f} ms = {tms / ms_it:.2f} x this project's", flush=True)
        except RuntimeError as e:
            print(f"  torch's conv ops do not run here: {str(e).splitlines()[0][:100]}", flush=True)
    del gen, opt
    torch.cuda.empty_cache()
