"""Dev tool: times of one WaveGlow training iteration on the GPU -- ``model((mel, audio))`` of a ``trainable()`` model, then
``WaveGlowLoss`` and ``backward()`` -- next to ``WaveGlow.nll`` at the same shape, the published model (80 mel channels, 12 flows,
n_group 8, an early output of 2 channels every 4 flows, WN of 8 layers x 256 channels) with seeded weights:

  python scripts/time_waveglow_train.py [--channels 256] [--warmup 2] [--reps 5] [--repeats 3]

Two shapes: the reference's training shape (waveglow/config.json: batch 12, segments of 16000 samples, 63 frames) and B = 1 with
64000 samples (250 frames).  Per shape and per repeat, ``nll`` under no_grad, the trainable forward alone (grad mode on: it keeps
what the backward reads) and forward + loss + backward are timed one after the other in the same process (HIP events around
--reps calls after --warmup calls; allocations, the device fold and the per-step packing are inside), so that a drift of the
clocks meets all three alike.  Printed: ms per call (the median of the repeats, and their spread), the ratios iteration / nll
(the FLOP ratio is 3.0) and trainable forward / nll (1.0 plus the stores of x_i, tanh and sigmoid), and, from one more iteration
with every launch between two events, the time per kind of kernel with its share of the 157.3 TFLOP/s fp32-matrix peak from this
script's own count of the useful FLOPs.  A run without a GPU fails."""
import argparse, os, statistics, sys
ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=256)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import waveglow_fwd_ref as FR
import waveglow_ref as R
from tacotron2_subword_amd.waveglow.glow import WaveGlow, WaveGlowLoss

if not torch.cuda.is_available():
    raise SystemExit("time_waveglow_train.py measures on the GPU: none found")
PEAK = 157.3e12
CFG = dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2, WN_config=dict(n_layers=8, n_channels=a.channels, kernel_size=3))
SHAPES = [("training shape", 12, 63, 16000), ("one item of 64000 samples", 1, 250, 64000)]


def flops(cfg, B, T, L):
    """Useful FLOPs per kind of kernel, forward and backward, for B items of L columns."""
    nc, nl, G, n_mel = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"], cfg["n_group"], cfg["n_mel_channels"]
    n_cond, cols = n_mel * G, L * B
    fwd = dict(upsample=2.0 * n_mel * n_mel * 4 * L * G * B, start=0.0, gated_conv=0.0, res_skip=0.0, head=2.0 * G * G * cols, tail=0.0, sums=0.0)
    bwd = dict(tail_backward=0.0, gate_backward=0.0, conv_backward=0.0, cond_backward=0.0, weight_grad=0.0, weight_grad_reduce=0.0, start_backward=0.0,
               upsample_backward=2.0 * n_mel * n_mel * 1024 * B * (T + 3))
    for ch in R.flow_channels(cfg):
        rs = (nl - 1) * 2.0 * (2 * nc) * nc + 2.0 * nc * nc
        fwd["start"] += 2.0 * nc * (ch // 2) * cols
        fwd["gated_conv"] += nl * 2.0 * (2 * nc) * (3 * nc + n_cond) * cols
        fwd["res_skip"] += rs * cols
        fwd["tail"] += (2.0 * ch * nc + 2.0 * ch * ch) * cols
        bwd["tail_backward"] += (3 * 2.0 * ch * nc + 4.0 * ch * ch) * cols                  # end again, d_out, dW_end; the mix and its gradient
        bwd["gate_backward"] += rs * cols
        bwd["conv_backward"] += nl * 2.0 * nc * (3 * 2 * nc) * cols
        bwd["cond_backward"] += nl * 2.0 * n_cond * (2 * nc) * cols
        bwd["weight_grad"] += (nl * 2.0 * (2 * nc) * (3 * nc + n_cond) + rs + 2.0 * nc * (ch // 2)) * cols
        bwd["start_backward"] += 2.0 * nc * (ch // 2) * cols
    return fwd, bwd


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


model = WaveGlow(**CFG)
model.load_state_dict(FR.skew_mixes(R.make_state_dict(CFG, 1), CFG, 2))
model = model.cuda().trainable()
criterion = WaveGlowLoss(1.0)
print(f"{a.channels} channels, 12 flows, 8 layers, fp32; {a.repeats} repeats of {a.warmup} warm-up + {a.reps} timed calls per figure", flush=True)
for name, B, T, N in SHAPES:
    mel = R.make_mel(B, T, 3).cuda()
    audio = (torch.randn(B, N, generator=torch.Generator().manual_seed(4)) * 0.3).cuda()

    def nll():
        with torch.no_grad():
            return model.nll(mel, audio, sigma=1.0)

    def forward():
        return model((mel, audio))

    def iteration():
        model.zero_grad(set_to_none=True)
        loss = criterion(model((mel, audio)))
        loss.backward()
        return loss

    calls = dict(nll=nll, forward=forward, iteration=iteration)
    ms = {k: [] for k in calls}
    nll()                                                     # the one-off packing of nll's buffer stays outside
    for _ in range(a.repeats):
        for k, fn in calls.items():                           # alternating: one figure of each per repeat
            ms[k].append(event_ms(fn, a.warmup, a.reps))
    times = {}
    model.zero_grad(set_to_none=True)
    loss = criterion(model._train_forward((mel, audio), kernel_times=times))
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    L = N // CFG["n_group"]
    fwd, bwd = flops(CFG, B, T, L)
    f_total, b_total = sum(fwd.values()), sum(bwd.values())
    print(f"{name}: B={B} T={T} N={N} (L={L}), loss = {float(loss.detach()):.6f} (nll {float(nll()):.6f}); forward {f_total / 1e12:.3f} TFLOP, backward "
          f"{b_total / 1e12:.3f} TFLOP, ratio (forward + backward) / forward = {(f_total + b_total) / f_total:.3f}; peak memory "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB", flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        total = f_total + (b_total if k == "iteration" else 0.0)
        print(f"  {k:9s} {med[k]:9.3f} ms/call (repeats {' '.join(f'{x:.3f}' for x in v)}; spread {100 * (max(v) - min(v)) / med[k]:4.1f} %)  "
              f"{total / (med[k] * 1e-3) / 1e12:6.2f} TFLOP/s = {100 * total / (med[k] * 1e-3) / PEAK:5.2f} % of fp32-matrix peak", flush=True)
    print(f"  iteration / nll = {med['iteration'] / med['nll']:.3f} (FLOP ratio 3.0)   trainable forward / nll = {med['forward'] / med['nll']:.3f}", flush=True)
    shares = {}
    for label, kms, fl in (("trainable forward", times["forward"], fwd), ("backward", times["backward"], bwd)):
        print(f"  {label} per kind of kernel (one call, every launch between two events; sum {sum(kms.values()):9.3f} ms):", flush=True)
        for kind, t in kms.items():
            rate = fl[kind] / (t * 1e-3) / 1e12 if t > 0 else 0.0
            shares[kind] = 100 * rate * 1e12 / PEAK
            print(f"    {kind:18s} {t:9.3f} ms  {fl[kind] / 1e9:9.1f} GFLOP  {rate:6.2f} TFLOP/s = {shares[kind]:5.2f} % of fp32-matrix peak", flush=True)
    print(f"  weight gradient / gated conv (share of the peak) = {shares['weight_grad'] / shares['gated_conv']:.3f}", flush=True)
