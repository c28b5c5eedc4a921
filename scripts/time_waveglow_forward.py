"""Dev tool: times of WaveGlow's forward direction (``WaveGlow.nll`` and ``WaveGlow.analyze``: audio -> z and the negative
log-likelihood) on the GPU next to ``WaveGlow.infer`` at the same (B, T), the published shape (80 mel channels, 12 flows,
n_group 8, an early output of 2 channels every 4 flows, WN of 8 layers x 256 channels) with seeded weights:

  python scripts/time_waveglow_forward.py [--channels 256] [--warmup 2] [--reps 5] [--repeats 3]

Two shapes: the reference's training shape (waveglow/config.json: batch 12, segments of 16000 samples, 63 frames) and one 9 s
utterance (B = 1, T = 775, N = T * 256).  Per shape and per repeat, ``nll``, ``analyze`` and ``infer`` are timed one after the
other in the same process (HIP events around --reps calls after --warmup calls; the module call: the workspace allocation and
the plan query are inside, the one-off weight packing is not), so that a drift of the clocks meets all three alike.  Printed:
ms per call (the median of the repeats, and their spread), audio samples per second, the ratio nll / infer, the share of the
157.3 TFLOP/s fp32-matrix peak from this script's own count of the useful FLOPs (2 * rows * K per column of every GEMM), and,
from one more call with every launch between two events, the time per kind of kernel.  A run without a GPU fails."""
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
from tacotron2_subword_amd.waveglow.glow import WaveGlow

if not torch.cuda.is_available():
    raise SystemExit("time_waveglow_forward.py measures on the GPU: none found")
PEAK = 157.3e12
CFG = dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2, WN_config=dict(n_layers=8, n_channels=a.channels, kernel_size=3))
SHAPES = [("training shape", 12, 63, 16000), ("one 9 s utterance", 1, 775, 775 * 256)]


def flops(cfg, B, T, L):
    """Useful FLOPs per kind of kernel of the forward direction for B items of L columns."""
    nc, nl, G, n_mel = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"], cfg["n_group"], cfg["n_mel_channels"]
    out = dict(upsample=2.0 * n_mel * n_mel * 4 * L * G * B, start=0.0, gated_conv=0.0, res_skip=0.0, head=2.0 * G * G * L * B, tail=0.0, sums=0.0)
    for ch in R.flow_channels(cfg):
        out["start"] += 2.0 * nc * (ch // 2) * L * B
        out["gated_conv"] += nl * 2.0 * (2 * nc) * (3 * nc + n_mel * G) * L * B
        out["res_skip"] += ((nl - 1) * 2.0 * (2 * nc) * nc + 2.0 * nc * nc) * L * B
        out["tail"] += (2.0 * ch * nc + 2.0 * ch * ch) * L * B
    return out


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
model = model.cuda().eval()
print(f"{a.channels} channels, 12 flows, 8 layers, fp32; {a.repeats} repeats of {a.warmup} warm-up + {a.reps} timed calls per figure", flush=True)
for name, B, T, N in SHAPES:
    mel = R.make_mel(B, T, 3).cuda()
    audio = (torch.randn(B, N, generator=torch.Generator().manual_seed(4)) * 0.3).cuda()
    calls = dict(nll=lambda: model.nll(mel, audio, sigma=1.0), analyze=lambda: model.analyze((mel, audio)), infer=lambda: model.infer(mel, sigma=0.666))
    ms = {k: [] for k in calls}
    with torch.no_grad():
        for fn in calls.values():                         # the one-off packing of both buffers stays outside
            fn()
        for _ in range(a.repeats):
            for k, fn in calls.items():                   # alternating: one figure of each per repeat
                ms[k].append(event_ms(fn, a.warmup, a.reps))
        z, log_s, logdet, info = model.analyze_debug((mel, audio), kernel_times=True)
        _, infer_info = model.infer_debug(mel, sigma=0.666, kernel_times=True)
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(info["loss"]))
    L = N // CFG["n_group"]
    fl = flops(CFG, B, T, L)
    total = sum(fl.values())
    print(f"{name}: B={B} T={T} N={N} (L={L}), nll = {float(info['loss']):.6f}", flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        samples = B * (N if k != "infer" else T * 256)
        print(f"  {k:8s} {med[k]:9.3f} ms/call (repeats {' '.join(f'{x:.3f}' for x in v)}; spread {100 * (max(v) - min(v)) / med[k]:4.1f} %)  "
              f"{samples / (med[k] * 1e-3) / 1e6:8.2f} M samples/s" +
              (f"  {total / 1e12:6.3f} TFLOP  {total / (med[k] * 1e-3) / 1e12:6.2f} TFLOP/s = {100 * total / (med[k] * 1e-3) / PEAK:5.2f} % of fp32-matrix peak" if k != "infer" else ""),
              flush=True)
    print(f"  nll / infer = {med['nll'] / med['infer']:.3f}   analyze / infer = {med['analyze'] / med['infer']:.3f}"
          f"   (infer makes {T * 256} samples per item, the forward direction reads {N})", flush=True)
    kms = info["kernel_ms"]
    print(f"  forward direction per kind of kernel (one call, every launch between two events; sum {sum(kms.values()):9.3f} ms):", flush=True)
    for kind, t in kms.items():
        rate = fl[kind] / (t * 1e-3) / 1e12 if t > 0 else 0.0
        print(f"    {kind:10s} {t:9.3f} ms  {fl[kind] / 1e9:9.1f} GFLOP  {rate:6.2f} TFLOP/s = {100 * rate * 1e12 / PEAK:5.2f} % of fp32-matrix peak", flush=True)
    ims = infer_info["kernel_ms"]
    print(f"  infer per kind of kernel (sum {sum(ims.values()):9.3f} ms): " + "  ".join(f"{k} {t:.3f}" for k, t in ims.items()), flush=True)
