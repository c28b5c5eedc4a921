"""Dev tool: times of WaveGlow inference (tacotron2_subword_amd/waveglow) on the GPU, the published shape (80 mel channels,
12 flows, n_group 8, an early output of 2 channels every 4 flows, WN of 8 layers x 256 channels) with seeded weights, B = 1:

  python scripts/time_waveglow.py [--frames 775] [--channels 256] [--warmup 2] [--reps 5]

Per T (775 frames = 9.0 s at 22 050 Hz): ms per call from HIP events around --reps calls of ``infer`` after --warmup calls
(the module call: the noise draws, the workspace allocation and the plan query are inside, the one-off weight packing is
not), the real-time factor (audio seconds per second of compute), and the achieved fraction of the 157.3 TFLOP/s fp32-matrix
peak from this script's own count of the useful FLOPs (2 * rows * K per column of every GEMM; the padding of K up to
16-channel chunks is not counted as work).  Then one more call with every launch bracketed by events
(``infer_debug(kernel_times=True)``): the time per kind of kernel, and the gated conv's own share of the peak.
The script calls no torch convolution, on any device, and compares with no torch statement of the model.  A run without a
GPU fails."""
import argparse, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, nargs="+", default=[775])
ap.add_argument("--channels", type=int, default=256)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import waveglow_ref as R
from tacotron2_subword_amd.waveglow.glow import WaveGlow

assert torch.cuda.is_available(), "time_waveglow.py measures on the GPU: none found"
PEAK = 157.3e12
SR = 22050
CFG = dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2, WN_config=dict(n_layers=8, n_channels=a.channels, kernel_size=3))


def flops(cfg, T):
    """Useful FLOPs per kind of kernel for one item of T frames."""
    nc, nl, G, n_mel = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"], cfg["n_group"], cfg["n_mel_channels"]
    L = T * 256 // G
    out = dict(upsample=2.0 * n_mel * n_mel * 1024 * T, start=0.0, gated_conv=0.0, res_skip=0.0, couple=0.0)
    for ch in R.flow_channels(cfg):
        out["start"] += 2.0 * nc * (ch // 2) * L
        out["gated_conv"] += nl * 2.0 * (2 * nc) * (3 * nc + n_mel * G) * L
        out["res_skip"] += ((nl - 1) * 2.0 * (2 * nc) * nc + 2.0 * nc * nc) * L
        out["couple"] += (2.0 * ch * nc + 2.0 * ch * ch) * L
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
model.load_state_dict(R.make_state_dict(CFG, 1))
model = model.cuda().eval()
model.repack()
print(f"{a.channels} channels, 12 flows, 8 layers, B = 1, fp32, sigma = 0.666; {a.warmup} warm-up + {a.reps} timed calls per figure", flush=True)
for T in a.frames:
    mel = R.make_mel(1, T, 3).cuda()
    with torch.no_grad():
        ms = event_ms(lambda: model.infer(mel, sigma=0.666), a.warmup, a.reps)
        audio, info = model.infer_debug(mel, sigma=0.666, kernel_times=True)
    assert bool(torch.isfinite(audio).all())
    n, fl = T * 256, flops(CFG, T)
    total = sum(fl.values())
    print(f"T={T:5d} ({n / SR:5.2f} s)  {ms:9.3f} ms/call  real-time factor {n / SR / (ms * 1e-3):7.1f}  {total / 1e12:6.3f} TFLOP "
          f"({total / n / 1e6:5.2f} MFLOP per sample)  {total / (ms * 1e-3) / 1e12:6.2f} TFLOP/s = {100 * total / (ms * 1e-3) / PEAK:5.2f} % of fp32-matrix peak", flush=True)
    kms = info["kernel_ms"]
    print(f"  per kind of kernel (one call, every launch between two events; sum {sum(kms.values()):9.3f} ms):", flush=True)
    for kind, t in kms.items():
        rate = fl[kind] / (t * 1e-3) / 1e12 if t > 0 else 0.0
        print(f"    {kind:10s} {t:9.3f} ms  {fl[kind] / 1e9:9.1f} GFLOP  {rate:6.2f} TFLOP/s = {100 * rate * 1e12 / PEAK:5.2f} % of fp32-matrix peak", flush=True)
