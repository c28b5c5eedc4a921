"""Dev tool: times of the HiFi-GAN generator (tacotron2_subword_amd/hifigan_infer) on the GPU, config_v1 shape (512 initial
channels, rates 8-8-2-2, ResBlock1) with seeded weights, B = 1, T in {100, 400, 800} frames:

  python scripts/time_hifigan.py [--frames 100 400 800] [--warmup 3] [--reps 10] [--no-torch]
  python scripts/time_hifigan.py --ragged [--warmup 3] [--reps 10]

Per T: ms per call from HIP events around --reps calls after --warmup calls (the module call: workspace allocation and
the plan query are inside, the one-off weight packing is not), samples/s, the real-time factor at 22 050 Hz (audio seconds
per second of compute), and the achieved fraction of the 157.3 TFLOP/s fp32-matrix peak from this script's own count of
the useful FLOPs (2 * Cin * Cout * k per output position of a Conv1d, per input position of a ConvTranspose1d; the padding
of narrow layers up to the 32-row MFMA tile is not counted as work).
Per-stage split at the largest T: the generator is also built with only its first n upsampling stages (n = 1..4, conv_post
on that stage's channels) and timed the same way; stage n's share is time(n) - time(n-1), so stage 1 carries conv_pre and
every figure a small conv_post of its own.  That is a difference of module calls, not a kernel trace.
Unless --no-torch: the tests' functional restatement (tests/hifigan_ref.py) on torch's own conv1d / conv_transpose1d on
the same GPU in fp32, timed the same way, as a comparison; if those ops do not run here that is reported and skipped.
--ragged instead times a padded batch of utterances of different lengths: B = 16, frame counts drawn seeded and uniformly from
200..800.  It prints ms per call of the ragged call (lengths as an int32 device tensor), of the padded call (lengths=None at
T_max, what a caller had to run before, with wrong last frames) and the sum of the sixteen B = 1 calls on each item's own
frames, and the tile ratio sum(ceil(len_b * rate / 128)) / (B * ceil(T_max * rate / 128)) summed over the conv launches of all
stages, weighted by each launch's FLOPs per tile: the share of the padded call's matrix work the ragged call does, counted
from shapes, which ragged / padded time should approach.
A run without a GPU fails."""
import argparse, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, nargs="+", default=[100, 400, 800])
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--ragged", action="store_true")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import hifigan_ref as R
from tacotron2_subword_amd.hifigan_infer import Generator

assert torch.cuda.is_available(), "time_hifigan.py measures on the GPU: none found"
PEAK = 157.3e12
SR = 22050
V1 = R.H(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
         resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]])


def flops(h, T):
    total = 0.0
    rate = 1
    stage_len = [T]
    for u in h["upsample_rates"]:
        rate *= u
        stage_len.append(T * rate)
    for name, kind, cin, cout, k, _ in R.layer_names(h):
        if name == "conv_pre":
            n = T
        elif kind == "convT":
            n = stage_len[int(name.split(".")[1])]                 # per input position
        elif name == "conv_post":
            n = stage_len[-1]
        else:
            n = stage_len[int(name.split(".")[1]) // len(h["resblock_kernel_sizes"]) + 1]
        total += 2.0 * cin * cout * k * n
    return total


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


def build(h, seed=1):
    sd = R.calibrate(R.make_state_dict(h, seed), h, R.make_mel(1, 8, 2))
    gen = Generator(h)
    gen.load_state_dict(sd)
    gen = gen.cuda().eval()
    gen.remove_weight_norm()
    return gen, {k: v.cuda() for k, v in R.fold(sd).items()}


def tile_ratio(h, lens, T_max, tile=128):
    """Time tiles the ragged call runs over those of the padded call, each conv launch weighted by its FLOPs per tile."""
    rate, stage_rate = 1, [1]
    for u in h["upsample_rates"]:
        rate *= u
        stage_rate.append(rate)
    nk = len(h["resblock_kernel_sizes"])
    run = full = 0.0
    for name, kind, cin, cout, k, _ in R.layer_names(h):
        if name == "conv_post":
            continue                                               # not a tiled GEMM, and 1 output channel: no weight
        st = 0 if name == "conv_pre" else int(name.split(".")[1]) if kind == "convT" else int(name.split(".")[1]) // nk + 1
        w = float(cin) * cout * k
        tiles = lambda T: -(-T * stage_rate[st] // tile)
        run += w * sum(tiles(n) for n in lens)
        full += w * len(lens) * tiles(T_max)
    return run / full


def ragged_report():
    B = 16
    lens = torch.randint(200, 801, (B,), generator=torch.Generator().manual_seed(16)).tolist()
    T_max = max(lens)
    mel = R.make_mel(B, T_max, 3).cuda()
    dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    singles = [mel[b:b + 1, :, :n].contiguous() for b, n in enumerate(lens)]
    with torch.no_grad():
        ms_r = event_ms(lambda: gen(mel, lengths=dl), a.warmup, a.reps)
        ms_p = event_ms(lambda: gen(mel), a.warmup, a.reps)
        ms_1 = event_ms(lambda: [gen(m) for m in singles], a.warmup, a.reps)
        audio, n = gen(mel, lengths=dl)
        same = all(torch.equal(audio[b:b + 1, :, :lens[b] * 256], gen(singles[b])) for b in range(B))
    ratio = tile_ratio(V1, lens, T_max)
    print(f"config_v1 shape, B = {B}, frame counts {lens} (sum {sum(lens)}, T_max {T_max}), fp32; {a.warmup} warm-up + {a.reps} timed calls per figure")
    print(f"ragged call (lengths on the device)   {ms_r:9.3f} ms/call")
    print(f"padded call (lengths=None at T_max)    {ms_p:9.3f} ms/call")
    print(f"sum of the {B} B = 1 calls             {ms_1:9.3f} ms")
    print(f"ragged / padded = {ms_r / ms_p:.3f}; tile ratio counted from shapes = {ratio:.3f}; frame ratio sum(len) / (B * T_max) = {sum(lens) / (B * T_max):.3f}")
    print(f"ragged / sum of single calls = {ms_r / ms_1:.3f}; every item bit-equal to its single call: {same}", flush=True)


gen, folded = build(V1)
if a.ragged:
    ragged_report()
    sys.exit(0)
print(f"config_v1 shape, B = 1, fp32; {a.warmup} warm-up + {a.reps} timed calls per figure", flush=True)
for T in a.frames:
    mel = R.make_mel(1, T, 3).cuda()
    with torch.no_grad():
        ms = event_ms(lambda: gen(mel), a.warmup, a.reps)
    n, fl = T * 256, flops(V1, T)
    line = (f"T={T:4d}  {ms:9.3f} ms/call  {n / ms * 1e3:12.0f} samples/s  real-time factor {n / SR / (ms * 1e-3):8.1f}  "
            f"{fl / 1e9:8.1f} GFLOP  {fl / (ms * 1e-3) / 1e12:6.2f} TFLOP/s = {100 * fl / (ms * 1e-3) / PEAK:5.2f} % of fp32-matrix peak")
    if not a.no_torch:
        try:
            with torch.no_grad():
                tms = event_ms(lambda: R.generator_forward(folded, V1, mel, torch.float32), a.warmup, a.reps)
                err = float((R.generator_forward(folded, V1, mel, torch.float32)[0] - gen(mel)).abs().max())
            line += f"  | torch conv1d/conv_transpose1d restatement {tms:9.3f} ms (max-abs difference {err:.2e})"
        except RuntimeError as e:
            line += f"  | torch's conv ops do not run here: {str(e).splitlines()[0][:80]}"
    print(line, flush=True)

T = max(a.frames)
mel = R.make_mel(1, T, 3).cuda()
prev, prev_fl = 0.0, 0.0
print(f"per-stage split at T={T} (time of the generator cut after stage n, minus the one cut after stage n-1):", flush=True)
for n in range(1, 5):
    h = R.H(V1, upsample_rates=V1.upsample_rates[:n], upsample_kernel_sizes=V1.upsample_kernel_sizes[:n])
    try:
        g_n, _ = build(h)
    except RuntimeError as e:                                  # e.g. a cut the channel rule refuses
        print(f"  stage {n}: not measured ({e})", flush=True)
        continue
    with torch.no_grad():
        ms = event_ms(lambda: g_n(mel), a.warmup, a.reps)
    fl = flops(h, T)
    ch = 512 >> n
    print(f"  stage {n} ({ch:3d} channels, {T * int(torch.tensor(h.upsample_rates).prod()):7d} samples): cumulative {ms:9.3f} ms, stage {ms - prev:9.3f} ms, "
          f"{(fl - prev_fl) / 1e9:8.1f} GFLOP, {(fl - prev_fl) / ((ms - prev) * 1e-3) / 1e12:6.2f} TFLOP/s", flush=True)
    prev, prev_fl = ms, fl
