"""Dev tool: times of the silence trim (csrc/silence.hip, remove_silence.trim_silence) on the GPU at 22 050 Hz:

  python scripts/time_silence.py [--items 64] [--warmup 5] [--reps 50] [--rounds 3] [--no-hifigan]

--items utterances of 200..800 mel frames' worth of audio (256 samples per frame, seeded), loud in the middle, with random
silent heads and tails of up to a second, as one padded batch with lengths on the device.  Printed:
  - ms per trim_silence call from HIP events around --reps calls after --warmup calls, median of --rounds, for int16 in /
    int16 out and for fp32 in / fp32 out (the form the scoring loop uses: bias remover -> trim -> mel_spectrogram); output
    allocation and the plan query are inside.  With it the bytes the call reads and writes at most (every live sample twice,
    once per direction, and every output sample once) over that time;
  - the same trim by the CPU restatement of tests/silence_ref.py, item by item, from samples already on the host: wall time of
    one pass.  That is pure Python over audioop, not pydub, and it leaves out the two wav files per utterance the reference's
    loop also writes and reads;
  - whether every item of the batch has the restatement's bits;
  - unless --no-hifigan, for scale: ms per call of the ragged HiFi-GAN generator (config_v1 shape, seeded weights) on mels of
    the same frame counts, the call that would have produced this audio.
A run without a GPU fails."""
import argparse, os, statistics, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=64)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-hifigan", action="store_true")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import silence_ref as R
from tacotron2_subword_amd import remove_silence as RS

assert torch.cuda.is_available(), "time_silence.py measures on the GPU: none found"
SR, HOP = 22050, 256


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


def median_ms(fn, reps):
    runs = [event_ms(fn, min(a.warmup, reps), reps) for _ in range(a.rounds)]
    return statistics.median(runs), runs


rng = np.random.default_rng(64)
frames = rng.integers(200, 801, a.items).tolist()
items = []
for i, f in enumerate(frames):
    n = f * HOP
    head, tail = int(rng.integers(0, min(SR, n // 3))), int(rng.integers(0, min(SR, n // 3)))
    x = rng.integers(-20, 21, n).astype(np.int16)
    t = np.arange(n - head - tail)
    x[head:n - tail] = (8000 * np.sin(t * (0.03 + 0.001 * i)) + rng.integers(-800, 801, t.size)).astype(np.int16)
    items.append(x)
lens = [len(x) for x in items]
n_max = max(lens)
batch = np.zeros((a.items, n_max), dtype=np.int16)
for i, x in enumerate(items):
    batch[i, :lens[i]] = x
x16 = torch.from_numpy(batch).cuda()
x32 = x16.float()
dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
live = sum(lens)
print(f"{a.items} items of {min(frames)}..{max(frames)} frames = {min(lens)}..{n_max} samples ({live} live of {a.items * n_max} padded) at {SR} Hz, "
      f"threshold -50 dBFS, 10 ms chunks; {a.warmup} warm-up + {a.reps} timed calls per figure, median of {a.rounds} rounds", flush=True)

with torch.no_grad():
    out16 = RS.trim_silence(x16, dl)
    W = out16[0].shape[1]
    for name, fn, bin_, bout in (("int16 in, int16 out", lambda: RS.trim_silence(x16, dl), 2, 2),
                                 ("fp32 in, fp32 out", lambda: RS.trim_silence(x32, dl, out_dtype=torch.float32), 4, 4)):
        ms, runs = median_ms(fn, a.reps)
        moved = 3 * live * bin_ + a.items * W * bout      # at most: two scans and the copy read, every output sample written
        print(f"  trim_silence, {name:20s} {ms:8.4f} ms/call   (rounds: {', '.join(f'{v:.4f}' for v in runs)})   "
              f"at most {moved / 1e6:.1f} MB moved = {moved / ms / 1e6:.1f} GB/s", flush=True)

    t0 = time.perf_counter()
    refs = [R.trim(x) for x in items]
    cpu_ms = (time.perf_counter() - t0) * 1e3
    print(f"  CPU restatement, item by item         {cpu_ms:8.1f} ms for the {a.items} items (one pass, samples already on the host, no wav files)", flush=True)
    out, new, start, end = (t.cpu().numpy() for t in out16)
    same = all(w is not None and int(new[i]) == len(w) and (int(start[i]), int(end[i])) == (s, e) and np.array_equal(out[i, :len(w)], w)
               and not out[i, len(w):].any() for i, (w, s, e) in enumerate(refs))
    print(f"  every item bit-equal to the restatement: {same}; start_silence / limit_silence / dropped = {RS.silence_stats(out16[2])}", flush=True)

    if not a.no_hifigan:
        import hifigan_ref as H
        from tacotron2_subword_amd.hifigan_infer import Generator
        V1 = H.H(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
                 resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]])
        sd = H.calibrate(H.make_state_dict(V1, 1), V1, H.make_mel(1, 8, 2))
        gen = Generator(V1)
        gen.load_state_dict(sd)
        gen = gen.cuda().eval()
        gen.remove_weight_norm()
        mel = H.make_mel(a.items, max(frames), 3).cuda()
        fl = torch.tensor(frames, dtype=torch.int32, device="cuda")
        ms = event_ms(lambda: gen(mel, lengths=fl), 1, 3)
        print(f"  for scale: ragged HiFi-GAN (config_v1) on the same frame counts  {ms:8.2f} ms/call (1 warm-up + 3 timed calls)", flush=True)
