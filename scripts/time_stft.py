"""Dev tool: times of the STFT synthesis side (csrc/stft.hip) on the GPU for a 9 s signal at 22 050 Hz, B = 1, with
filter_length / hop_length / win_length = 1024 / 256 / 1024:

  python scripts/time_stft.py [--seconds 9] [--warmup 5] [--reps 50] [--gl-reps 5] [--no-statement]

ms per call from HIP events around --reps calls after --warmup calls (module calls: output allocation and the plan query are
inside, the one-off packing of the tables is not) of
  (a) hifiganBiasRemover.forward(audio, 0.9)   analysis kernel (re, im) + denoise-mode synthesis kernel: two launches
  (b) STFT.forward(audio)                      transform (framing copy, the general GEMM, torch element-wise ops) + polar synthesis kernel
  (c) griffin_lim(magnitudes, stft, 30)        31 polar syntheses and 30 transforms (--gl-reps calls)
and the two kernels by themselves (unit entry points), each against
  (d) the same formula written with torch ops on the same GPU in fp32 (the "matmul/fold statement"): reflect pad, unfold +
      matmul with the forward basis, sqrt/atan2; cos/sin + cat, matmul with the inverse basis + F.fold for the overlap-add,
      and the window sum-square envelope built with numpy on the host and copied on every call, as stft.py:117-128 does (so
      it includes that host round trip).  This is not the reference's own F.conv1d / F.conv_transpose1d: that form is not
      timed here.  All of this package's figures are printed before the first statement call.
The useful work is 2 * 2*(N/2+1) * N FLOP per frame for either direction (about 1.6 GFLOP per call here); the line for each
kernel gives that over its time.  A run without a GPU fails."""
import argparse, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=9.0)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--gl-reps", type=int, default=5)
ap.add_argument("--no-statement", action="store_true")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F
from tacotron2_subword_amd import stft as S
from tacotron2_subword_amd.audio_processing import griffin_lim, window_sumsquare
from tacotron2_subword_amd.bias_remover import hifiganBiasRemover

assert torch.cuda.is_available(), "time_stft.py measures on the GPU: none found"
N, HOP, WIN, SR = 1024, 256, 1024, 22050


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


# ---- the matmul/fold statement of stft.py:77-136, bias_remover.py:31-36, audio_processing.py:59-75
def t_transform(m, x):
    xp = F.pad(x.view(x.size(0), 1, 1, -1), (N // 2, N // 2, 0, 0), mode="reflect").squeeze(1)
    ft = torch.matmul(xp[:, 0].unfold(1, N, HOP), m.forward_basis[:, 0, :].t()).transpose(1, 2)
    re, im = ft[:, :N // 2 + 1], ft[:, N // 2 + 1:]
    return torch.sqrt(re ** 2 + im ** 2), torch.atan2(im, re)


def t_inverse(m, mag, ph):
    X = torch.cat([mag * torch.cos(ph), mag * torch.sin(ph)], dim=1)
    nfr = mag.size(-1)
    y = F.fold(torch.matmul(m.inverse_basis[:, 0, :].t(), X), (1, N + HOP * (nfr - 1)), (1, N), stride=(1, HOP)).view(mag.size(0), 1, -1)
    env = window_sumsquare("hann", mag.size(-1), hop_length=HOP, win_length=WIN, n_fft=N, dtype=np.float32)
    nz = torch.from_numpy(np.where(env > np.finfo(np.float32).tiny)[0]).cuda()
    env = torch.from_numpy(env).cuda()
    y[:, :, nz] /= env[nz]
    y *= float(N) / HOP
    return y[:, :, N // 2:-(N // 2)]


def t_remove(m, bias, x, strength):
    mag, ph = t_transform(m, x)
    return t_inverse(m, torch.clamp(mag - bias * strength, 0.0), ph)


def t_griffin_lim(m, mag, angles, iters):
    sig = t_inverse(m, mag, angles).squeeze(1)
    for _ in range(iters):
        _, ang = t_transform(m, sig)
        sig = t_inverse(m, mag, ang).squeeze(1)
    return sig


n = int(a.seconds * SR)
g = torch.Generator().manual_seed(3)
t = torch.arange(n) / SR
x = (0.4 * torch.sin(2 * np.pi * 440 * t) + 0.2 * torch.sin(2 * np.pi * 1700 * t) + 0.05 * torch.randn(n, generator=g)).clamp(-1, 1).view(1, n).cuda()
noise = torch.randn(88 * 256, generator=g).cuda()
model = lambda mel: (noise + mel.sum()).view(1, 1, -1)             # a stand-in vocoder: the remover only needs its output for zeros
with torch.no_grad():
    m = S.STFT(N, HOP, WIN).cuda()
    br = hifiganBiasRemover(model, N, N // HOP, WIN).cuda()
    mag, ph = m.transform(x)
    nf = mag.shape[-1]
    angles = ((torch.rand(mag.shape, generator=g) * 2 - 1) * np.pi).cuda()
    gflop = 2.0 * 2 * (N // 2 + 1) * N * nf / 1e9
    print(f"{a.seconds:g} s at {SR} Hz = {n} samples, {nf} frames, {N}/{HOP}/{WIN}, B = 1, fp32; {gflop:.2f} GFLOP per transform or inverse; "
          f"{a.warmup} warm-up + {a.reps} timed calls per figure ({a.gl_reps} for Griffin-Lim)", flush=True)
    packed = m.tables()
    re, im = S.analysis(x, packed, N, HOP)
    k_ana = event_ms(lambda: S.analysis(x, packed, N, HOP), a.warmup, a.reps)
    k_ana4 = event_ms(lambda: S.analysis(x, packed, N, HOP, want=("re", "im", "mag", "phase")), a.warmup, a.reps)
    k_pol = event_ms(lambda: S.synthesis(mag, ph, packed, N, HOP), a.warmup, a.reps)
    k_den = event_ms(lambda: S.synthesis(re, im, packed, N, HOP, mode=1, bias=br.bias_spec, strength=0.9), a.warmup, a.reps)
    for name, ms in (("analysis kernel (re, im)", k_ana), ("analysis kernel (re, im, mag, phase)", k_ana4), ("synthesis kernel, polar", k_pol),
                     ("synthesis kernel, denoise", k_den)):
        print(f"  {name:38s} {ms:8.3f} ms/call  {gflop / ms:7.2f} TFLOP/s", flush=True)
    rows = [("(a) hifiganBiasRemover.forward", lambda: br(x, 0.9), lambda: t_remove(m, br.bias_spec, x, 0.9), a.reps),
            ("(b) STFT.forward", lambda: m.forward(x), lambda: t_inverse(m, *t_transform(m, x)), a.reps),
            ("    STFT.transform (unchanged path)", lambda: m.transform(x), lambda: t_transform(m, x), a.reps),
            ("    STFT.inverse", lambda: m.inverse(mag, ph), lambda: t_inverse(m, mag, ph), a.reps),
            ("(c) griffin_lim, 30 iterations", lambda: griffin_lim(mag, m, 30, angles=angles), lambda: t_griffin_lim(m, mag, angles, 30), a.gl_reps)]
    ours_ms = {}
    for name, ours, theirs, reps in rows:
        ours_ms[name] = event_ms(ours, min(a.warmup, reps), reps)
        print(f"  {name:38s} {ours_ms[name]:8.3f} ms/call", flush=True)
    if not a.no_statement:
        print("matmul/fold statement in torch ops:", flush=True)
        for name, ours, theirs, reps in rows:
            tms = event_ms(theirs, min(a.warmup, reps), reps)
            o, t_ = ours(), theirs()
            err = float((o[0] - t_[0]).abs().max()) if isinstance(o, tuple) else float((o - t_).abs().max())
            print(f"  {name:38s} {tms:8.3f} ms/call  = {tms / ours_ms[name]:5.2f} x this package's; max-abs difference {err:.2e}", flush=True)
