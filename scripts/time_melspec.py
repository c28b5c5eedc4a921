"""Dev tool: times of the log-mel front end (csrc/melspec.hip) on the GPU at 22 050 Hz, 1024 / 256 / 1024, 80 mel bands:

  python scripts/time_melspec.py [--seconds 9] [--warmup 5] [--reps 50] [--rounds 3] [--pairs 32]

ms per call from HIP events around --reps calls after --warmup calls, this package's path and the path it replaces timed in
the same process in alternating rounds (the figure is the median over --rounds; the spread between runs comes from repeating
the command):
  (a) B = 1, one utterance of --seconds:  TacotronSTFT.mel_spectrogram (the kernel; output allocation and the plan query are
      inside, the one-off packing of the tables is not) against the torch-op path it replaces: STFT.transform (reflect-pad
      copy, unfold into a frame matrix, the general GEMM, sqrt, atan2), matmul with the mel basis, clamp, log.
  (b) B = 64, ragged 6 .. --seconds:      the kernel with per-item lengths against the torch-op path on the dense padded
      batch (it has no lengths: it computes every padded frame).
  (c) --pairs pairs of wav files:         Audio.tools.get_mel_batch + one SoftDTW call with lengths, against the per-file
      loop of softdtw.py:78-84 (get_mel, numpy transpose, copy to the GPU, one SoftDTW call per pair).  Reading the files is
      inside both.
Then the launch shapes: the kernel alone (stft.log_mel into a caller's buffers) for B utterances of --seconds at every
split count, which is what the plan's threshold (kernels.h kMelSplitBelow) is chosen from.
The kernel's useful work is 2 * 2*(N/2+1) * N FLOP per frame (the mel product adds 2 * n_mels * (N/2+1), 4 %, not counted);
each kernel line gives that over its time and the share of the 157.3 TFLOP/s fp32 matrix peak.  A run without a GPU fails.

  python scripts/time_melspec.py --grad [--seconds 9] [--warmup 5] [--reps 50] [--rounds 3]

times instead the spectral loss  sum |mel(y_hat) - mel(y)|  in utils.mel_spectrogram's convention, forward and backward down
to y_hat.grad, at 16 x 8192 samples (HiFi-GAN's training segment) and at one utterance of --seconds: this package's path
(utils.mel_spectrogram_from_audio(differentiable=True): melspec_kernel keeping the mel sum, melspec_grad_kernel, the overlap-add
GEMM, the fold) against the same formula in torch ops under autograd on the same GPU (reflect pad, torch.stft, sqrt, matmul,
clamp, log).  Then the HIP path's two C calls alone on buffers of this script: the forward keeping the mel sum (t2_melspec) and
the whole backward (t2_melspec_backward).  The split of the backward by kernel comes from running this command under
rocprofv3 --kernel-trace --stats (profiles/README.md)."""
import argparse, os, statistics, sys, tempfile
ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=9.0)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--grad", action="store_true")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from scipy.io.wavfile import write
from tacotron2_subword_amd import _lib as L
from tacotron2_subword_amd import stft as S
from tacotron2_subword_amd.Audio import tools
from tacotron2_subword_amd.audio_processing import dynamic_range_compression
from tacotron2_subword_amd.soft_dtw_cuda import SoftDTW

assert torch.cuda.is_available(), "time_melspec.py measures on the GPU: none found"
N, HOP, WIN, SR, NMEL, PEAK = 1024, 256, 1024, 22050, 80, 157.3


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


def alternating(ours, theirs, reps):
    o, t = [], []
    for _ in range(a.rounds):
        o.append(event_ms(ours, min(a.warmup, reps), reps))
        t.append(event_ms(theirs, min(a.warmup, reps), reps))
    return statistics.median(o), statistics.median(t), o, t


def torch_op_mel(m, y):
    """The path TacotronSTFT.mel_spectrogram took for CUDA tensors before the kernel (with its two range checks, which
    synchronise, as the kernel path's do)."""
    assert torch.min(y.data) >= -1
    assert torch.max(y.data) <= 1
    mag, _ = m.stft_fn.transform(y)
    return dynamic_range_compression(torch.matmul(m.mel_basis, mag))


def signal(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / SR
    return (0.4 * torch.sin(2 * np.pi * (200 + 37 * seed) * t) + 0.2 * torch.sin(2 * np.pi * 1700 * t) + 0.05 * torch.randn(n, generator=g)).clamp(-1, 1)


def report(name, o, t, os_, ts_, note=""):
    print(f"  {name:44s} kernel path {o:8.3f} ms   replaced path {t:8.3f} ms  = {t / o:6.2f} x   (rounds: {', '.join(f'{v:.3f}' for v in os_)} | "
          f"{', '.join(f'{v:.3f}' for v in ts_)}){note}", flush=True)


def grad_times():
    from tacotron2_subword_amd import utils
    pad = (N - HOP) // 2
    front, basis = utils._front(N, NMEL, SR, HOP, WIN, 0.0, 8000.0, torch.device("cuda", torch.cuda.current_device()))
    window = torch.hann_window(WIN, device="cuda")

    def torch_mel(y):
        yp = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
        spec = torch.stft(yp, N, hop_length=HOP, win_length=WIN, window=window, center=False, return_complex=True)
        return torch.log(torch.clamp(torch.matmul(basis, torch.sqrt(spec.real.pow(2) + spec.imag.pow(2) + 1e-9)), min=1e-5))

    print(f"spectral loss sum|mel(y_hat) - mel(y)|, forward + backward to y_hat.grad, {N}/{HOP}/{WIN}, {NMEL} mel bands, pad {pad}, fp32; "
          f"{a.warmup} warm-up + {a.reps} timed calls per figure, median of {a.rounds} alternating rounds", flush=True)
    for name, B, n in (("16 x 8192 samples", 16, 8192), (f"1 x {a.seconds:g} s", 1, int(a.seconds * SR))):
        y = torch.stack([signal(n, i) for i in range(B)]).cuda()
        y_hat = (0.9 * torch.stack([signal(n, 50 + i) for i in range(B)])).cuda().requires_grad_(True)
        with torch.no_grad():
            target = utils.mel_spectrogram_from_audio(y)

        def ours():
            y_hat.grad = None
            (utils.mel_spectrogram_from_audio(y_hat, differentiable=True) - target).abs().sum().backward()

        def theirs():
            y_hat.grad = None
            (torch_mel(y_hat) - target).abs().sum().backward()

        ours()
        g_ours = y_hat.grad.clone()
        theirs()
        diff = float((g_ours - y_hat.grad).abs().max() / y_hat.grad.abs().max())
        o, t, os_, ts_ = alternating(ours, theirs, a.reps)
        report(name, o, t, os_, ts_, f"  gradients differ by {diff:.2e} of the largest")
        # the split by kernel, through the C entries on buffers of this script
        plan, gplan = L.melspec_plan(N, HOP, pad, NMEL, n, B), L.melspec_grad_plan(N, HOP, pad, NMEL, n, B)
        x = y_hat.detach().contiguous()
        out = torch.empty(B, NMEL, plan.nf_max, device="cuda")
        sums = torch.empty(B, plan.nf_max, NMEL, device="cuda")
        scratch = torch.empty(max(plan.split_scratch_floats, 1), device="cuda")
        g = torch.sign(torch.randn(B, NMEL, plan.nf_max, device="cuda"))
        ws, dx = torch.empty(gplan.workspace_floats, device="cuda"), torch.empty_like(x)
        tables, gtables = front.mel_tables(basis), front.mel_grad_tables(basis)
        fa = L.MelspecArgs(B, N, HOP, pad, NMEL, n, L.ptr(x), None, L.ptr(tables), L.ptr(out), L.ptr(scratch), scratch.numel(), None,
                           1e-9, 1e-5, 1.0, 0.0, 0, 0, 0, L.ptr(sums))
        ba = L.MelspecBackwardArgs(B, N, HOP, pad, NMEL, n, L.ptr(x), None, L.ptr(tables), L.ptr(gtables), L.ptr(sums), L.ptr(g), L.ptr(ws), ws.numel(),
                                   L.ptr(dx), 1e-9, 1e-5, 0)
        f_ms = event_ms(lambda: L.check(L.lib().t2_melspec(fa, L.stream())), a.warmup, a.reps)
        b_ms = event_ms(lambda: L.check(L.lib().t2_melspec_backward(ba, L.stream())), a.warmup, a.reps)
        print(f"    C calls alone: forward keeping the mel sum (plan splits {plan.splits}) {f_ms:.3f} ms   backward {b_ms:.3f} ms   "
              f"grids: bins ({gplan.grid_x}, {gplan.grid_y}, {gplan.grid_z}), GEMM ({gplan.fold_grid_x}, {gplan.fold_grid_y}, {B})", flush=True)


if a.grad:
    grad_times()
    sys.exit(0)

with torch.no_grad():
    m = S.TacotronSTFT(N, HOP, WIN, NMEL, SR, 0.0, 8000.0).cuda()
    n = int(a.seconds * SR)
    nf = 1 + n // HOP
    gflop = 2.0 * 2 * (N // 2 + 1) * N * nf / 1e9
    print(f"{a.seconds:g} s at {SR} Hz = {n} samples, {nf} frames, {N}/{HOP}/{WIN}, {NMEL} mel bands, fp32; {gflop:.2f} GFLOP per utterance; "
          f"{a.warmup} warm-up + {a.reps} timed calls per figure, median of {a.rounds} alternating rounds", flush=True)
    # (a)
    x1 = signal(n, 0).view(1, n).cuda()
    err = float((m.mel_spectrogram(x1) - torch_op_mel(m, x1)).abs().max())
    report(f"(a) B = 1, {a.seconds:g} s", *alternating(lambda: m.mel_spectrogram(x1), lambda: torch_op_mel(m, x1), a.reps), f"  max-abs difference {err:.2e}")
    # (b)
    B = 64
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(int(6 * SR), n + 1, (B,), generator=g)
    lens[0] = n
    xb = torch.zeros(B, n)
    for i in range(B):
        xb[i, :lens[i]] = signal(int(lens[i]), i)
    xb, lens_gpu = xb.cuda(), lens.to(torch.int32).cuda()
    frames = int((1 + lens // HOP).sum())
    o, t, os_, ts_ = alternating(lambda: m.mel_spectrogram(xb, lengths=lens_gpu), lambda: torch_op_mel(m, xb), max(1, a.reps // 5))
    report(f"(b) B = 64, ragged 6 .. {a.seconds:g} s", o, t, os_, ts_, f"  {frames} live of {B * nf} padded frames")
    # (c)
    sdtw = SoftDTW(use_cuda=True, gamma=0.1)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(2 * a.pairs):
            paths.append(os.path.join(d, f"{i}.wav"))
            write(paths[-1], SR, (signal(int(lens[i % B]), 100 + i) * 30000).round().to(torch.int16).numpy())

        def batched():
            mel, fl = tools.get_mel_batch(paths)
            return sdtw(mel[:a.pairs], mel[a.pairs:], fl[:a.pairs], fl[a.pairs:])

        def per_file():
            out = []
            for i in range(a.pairs):
                src = torch.from_numpy(np.transpose(tools.get_mel(paths[i]).numpy().astype(np.float32))).to("cuda").unsqueeze(0)
                trg = torch.from_numpy(np.transpose(tools.get_mel(paths[a.pairs + i]).numpy().astype(np.float32))).to("cuda").unsqueeze(0)
                out.append(sdtw(src, trg))
            return torch.cat(out)

        same = torch.equal(batched(), per_file())
        o, t, os_, ts_ = alternating(batched, per_file, max(1, a.reps // 10))
        report(f"(c) {a.pairs} pairs, get_mel_batch + SoftDTW", o, t, os_, ts_, f"  scores bit-identical: {same}")
    # launch shapes
    passes = L.melspec_plan(N, HOP, N // 2, NMEL, n, 1).passes
    print(f"kernel alone (caller's buffers), B utterances of {a.seconds:g} s, by split count (0 = the plan's choice):", flush=True)
    for Bk in (1, 2, 3, 4, 5, 6, 8, 12, 64):
        xs = xb[:Bk].contiguous()
        xs[:] = xb[0]
        plan = L.melspec_plan(N, HOP, N // 2, NMEL, n, Bk)
        out = torch.empty(Bk, NMEL, plan.nf_max, device="cuda")
        scratch = torch.empty(plan.split_scratch_floats, device="cuda")
        m.stft_fn.mel_tables(m.mel_basis)
        cells = []
        for s in (0, 1, 2, 3, 5, passes):
            ms = event_ms(lambda: S.log_mel(xs, m.stft_fn, m.mel_basis, force_splits=s, out=out, scratch=scratch), a.warmup, a.reps)
            cells.append(f"S={s}: {ms:7.3f} ms {gflop * Bk / ms:6.1f} TF {100 * gflop * Bk / ms / PEAK:4.1f} %")
        print(f"  B = {Bk:2d}, {plan.frame_tiles * Bk:5d} frame tiles, plan splits {plan.splits}:  " + " | ".join(cells), flush=True)
