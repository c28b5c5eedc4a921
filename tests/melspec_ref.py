"""Shared by the log-mel tests (csrc/melspec.hip): the test signal, the fp64 formulas built on stft_ref.analysis64, and the
per-element bound the kernel is held to.

The bound is derived, not fitted:
  re, im:     e = 1e-6 * S + 1e-7 per element, S = the same products over absolute values in fp64 (test_gpu_stft.py: an fp32
              MFMA chain is a k-ordered fmaf chain with up to 3.5e-7 * S of error; 1e-6 is that with a margin of 3).
  magnitude:  | |z'| - |z| | <= |z' - z| <= hypot(e_re, e_im), and sqrt(|z|^2 + eps) is 1-Lipschitz in |z| as well; the two
              squares, the add(s) and sqrtf add a few ulp: 4e-7 * magnitude.
  mel:        sum_bin melb * (magnitude bound), plus the second chain's own error 1e-6 * sum_bin melb * magnitude (melb >= 0).
  log-mel:    d log(v) = dv / v: the mel bound over max(mel, clip).  logf's own rounding (1 ulp of a value below 16: 1e-6) is
              within the margin of the first term.
The second convention compared with torch.stft adds 2^-24 * S to e: the kernel's basis table is the fp32 rounding of the
windowed Fourier basis that torch.stft applies in fp64."""
import math

import torch
import torch.nn.functional as F

import stft_ref

CONFIGS = {"default": (1024, 256, 1024, 80), "small": (64, 16, 64, 8), "short_window": (512, 128, 400, 20), "nonpow2": (800, 200, 800, 80)}


def signal(B, n, seed=0):
    """test_gpu_stft.py's _signal restated ((0.3 + 0.5 t/n) * sign_t * gain_b + a seeded tone), clamped to [-1, 1]."""
    g = torch.Generator().manual_seed(100 + seed)
    t = torch.arange(n, dtype=torch.float64)
    gain = torch.tensor([1.0, -0.75, 0.5, 0.9])[:B].double().view(B, 1)
    f = (0.01 + 0.2 * torch.rand(B, 1, generator=g, dtype=torch.float64))
    ph = 6.0 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    sign = (torch.randint(0, 2, (n,), generator=torch.Generator().manual_seed(55)) * 2 - 1).double()
    return (gain * sign * (0.3 + 0.5 * t / n) + 0.2 * torch.sin(2 * math.pi * f * t + ph)).clamp(-1.0, 1.0).float()


def frames(length, N, hop, pad):
    return (length + 2 * pad - N) // hop + 1 if (length > pad and length + 2 * pad >= N) else 0


def analysis64(x, fwd, N, hop, pad):
    """x [B, n], fwd [2*(N/2+1), N] -> (re, im, (S_re, S_im)) in fp64 with `pad` samples of reflect padding per side."""
    if pad == N // 2:
        return stft_ref.analysis64(x, fwd, N, hop)
    x, fwd = x.double(), fwd.double()
    xp = F.pad(x[:, None, None, :], (pad, pad, 0, 0), mode="reflect")[:, 0]
    y = F.conv1d(xp, fwd[:, None, :], stride=hop)
    s = F.conv1d(xp.abs(), fwd.abs()[:, None, :], stride=hop)
    c = N // 2 + 1
    return y[:, :c], y[:, c:], (s[:, :c], s[:, c:])


def logmel64(x, fwd, melb, N, hop, pad, mag_eps=0.0, clip=1e-5, C=1.0, basis_rounding=0.0):
    """-> dict(mel, logmel, mel_bound, log_bound), each [B, n_mels, frames] in fp64.  fwd and melb are what the kernel is
    given (fp32 values); basis_rounding = 2^-24 when fwd is an fp64 basis that the kernel holds rounded to fp32."""
    re, im, (sre, sim) = analysis64(x, fwd, N, hop, pad)
    melb = melb.double()
    e_re = (1e-6 + basis_rounding) * sre + 1e-7
    e_im = (1e-6 + basis_rounding) * sim + 1e-7
    mag = torch.sqrt(re ** 2 + im ** 2 + mag_eps)
    mag_bound = torch.sqrt(e_re ** 2 + e_im ** 2) + 4e-7 * mag
    mel = torch.matmul(melb, mag)
    mel_bound = torch.matmul(melb.abs(), mag_bound) + 1e-6 * torch.matmul(melb.abs(), mag)
    return dict(mel=mel, logmel=torch.log(torch.clamp(mel, min=clip) * C), mel_bound=mel_bound, log_bound=mel_bound / torch.clamp(mel, min=clip),
                clipped=(mel <= clip))


def logmel32(x, fwd, melb, N, hop, pad, mag_eps=0.0, clip=1e-5, C=1.0):
    """The same formula in fp32 torch ops on the CPU (what the module computes for CPU tensors)."""
    xp = F.pad(x[:, None, None, :], (pad, pad, 0, 0), mode="reflect")[:, 0]
    y = F.conv1d(xp, fwd[:, None, :], stride=hop)
    c = N // 2 + 1
    mag = torch.sqrt(y[:, :c] ** 2 + y[:, c:] ** 2 + mag_eps)
    return torch.log(torch.clamp(torch.matmul(melb, mag), min=clip) * C)


def stft_basis64(N, win):
    """The windowed Fourier basis torch.stft applies, in fp64: rows cos then -sin, times the periodic Hann window centre-padded
    to N."""
    k = torch.arange(N // 2 + 1, dtype=torch.float64)[:, None]
    t = torch.arange(N, dtype=torch.float64)[None, :]
    w = torch.hann_window(win, dtype=torch.float64)
    lp = (N - win) // 2
    w = F.pad(w, (lp, N - win - lp))
    ang = 2 * math.pi * k * t / N
    return torch.cat([torch.cos(ang), -torch.sin(ang)], 0) * w
