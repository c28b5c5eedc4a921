"""Shared by the STFT synthesis / bias removal tests: the recording's inputs restated, and the fp64 formulas the kernels of
csrc/stft.hip are held to."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = {"default": (1024, 256, 1024), "short_window": (512, 128, 400), "small": (64, 16, 64)}


def golden():
    z = np.load(os.path.join(GOLDEN, "stft_inverse.npz"))
    return {k: z[k] for k in z.files}


def wave():
    """The waveform of tests/golden/make_golden_stft.py (B = 2, n = 4000), as stored in stft.npz."""
    return torch.from_numpy(np.load(os.path.join(GOLDEN, "stft.npz"))["wave"])


def stub_model(mel):
    """tests/golden/make_golden_stft_inverse.py's stand-in vocoder restated: a fixed affine map mel [1, 80, 88] ->
    audio [1, 1, 88 * 256], seeded noise plus a per-frame weighted sum of the mel."""
    g = np.random.Generator(np.random.PCG64(5))
    c = torch.from_numpy(g.normal(size=88 * 256).astype(np.float32)).to(mel)
    w = torch.from_numpy((g.normal(size=80) / 80).astype(np.float32)).to(mel)
    return (c + (mel[0] * w[:, None]).sum(0).repeat_interleave(256)).view(1, 1, -1)


def analysis64(x, fwd, N, hop):
    """x [B, n], fwd [2*(N/2+1), N] -> (re, im, S) in fp64; S is the same product over absolute values."""
    x, fwd = x.double(), fwd.double()
    xp = F.pad(x[:, None, None, :], (N // 2, N // 2, 0, 0), mode="reflect")[:, 0]
    y = F.conv1d(xp, fwd[:, None, :], stride=hop)
    s = F.conv1d(xp.abs(), fwd.abs()[:, None, :], stride=hop)
    c = N // 2 + 1
    return y[:, :c], y[:, c:], (s[:, :c], s[:, c:])


def ola64(X, inv, N, hop):
    """X [B, 2*(N/2+1), nf], inv [2*(N/2+1), N] -> the untrimmed overlap-add sum [B, 1, N + hop*(nf-1)] in fp64."""
    return F.conv_transpose1d(X.double(), inv.double()[:, None, :], stride=hop)


def envelope64(wsq, nf, N, hop):
    """The sum-square envelope in exact fp64 (the kernel rounds each partial sum to fp32 as numpy does)."""
    env = torch.zeros(N + hop * (nf - 1), dtype=torch.float64)
    for i in range(nf):
        env[i * hop:i * hop + N] += wsq
    return env


def finish64(y, env32, N, hop):
    """stft.py:117-134 in fp64 on the untrimmed sum y, with the fp32 envelope the reference divides by."""
    y = y.clone()
    if env32 is not None:
        env = torch.from_numpy(np.asarray(env32)).double()
        nz = env > float(np.finfo(np.float32).tiny)
        y[:, :, nz] /= env[nz]
        y *= float(N) / hop
    return y[:, :, N // 2:y.shape[-1] - N // 2]
