"""Shared by the log-mel backward tests (csrc/melspec.hip melspec_grad_kernel, csrc/stft.hip stft_analysis_backward): the fp64
restatement of the gradient with respect to the samples, written out formula by formula, and torch autograd through the
melspec_ref-style ops in either precision.

    ds[m][f]  = g[m][f] / s[m][f]  where s >= clip (torch.clamp's mask), else 0
    dmag[bin] = sum_m melb[m][bin] * ds[m]
    dz        = dmag * z / mag     where mag > 0, else exactly 0     (the zero rule: torch gives 0 * inf = NaN there)
    dxpad[t]  = sum_{f*hop + k = t} sum_c fwd[c][k] * dz[c][f]
    dx[i]     = dxpad[pad+i] + [1 <= i <= pad] dxpad[pad-i] + [L-1-pad <= i <= L-2] dxpad[pad+2(L-1)-i],  i < L;  0 behind L

The yardstick of the GPU test is measured, not invented: `rel_err` of the fp32 torch-op statement (`autograd` with
dtype=float32, melspec_ref.logmel32's ops) against fp64 on the same cases."""
import torch
import torch.nn.functional as F

import melspec_ref as M  # noqa: F401  (configurations and signal for the tests that import this module)


def forward64(x, fwd, N, hop, pad):
    """One item x [L] -> (re, im) [bins, nf] in fp64 with its own reflect padding."""
    xp = F.pad(x.double()[None, None, None, :], (pad, pad, 0, 0), mode="reflect")[0, 0]
    y = F.conv1d(xp[None], fwd.double()[:, None, :], stride=hop)[0]
    c = N // 2 + 1
    return y[:c], y[c:]


def fold64(dxpad, L, pad):
    """The reflect padding's backward, the three terms in the order above."""
    dx = dxpad[pad:pad + L].clone()
    for i in range(1, min(pad, L - 1) + 1):
        dx[i] += dxpad[pad - i]
    for i in range(max(L - 1 - pad, 0), L - 1):
        dx[i] += dxpad[pad + 2 * (L - 1) - i]
    return dx


def overlap_add64(d_re, d_im, fwd, N, hop, padded_len):
    """dxpad [padded_len] from dz [bins, nf]: every frame adds fwd^T dz[:, f] at f*hop."""
    c = N // 2 + 1
    fwd = fwd.double()
    contrib = d_re.t() @ fwd[:c] + d_im.t() @ fwd[c:]             # [nf, N]
    dxpad = torch.zeros(padded_len, dtype=torch.float64)
    for f in range(contrib.shape[0]):
        dxpad[f * hop:f * hop + N] += contrib[f]
    return dxpad


def backward64(x, fwd, melb, N, hop, pad, g, mag_eps=0.0, clip=1e-5, lengths=None):
    """x [B, n], g [B, n_mels, nf_max] (read at an item's own frames only) -> dict(dx [B, n], min_mag, min_mel, clipped) in fp64.
    Item b is x[b, :lengths[b]] alone; dx is 0 behind its length."""
    B, n = x.shape
    melb = melb.double()
    dx = torch.zeros(B, n, dtype=torch.float64)
    min_mag, min_mel, clipped = float("inf"), float("inf"), 0
    for b in range(B):
        L = n if lengths is None else int(lengths[b])
        nf = M.frames(L, N, hop, pad)
        if nf == 0:
            continue
        re, im = forward64(x[b, :L], fwd, N, hop, pad)
        assert re.shape[1] == nf
        mag = torch.sqrt(re ** 2 + im ** 2 + mag_eps)
        s = melb @ mag
        live = s >= clip
        ds = torch.where(live, g[b, :, :nf].double() / torch.where(live, s, torch.ones_like(s)), torch.zeros_like(s))
        dmag = melb.t() @ ds
        pos = mag > 0
        safe = torch.where(pos, mag, torch.ones_like(mag))
        d_re = torch.where(pos, dmag * re / safe, torch.zeros_like(mag))
        d_im = torch.where(pos, dmag * im / safe, torch.zeros_like(mag))
        dx[b, :L] = fold64(overlap_add64(d_re, d_im, fwd, N, hop, L + 2 * pad), L, pad)
        min_mag, min_mel, clipped = min(min_mag, float(mag.min())), min(min_mel, float(s.min())), clipped + int((~live).sum())
    return dict(dx=dx, min_mag=min_mag, min_mel=min_mel, clipped=clipped)


def autograd(x, fwd, melb, N, hop, pad, g, mag_eps=0.0, clip=1e-5, lengths=None, dtype=torch.float64, mag_floor=0.0):
    """The same gradient from torch autograd through melspec_ref.logmel32's ops in `dtype`, item by item -> dx [B, n] (dtype).
    mag_floor is added under the square root beside mag_eps (the silence test gives the magnitude an epsilon with it)."""
    B, n = x.shape
    dx = torch.zeros(B, n, dtype=dtype)
    c = N // 2 + 1
    for b in range(B):
        L = n if lengths is None else int(lengths[b])
        nf = M.frames(L, N, hop, pad)
        if nf == 0:
            continue
        xi = x[b, :L].to(dtype).clone().requires_grad_(True)
        xp = F.pad(xi[None, None, None, :], (pad, pad, 0, 0), mode="reflect")[0]
        y = F.conv1d(xp, fwd.to(dtype)[:, None, :], stride=hop)[0]
        mag = torch.sqrt(y[:c] ** 2 + y[c:] ** 2 + mag_eps + mag_floor)
        out = torch.log(torch.clamp(torch.matmul(melb.to(dtype), mag), min=clip))
        (out * g[b, :, :nf].to(dtype)).sum().backward()
        dx[b, :L] = xi.grad
    return dx


def analysis_autograd(x, fwd, N, hop, d_re, d_im, lengths=None, dtype=torch.float64):
    """dx of sum(re * d_re + im * d_im) through reflect pad (N/2) and conv1d, item by item; d_* [B, bins, nf_max]."""
    B, n = x.shape
    dx = torch.zeros(B, n, dtype=dtype)
    c, pad = N // 2 + 1, N // 2
    for b in range(B):
        L = n if lengths is None else int(lengths[b])
        xi = x[b, :L].to(dtype).clone().requires_grad_(True)
        xp = F.pad(xi[None, None, None, :], (pad, pad, 0, 0), mode="reflect")[0]
        y = F.conv1d(xp, fwd.to(dtype)[:, None, :], stride=hop)[0]
        nf = y.shape[1]
        ((y[:c] * d_re[b, :, :nf].to(dtype)).sum() + (y[c:] * d_im[b, :, :nf].to(dtype)).sum()).backward()
        dx[b, :L] = xi.grad
    return dx


def rel_err(got, ref):
    """max |got - ref| / max |ref| per item -> list of floats."""
    return [float((got[b].double() - ref[b]).abs().max() / ref[b].abs().max()) for b in range(ref.shape[0])]


def upstream(B, n_mels, nf, seed=0):
    """The fixed seeded normal upstream gradient [B, n_mels, nf]."""
    return torch.randn(B, n_mels, nf, generator=torch.Generator().manual_seed(1000 + seed))


def silence_signal(N, hop, n):
    """Five hops of exact zeros, then melspec_ref.signal."""
    x = M.signal(1, n)
    x[:, :5 * hop] = 0.0
    return x
