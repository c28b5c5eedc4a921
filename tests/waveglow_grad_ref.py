"""Differentiable restatement of WaveGlow's training direction for the tests: the forward of waveglow_fwd_ref without its
``no_grad``, built on waveglow_ref.wn, waveglow_ref.fold and waveglow_fwd_ref.upsample (none of which has one inside), and the
per-parameter gradients by CPU autograd in fp64 or fp32, for WaveGlowLoss and for an arbitrary linear functional of (z, log_s).

Parameters travel as state dicts with the reference's keys, weight-normed (``weight_g`` / ``weight_v``) or folded (``weight``);
the gradients come back under the same keys."""
import torch
import torch.nn.functional as F

import waveglow_fwd_ref as FR
import waveglow_ref as R


def forward(sd, cfg, mel, audio, dtype=torch.float64):
    """(z [B, G, L], [log_s_k], [logdet W_k]) as differentiable functions of the tensors of ``sd`` (already of ``dtype``)."""
    G, ne = cfg["n_group"], cfg["n_early_size"]
    folded = R.fold(sd)
    B, N = audio.shape
    L = N // G
    spect = FR.upsample(folded, cfg, mel, N, dtype)
    x = audio[:, :L * G].to(dtype).reshape(B, L, G).permute(0, 2, 1)
    outs, log_s, logdet = [], [], []
    for k in range(cfg["n_flows"]):
        if k % cfg["n_early_every"] == 0 and k > 0:
            outs.append(x[:, :ne])
            x = x[:, ne:]
        W = folded[f"convinv.{k}.conv.weight"]
        logdet.append(torch.logdet(W.squeeze(-1)))
        x = F.conv1d(x, W)
        nh = x.shape[1] // 2
        a0, a1 = x[:, :nh], x[:, nh:]
        o = R.wn(folded, cfg, k, a0, spect, dtype)
        log_s.append(o[:, nh:])
        x = torch.cat([a0, torch.exp(o[:, nh:]) * a1 + o[:, :nh]], 1)
    outs.append(x)
    return torch.cat(outs, 1), log_s, logdet


def loss(z, log_s, logdet, sigma):
    """WaveGlowLoss(sigma) (glow.py:48-59) in the dtype of its inputs; logdet per matrix, as ``forward`` returns it."""
    B, G, L = z.shape
    total = torch.sum(z * z) / (2 * sigma * sigma)
    for s, ld in zip(log_s, logdet):
        total = total - torch.sum(s) - B * L * ld
    return total / z.numel()


def functional(z, log_s, cz, cs):
    """sum cz * z + sum_k sum cs[k] * log_s[k]; cs[k] None leaves log_s[k] out."""
    total = torch.sum(cz.to(z.dtype) * z)
    for s, c in zip(log_s, cs):
        if c is not None:
            total = total + torch.sum(c.to(s.dtype) * s)
    return total


def leaves(sd, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def grads(sd, cfg, mel, audio, dtype=torch.float64, sigma=None, cz=None, cs=None):
    """({key: gradient}, value, (z, log_s)) of WaveGlowLoss(sigma) -- or, sigma None, of ``functional`` -- by CPU autograd in ``dtype``."""
    p = leaves(sd, dtype)
    z, log_s, logdet = forward(p, cfg, mel, audio, dtype)
    value = loss(z, log_s, logdet, sigma) if sigma is not None else functional(z, log_s, cz, cs)
    value.backward()
    return ({k: (torch.zeros_like(v) if v.grad is None else v.grad).detach() for k, v in p.items()}, float(value.detach()),
            (z.detach(), [s.detach() for s in log_s]))


def sgd_steps(sd, cfg, mel, audio, dtype, sigma, lr, steps):
    """Plain SGD (p -= lr * grad) on WaveGlowLoss(sigma): ([loss before every step, loss after the last], final state dict)."""
    sd = {k: v.detach().to(dtype).clone() for k, v in sd.items()}
    losses = []
    for _ in range(steps):
        g, value, _ = grads(sd, cfg, mel, audio, dtype, sigma=sigma)
        losses.append(value)
        sd = {k: v - lr * g[k] for k, v in sd.items()}
    with torch.no_grad():
        losses.append(float(loss(*forward(sd, cfg, mel, audio, dtype), sigma)))
    return losses, sd
