"""Gradients of the HiFi-GAN generator through torch's autograd over tests/hifigan_ref._walk, on the CPU in any dtype, for the tests:
the loss is sum(audio * gy) for a given upstream gradient gy on the audio, so every gradient is linear in gy."""
import torch

import hifigan_ref as R


def grads(sd, h, mel, gy, dtype=torch.float64):
    """({key: gradient} for every tensor of the (weight-normed or folded) state dict, the mel's gradient, the audio)."""
    specs = {s[0]: s for s in R.layer_names(h)}
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    m = mel.detach().to(dtype).clone().requires_grad_(True)

    def layer(name, x):
        if name + ".weight" in p:
            w = p[name + ".weight"]
        else:
            v, g = p[name + ".weight_v"], p[name + ".weight_g"]
            w = g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
        return R._apply(specs[name], x, w, p[name + ".bias"])

    audio, _ = R._walk(h, m, layer)
    (audio * gy.to(dtype)).sum().backward()
    return {k: v.grad for k, v in p.items()}, m.grad, audio.detach()


def upstream(B, n, seed):
    """A general gradient on the audio [B, 1, n]: random signs and sizes, nowhere zero."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 1, n, generator=g) + torch.where(torch.rand(B, 1, n, generator=g) > 0.5, 0.5, -0.5)


def sgd_steps(sd, h, mel, target, dtype, lr, steps):
    """p -= lr * grad of 0.5 * sum((audio - target)^2), `steps` times: ([the loss before every step and after the last], final state dict)."""
    sd = {k: v.detach().to(dtype).clone() for k, v in sd.items()}
    losses = []
    for n in range(steps + 1):
        a0 = _audio(sd, h, mel, dtype)
        losses.append(float(0.5 * ((a0 - target.to(dtype)) ** 2).sum()))
        if n == steps:
            break
        g, _, _ = grads(sd, h, mel, a0 - target.to(dtype), dtype)
        sd = {k: v - lr * g[k] for k, v in sd.items()}
    return losses, sd


def _audio(sd, h, mel, dtype):
    with torch.no_grad():
        return R.generator_forward(R.fold(sd) if any(k.endswith(".weight_g") for k in sd) else sd, h, mel, dtype)[0]


def adam_steps(sd, h, mel, target, dtype, lr, steps, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's update (no weight decay, no amsgrad) on 0.5 * sum((audio - target)^2), `steps` times, written out:
    ([the loss before every step and after the last], [the audio at the same points], final state dict)."""
    sd = {k: v.detach().to(dtype).clone() for k, v in sd.items()}
    m = {k: torch.zeros_like(v) for k, v in sd.items()}
    v2 = {k: torch.zeros_like(v) for k, v in sd.items()}
    losses, audios = [], []
    for n in range(steps + 1):
        a0 = _audio(sd, h, mel, dtype)
        audios.append(a0)
        losses.append(float(0.5 * ((a0 - target.to(dtype)) ** 2).sum()))
        if n == steps:
            break
        g, _, _ = grads(sd, h, mel, a0 - target.to(dtype), dtype)
        t = n + 1
        for k in sd:
            m[k] = betas[0] * m[k] + (1 - betas[0]) * g[k]
            v2[k] = betas[1] * v2[k] + (1 - betas[1]) * g[k] * g[k]
            denom = (v2[k].sqrt() / (1 - betas[1] ** t) ** 0.5) + eps
            sd[k] = sd[k] - (lr / (1 - betas[0] ** t)) * m[k] / denom
    return losses, audios, sd
