"""Functional restatement of WaveGlow's forward direction (audio -> z, log_s, log det W and the negative log-likelihood; the
structure of glow.py:207-249 and :48-59) for the tests: fp64 or fp32 on the CPU, built on waveglow_ref's ``wn`` and ``fold``.

    spect = ConvTranspose1d(n_mel, n_mel, 1024, stride 256)(mel)[:, :, :N], regrouped to [B, n_mel*G, L], L = N // G
            (N may reach (T-1)*256 + 1024: the trailing samples of the transposed conv are kept, where waveglow_ref.upsample cuts
            at T*256)
    x = audio[:, :L*G] regrouped to [B, G, L]
    for k = 0 .. n_flows-1:   if k % n_early_every == 0 and k > 0: the first n_early_size channels of x leave for z
        x = W_k x;  (a0, a1) = halves of x;  (b, s) = WN_k(a0, spect);  x = cat(a0, exp(s) * a1 + b);  log_s[k] = s
    z = cat(early outputs, k ascending; x);  log_det_W[k] = B * L * logdet(W_k)
    loss = (sum z^2 / (2 sigma^2) - sum_k sum log_s[k] - sum_k log_det_W[k]) / (B * G * L)"""
import torch
import torch.nn.functional as F

import waveglow_ref as R

HOP, UPK = R.HOP, R.UPK


def max_samples(T):
    """The length of the transposed conv's output: more audio than that is refused (glow.py:216)."""
    return (T - 1) * HOP + UPK


def upsample(folded, cfg, mel, n_samples, dtype=torch.float64):
    """The regrouped conditioning [B, n_mel*G, L] for n_samples of audio (glow.py:215-221)."""
    G = cfg["n_group"]
    up = F.conv_transpose1d(mel.to(dtype), folded["upsample.weight"].to(dtype), folded["upsample.bias"].to(dtype), stride=HOP)
    assert up.shape[2] == max_samples(mel.shape[2]) >= n_samples
    L = n_samples // G
    B, M, _ = up.shape
    return up[:, :, :L * G].reshape(B, M, L, G).permute(0, 1, 3, 2).reshape(B, M * G, L)


def forward(folded, cfg, mel, audio, dtype=torch.float64):
    """(z [B, G, L], [log_s_k [B, n_half_k, L]], logdet [n_flows] = log|det W_k| per matrix, NaN for a negative determinant)."""
    G, ne = cfg["n_group"], cfg["n_early_size"]
    with torch.no_grad():
        B, N = audio.shape
        L = N // G
        spect = upsample(folded, cfg, mel, N, dtype)
        x = audio[:, :L * G].to(dtype).reshape(B, L, G).permute(0, 2, 1)
        outs, log_s, logdet = [], [], []
        for k in range(cfg["n_flows"]):
            if k % cfg["n_early_every"] == 0 and k > 0:
                outs.append(x[:, :ne])
                x = x[:, ne:]
            W = folded[f"convinv.{k}.conv.weight"].to(dtype)
            logdet.append(torch.logdet(W.squeeze(-1)))
            x = F.conv1d(x, W)
            nh = x.shape[1] // 2
            a0, a1 = x[:, :nh], x[:, nh:]
            o = R.wn(folded, cfg, k, a0, spect, dtype)
            log_s.append(o[:, nh:])
            x = torch.cat([a0, torch.exp(o[:, nh:]) * a1 + o[:, :nh]], 1)
        outs.append(x)
        return torch.cat(outs, 1), log_s, torch.stack(logdet)


def nll_items(z, log_s, logdet, sigma):
    """[B]: every item's mean negative log-likelihood per sample; logdet per matrix, as ``forward`` returns it."""
    B, G, L = z.shape
    s = sum(t.double().flatten(1).sum(1) for t in log_s)
    return ((z.double() ** 2).flatten(1).sum(1) / (2.0 * sigma * sigma) - s - L * logdet.double().sum()) / (G * L)


def loss(z, log_s, logdet, sigma):
    """WaveGlowLoss(sigma) of the tuple, in fp64."""
    return nll_items(z, log_s, logdet, sigma).mean()


def loss_magnitude(z, log_s, logdet, sigma):
    """M = (sum z^2 / (2 sigma^2) + sum |log_s| + |sum_k B * L * logdet_k|) / (B * G * L): the size of the terms the loss adds."""
    B, G, L = z.shape
    s = sum(float(t.double().abs().sum()) for t in log_s)
    return (float((z.double() ** 2).sum()) / (2.0 * sigma * sigma) + s + abs(B * L * float(logdet.double().sum()))) / (B * G * L)


def skew_mixes(sd, cfg, seed):
    """The state dict with every 1x1 mix replaced by Q * diag(d), Q the orthonormal matrix it holds, d log-uniform in [0.5, 2]:
    a positive determinant whose logarithm is far from zero (the orthonormal ones have log det = 0, which pins nothing)."""
    g = torch.Generator().manual_seed(seed)
    out = dict(sd)
    for k, ch in enumerate(R.flow_channels(cfg)):
        d = torch.exp((torch.rand(ch, generator=g) * 2 - 1) * 0.6931471805599453)
        key = f"convinv.{k}.conv.weight"
        out[key] = (sd[key].squeeze(-1) * d.view(1, ch)).view(ch, ch, 1).contiguous()
    return out
