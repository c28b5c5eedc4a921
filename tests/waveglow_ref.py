"""Functional restatement of WaveGlow (Prenger et al. 2018; the structure glow.py:105-293 gives it) on torch.nn.functional, for
the tests: fp64 or fp32 on the CPU.  ``infer`` takes explicit noise planes, ``forward`` is the training direction (audio -> z).

    spect = ConvTranspose1d(n_mel, n_mel, 1024, stride 256)(mel)[:, :, :T*256], regrouped to [B, n_mel*G, L], L = T*256/G
    audio = sigma * z0                                     [B, n_remaining, L]
    for k = n_flows-1 .. 0:   (a0, a1) = halves of audio
        (b, s) = WN_k(a0, spect);  a1 = (a1 - b) / exp(s);  audio = W_k^-1 cat(a0, a1)
        if k % n_early_every == 0 and k > 0:  audio = cat(sigma * z, audio)
    WN: x = start(a0); per layer i: acts = tanh(u[:nc]) * sigmoid(u[nc:]), u = in_layers[i](x) + cond_layer(spect)[2nc*i : 2nc*(i+1)];
        rs = res_skip_layers[i](acts); x += rs[:nc], out += rs[nc:] (the last layer: out += rs); returns end(out)

State dicts use the reference's keys: ``upsample.weight/.bias``, ``WN.k.in_layers.i.*``, ``WN.k.res_skip_layers.i.*``, ``WN.k.start.*``,
``WN.k.end.weight/.bias``, ``WN.k.cond_layer.*``, ``convinv.k.conv.weight``; weight-normed layers hold ``bias, weight_g, weight_v``,
folded ones ``bias, weight``.  ``cfg`` is a dict of the constructor's arguments."""
import math

import torch
import torch.nn.functional as F

HOP, UPK = 256, 1024


def flow_channels(cfg):
    """Channels of `audio` in every flow, k ascending (glow.py:198-205)."""
    out, ch = [], cfg["n_group"]
    for k in range(cfg["n_flows"]):
        if k % cfg["n_early_every"] == 0 and k > 0:
            ch -= cfg["n_early_size"]
        out.append(ch)
    return out


def early_flows(cfg):
    """The flows after which inference prepends a noise plane, in the order it reaches them (k descending)."""
    return [k for k in reversed(range(cfg["n_flows"])) if k % cfg["n_early_every"] == 0 and k > 0]


def noise_shapes(cfg, B, T):
    L = T * HOP // cfg["n_group"]
    return [(B, flow_channels(cfg)[-1], L)] + [(B, cfg["n_early_size"], L) for _ in early_flows(cfg)]


def state_dict_keys(cfg, normed=True):
    """The reference's state-dict keys in its order."""
    wn = ["bias", "weight_g", "weight_v"] if normed else ["bias", "weight"]
    keys = ["upsample.weight", "upsample.bias"]
    nl = cfg["WN_config"]["n_layers"]
    for k in range(cfg["n_flows"]):
        p = f"WN.{k}."
        keys += [f"{p}in_layers.{i}.{s}" for i in range(nl) for s in wn]
        keys += [f"{p}res_skip_layers.{i}.{s}" for i in range(nl) for s in wn]
        keys += [f"{p}start.{s}" for s in wn] + [p + "end.weight", p + "end.bias"] + [f"{p}cond_layer.{s}" for s in wn]
    return keys + [f"convinv.{k}.conv.weight" for k in range(cfg["n_flows"])]


def fold(sd):
    """Weight-normed state dict -> folded: w = g * v / ||v||, the norm over all dims but 0."""
    out = {}
    for key, t in sd.items():
        if key.endswith(".weight_g"):
            name = key[:-len(".weight_g")]
            v = sd[name + ".weight_v"]
            out[name + ".weight"] = t * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
        elif not key.endswith(".weight_v"):
            out[key] = t
    return out


def make_state_dict(cfg, seed, end_std=None):
    """Seeded weight-normed state dict in the reference's key order: torch's default initialisation (uniform in
    +-1/sqrt(fan_in)) for every conv, orthonormal matrices of determinant 1 for the 1x1 mixes, and -- the reference starts
    `end` at zero, which would make every coupling the identity -- end.weight, end.bias ~ N(0, end_std), end_std = 0.2/sqrt(nc)
    (0.05 at 16 channels), so that s keeps its size as the sum over nc channels widens."""
    g = torch.Generator().manual_seed(seed)
    nc, nl = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"]
    n_mel, n_cond = cfg["n_mel_channels"], cfg["n_mel_channels"] * cfg["n_group"]
    end_std = 0.2 / math.sqrt(nc) if end_std is None else end_std

    def uni(shape, fan_in):
        b = 1.0 / math.sqrt(fan_in)
        return (torch.rand(shape, generator=g) * 2 - 1) * b

    def conv(cout, cin, k):
        v = uni((cout, cin, k), cin * k)
        return {"bias": uni((cout,), cin * k), "weight_g": v.flatten(1).norm(dim=1).view(-1, 1, 1), "weight_v": v}

    layers = {"upsample.weight": uni((n_mel, n_mel, UPK), n_mel * UPK), "upsample.bias": uni((n_mel,), n_mel * UPK)}
    for k, ch in enumerate(flow_channels(cfg)):
        p, nh = f"WN.{k}.", ch // 2
        for i in range(nl):
            for s, t in conv(2 * nc, nc, 3).items():
                layers[f"{p}in_layers.{i}.{s}"] = t
            for s, t in conv(2 * nc if i < nl - 1 else nc, nc, 1).items():
                layers[f"{p}res_skip_layers.{i}.{s}"] = t
        for s, t in conv(nc, nh, 1).items():
            layers[f"{p}start.{s}"] = t
        layers[p + "end.weight"] = torch.randn(2 * nh, nc, 1, generator=g) * end_std
        layers[p + "end.bias"] = torch.randn(2 * nh, generator=g) * end_std
        for s, t in conv(2 * nc * nl, n_cond, 1).items():
            layers[f"{p}cond_layer.{s}"] = t
        W = torch.linalg.qr(torch.randn(ch, ch, generator=g))[0]
        if torch.det(W) < 0:
            W[:, 0] = -W[:, 0]
        layers[f"convinv.{k}.conv.weight"] = W.view(ch, ch, 1)
    return {key: layers[key] for key in state_dict_keys(cfg)}


def make_mel(B, T, seed, n_mel=80):
    return torch.randn(B, n_mel, T, generator=torch.Generator().manual_seed(seed)) * 1.5 - 4.0


def upsample(folded, cfg, mel, dtype=torch.float64):
    """The regrouped conditioning [B, n_mel*G, L] (glow.py:252-258)."""
    G = cfg["n_group"]
    up = F.conv_transpose1d(mel.to(dtype), folded["upsample.weight"].to(dtype), folded["upsample.bias"].to(dtype), stride=HOP)
    up = up[:, :, :mel.shape[2] * HOP]
    B, M, n = up.shape
    L = n // G
    return up[:, :, :L * G].reshape(B, M, L, G).permute(0, 1, 3, 2).reshape(B, M * G, L)


def wn(folded, cfg, k, a0, spect, dtype=torch.float64):
    """end(out) of flow k's WN: [B, 2*n_half, L]."""
    nc, nl = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"]
    p = f"WN.{k}."
    w = lambda name: folded[p + name].to(dtype)
    x = F.conv1d(a0, w("start.weight"), w("start.bias"))
    out = torch.zeros_like(x)
    cond = F.conv1d(spect, w("cond_layer.weight"), w("cond_layer.bias"))
    for i in range(nl):
        d = 2 ** i
        u = F.conv1d(x, w(f"in_layers.{i}.weight"), w(f"in_layers.{i}.bias"), dilation=d, padding=d) + cond[:, 2 * nc * i:2 * nc * (i + 1)]
        acts = torch.tanh(u[:, :nc]) * torch.sigmoid(u[:, nc:])
        rs = F.conv1d(acts, w(f"res_skip_layers.{i}.weight"), w(f"res_skip_layers.{i}.bias"))
        if i < nl - 1:
            x = x + rs[:, :nc]
            out = out + rs[:, nc:]
        else:
            out = out + rs
    return F.conv1d(out, w("end.weight"), w("end.bias"))


def infer(folded, cfg, mel, noise, sigma, dtype=torch.float64, details=None):
    """audio [B, L*G] of WaveGlow.infer with the given noise planes (shapes: noise_shapes).  `details`, a dict, receives
    `spect`, `s_max` (max |s| over the flows) and `flow_audio` (the tensor after flow 0, [B, G, L])."""
    with torch.no_grad():
        spect = upsample(folded, cfg, mel, dtype)
        audio = sigma * noise[0].to(dtype)
        plane, s_max = 1, 0.0
        for k in reversed(range(cfg["n_flows"])):
            nh = audio.shape[1] // 2
            a0, a1 = audio[:, :nh], audio[:, nh:]
            o = wn(folded, cfg, k, a0, spect, dtype)
            b, s = o[:, :nh], o[:, nh:]
            s_max = max(s_max, float(s.abs().max()))
            a1 = (a1 - b) / torch.exp(s)
            W = folded[f"convinv.{k}.conv.weight"].squeeze(-1)
            Winv = W.float().inverse().to(dtype) if dtype == torch.float32 else W.double().inverse()
            audio = F.conv1d(torch.cat([a0, a1], 1), Winv.unsqueeze(-1))
            if k % cfg["n_early_every"] == 0 and k > 0:
                audio = torch.cat([sigma * noise[plane].to(dtype), audio], 1)
                plane += 1
        if details is not None:
            details.update(spect=spect, s_max=s_max, flow_audio=audio)
        return audio.permute(0, 2, 1).reshape(audio.shape[0], -1)


def forward(folded, cfg, mel, audio, dtype=torch.float64):
    """z [B, G, L] of WaveGlow.forward((mel, audio)) (glow.py:207-249): early outputs first, k ascending."""
    G = cfg["n_group"]
    with torch.no_grad():
        spect = upsample(folded, cfg, mel, dtype)
        x = audio.to(dtype).reshape(audio.shape[0], -1, G).permute(0, 2, 1)
        outs = []
        for k in range(cfg["n_flows"]):
            if k % cfg["n_early_every"] == 0 and k > 0:
                outs.append(x[:, :cfg["n_early_size"]])
                x = x[:, cfg["n_early_size"]:]
            x = F.conv1d(x, folded[f"convinv.{k}.conv.weight"].to(dtype))
            nh = x.shape[1] // 2
            a0, a1 = x[:, :nh], x[:, nh:]
            o = wn(folded, cfg, k, a0, spect, dtype)
            x = torch.cat([a0, torch.exp(o[:, nh:]) * a1 + o[:, :nh]], 1)
        outs.append(x)
        return torch.cat(outs, 1)


def planes_from_z(cfg, z):
    """The noise planes (for sigma = 1) that make `infer` undo the `forward` that gave z."""
    ne, n_rem = cfg["n_early_size"], flow_channels(cfg)[-1]
    n_early = len(early_flows(cfg))
    early = [z[:, j * ne:(j + 1) * ne] for j in range(n_early)]          # k ascending
    return [z[:, z.shape[1] - n_rem:].contiguous()] + [e.contiguous() for e in reversed(early)]
