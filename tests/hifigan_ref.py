"""Functional restatement of the HiFi-GAN generator on torch.nn.functional, written from the model's definition
(Kong et al. 2020, and the structure hifigan_model.py:75-116 gives it), for the tests: fp64 or fp32 on the CPU.  Plus the
helpers that make seeded weights whose activations neither vanish nor saturate the tanh.

    x = conv_pre(mel)
    per stage i:  x = ups[i](lrelu(x, 0.1));  x = mean_j resblock[i, j](x)
    audio = tanh(conv_post(lrelu(x, 0.01)))          # torch's default slope in front of conv_post
    ResBlock1: x = c2_m(lrelu(c1_m(lrelu(x)))) + x for the three (c1_m dilated, c2_m plain) pairs
    ResBlock2: x = c_m(lrelu(x)) + x for the two dilated convs

State dicts use the reference's keys: weight-normed ``<layer>.bias / .weight_g / .weight_v``, folded ``<layer>.bias /
.weight``.  ``h`` is anything with the config's fields as attributes or keys."""
import json

import torch
import torch.nn.functional as F


class H(dict):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.__dict__ = self


def load_config(path):
    with open(path) as f:
        return H(json.load(f))


def layer_names(h):
    """[(name, kind, cin, cout, k, d_or_u)] in state-dict order; kind 'conv' or 'convT'."""
    c0, nk = h["upsample_initial_channel"], len(h["resblock_kernel_sizes"])
    out = [("conv_pre", "conv", 80, c0, 7, 1)]
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        out.append((f"ups.{i}", "convT", c0 >> i, c0 >> (i + 1), k, u))
    for i in range(len(h["upsample_rates"])):
        ch = c0 >> (i + 1)
        for j, (k, ds) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            n = i * nk + j
            if str(h["resblock"]) == "1":
                out += [(f"resblocks.{n}.convs1.{m}", "conv", ch, ch, k, d) for m, d in enumerate(ds)]
                out += [(f"resblocks.{n}.convs2.{m}", "conv", ch, ch, k, 1) for m in range(len(ds))]
            else:
                out += [(f"resblocks.{n}.convs.{m}", "conv", ch, ch, k, d) for m, d in enumerate(ds)]
    out.append(("conv_post", "conv", ch, 1, 7, 1))
    return out


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


def _walk(h, mel, layer):
    """The generator's data flow; layer(name, x) applies the named conv (without any activation)."""
    nk = len(h["resblock_kernel_sizes"])
    kind1 = str(h["resblock"]) == "1"
    x = layer("conv_pre", mel)
    for i in range(len(h["upsample_rates"])):
        x = layer(f"ups.{i}", F.leaky_relu(x, 0.1))
        xs = None
        for j in range(nk):
            n, r = i * nk + j, x
            for m in range(len(h["resblock_dilation_sizes"][j])):
                if kind1:
                    t = layer(f"resblocks.{n}.convs1.{m}", F.leaky_relu(r, 0.1))
                    r = layer(f"resblocks.{n}.convs2.{m}", F.leaky_relu(t, 0.1)) + r
                else:
                    r = layer(f"resblocks.{n}.convs.{m}", F.leaky_relu(r, 0.1)) + r
            xs = r if xs is None else xs + r
        x = xs / nk
    pre = layer("conv_post", F.leaky_relu(x, 0.01))
    return torch.tanh(pre), pre


def _apply(spec, x, w, b):
    _, kind, _, _, k, du = spec
    if kind == "convT":
        return F.conv_transpose1d(x, w, b, stride=du, padding=(k - du) // 2)
    return F.conv1d(x, w, b, padding=(k * du - du) // 2, dilation=du)


def generator_forward(folded, h, mel, dtype=torch.float64):
    """(audio, pre_tanh) of the generator with the folded state dict, computed in dtype on the CPU."""
    specs = {s[0]: s for s in layer_names(h)}
    with torch.no_grad():
        return _walk(h, mel.to(dtype), lambda name, x: _apply(specs[name], x, folded[name + ".weight"].to(dtype), folded[name + ".bias"].to(dtype)))


def make_state_dict(h, seed):
    """Seeded weight-normed state dict in the reference's key order: v ~ N(0, 0.01), g = ||v||, bias ~ N(0, 0.1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, kind, cin, cout, k, _ in layer_names(h):
        v = torch.randn((cin, cout, k) if kind == "convT" else (cout, cin, k), generator=g) * 0.01
        sd[name + ".bias"] = torch.randn(cout, generator=g) * 0.1
        sd[name + ".weight_g"] = v.flatten(1).norm(dim=1).view(-1, 1, 1)
        sd[name + ".weight_v"] = v
    return sd


def calibrate(sd, h, mel):
    """Rescales every layer of the weight-normed state dict, in execution order, weight_g and bias together, so that its
    output on `mel` has standard deviation 1 (0.5 for conv_post, whose bias also centres its output).  Returns a new fp32 state dict with sd's keys."""
    sd = {k: v.clone().double() for k, v in sd.items()}
    specs = {s[0]: s for s in layer_names(h)}

    def layer(name, x):
        v, g = sd[name + ".weight_v"], sd[name + ".weight_g"]
        y = _apply(specs[name], x, g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1), sd[name + ".bias"])
        s = (0.5 if name == "conv_post" else 1.0) / float(y.std())
        sd[name + ".weight_g"] = g * s
        sd[name + ".bias"] = sd[name + ".bias"] * s
        y = y * s
        if name == "conv_post":          # its input carries a constant part that the scaling alone can push far into the tanh
            sd[name + ".bias"] = sd[name + ".bias"] - y.mean()
            y = y - y.mean()
        return y

    with torch.no_grad():
        _walk(h, mel.double(), layer)
    return {k: v.float() for k, v in sd.items()}


def make_mel(B, T, seed):
    return torch.randn(B, 80, T, generator=torch.Generator().manual_seed(seed)) * 1.5 - 4.0
