#!/usr/bin/env python3
"""Golden vectors for SSIM, recorded once on the CPU from the reference's own ssim.py (imported here only, never by a
test).  Usage: make_golden_ssim.py <directory that holds the reference's ssim.py>; writes ssim.npz next to this file.

Per case n: x, y; the reference's fp32 value, items (size_average=False), dx and dy (gradients of the value);
dev_* = max |reference fp32 - reference fp64| and win_* = max |reference fp64 - tests/ssim_ref.py| for value, items,
map, dx, dy.  The reference does not return its map, so the map's figures come from ssim_ref.reference_form, the
reference's arrangement written out; its fp32 value is asserted bit-identical to the reference's here.

To stay under 300 KB the inputs are multiples of 2^-10 (they compress), the three silence cases share one noise array
(x = y + amp * noise, formed in fp32 by the loader below), and the four largest cases (NO_DY) hold dx but not dy; their
dev_dy / win_dy are still recorded."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ssim_ref as R  # noqa: E402

WS = 11
SILENCE = np.float32(-11.5129)
NAMES = ["mel", "padded_mel", "normal", "one_pixel", "tiny", "wide", "silence_1e-1", "silence_1e-2", "silence_1e-3"]
AMPS = {"silence_1e-1": 0.1, "silence_1e-2": 0.01, "silence_1e-3": 0.001}
NO_DY = ("padded_mel",) + tuple(AMPS)


def _q(t):
    return torch.round(t * 1024) / 1024


def _mel(g, B, T):
    coarse = torch.randn(B, 1, 10, 6, generator=g)
    base = F.interpolate(coarse, size=(80, T), mode="bilinear", align_corners=False) * 3 - 6 + 0.5 * torch.randn(B, 1, 80, T, generator=g)
    y = _q(base.clamp(min=float(SILENCE)))
    x = _q(y + 0.3 * torch.randn(B, 1, 80, T, generator=g))
    return x, y


def load_case(z, name):
    """(x, y) of a case as fp32 tensors, from the loaded npz."""
    if name in AMPS:
        noise = z["silence_noise"]
        y = np.full_like(noise, SILENCE)
        return torch.from_numpy(y + np.float32(AMPS[name]) * noise), torch.from_numpy(y)
    return torch.from_numpy(z[f"{name}_x"]), torch.from_numpy(z[f"{name}_y"])


def main():
    sys.path.insert(0, sys.argv[1])
    import ssim as ref  # noqa
    g = torch.Generator().manual_seed(2026)
    out = dict(names=np.array(NAMES), ws=np.int64(WS))
    inputs = {}
    inputs["mel"] = _mel(g, 2, 37)
    x, y = _mel(g, 3, 50)
    for b, n in enumerate((50, 31, 17)):
        x[b, :, :, n:] = 0
        y[b, :, :, n:] = 0
    inputs["padded_mel"] = (x, y)
    for name, shape in (("normal", (2, 3, 17, 23)), ("one_pixel", (1, 1, 1, 1)), ("tiny", (1, 1, 3, 4)), ("wide", (2, 1, 5, 70))):
        inputs[name] = (_q(torch.randn(*shape, generator=g)), _q(torch.randn(*shape, generator=g)))
    out["silence_noise"] = _q(torch.randn(2, 1, 80, 40, generator=g)).numpy()
    for name in NAMES:
        if name in AMPS:
            x, y = load_case(out, name)
        else:
            x, y = inputs[name]
            out[f"{name}_x"], out[f"{name}_y"] = x.numpy(), y.numpy()
        Cn = x.shape[1]
        res = {}
        for dt in (torch.float32, torch.float64):
            a, b = x.clone().to(dt).requires_grad_(True), y.clone().to(dt).requires_grad_(True)
            win = ref.create_window(WS, Cn).to(dt)
            value = ref._ssim(a, b, win, WS, Cn, True)
            value.backward()
            items = ref._ssim(a.detach(), b.detach(), win, WS, Cn, False)
            v2, smap = R.reference_form(x, y, WS, True, dt)
            if dt == torch.float32:
                assert torch.equal(v2, value.detach()), name
            res[dt] = dict(value=value.detach().reshape(1), items=items.detach(), map=smap, dx=a.grad, dy=b.grad)
        dx64, dy64 = R.ssim_grad(x, y, WS)
        mine = dict(value=R.ssim_value(x, y, WS).reshape(1), items=R.ssim_value(x, y, WS, False), map=R.ssim_map(x, y, WS), dx=dx64, dy=dy64)
        r32, r64 = res[torch.float32], res[torch.float64]
        for k in ("value", "items", "dx", "dy"):
            if not (name in NO_DY and k == "dy"):
                out[f"{name}_{k}"] = r32[k].numpy()
        for k in ("value", "items", "map", "dx", "dy"):
            out[f"{name}_dev_{k}"] = np.float64((r32[k].double() - r64[k]).abs().max())
            out[f"{name}_win_{k}"] = np.float64((r64[k] - mine[k]).abs().max())
        print(name, tuple(x.shape), "value", float(r32["value"]), " ".join(f"dev_{k}={float(out[f'{name}_dev_{k}']):.1e}" for k in ("value", "items", "map", "dx", "dy")),
              " ".join(f"win_{k}={float(out[f'{name}_win_{k}']):.1e}" for k in ("value", "items", "map", "dx", "dy")), "max|dx|", float(r64["dx"].abs().max()))
    path = os.path.join(HERE, "ssim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
