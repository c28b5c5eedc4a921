#!/usr/bin/env python3
"""Golden vectors for WaveGlow's backward: the per-parameter gradients of WaveGlowLoss(0.7), recorded on the CPU in fp32 from the
reference's own glow.WaveGlow.forward, glow.WaveGlowLoss and torch's autograd.

Models "a" and "deep" of waveglow.npz with the skewed mixes of waveglow_forward.npz (neither is stored again); inputs are cases
1 and 3 of waveglow_forward.npz, (B, T, N) = (2, 4, 1024) and (3, 2, 1027).  Per model and case the file holds the loss and, per
tensor of the weight-normed state dict (in the order of ``{tag}_keys``), the recording's max deviation from the fp64 restatement
(tests/waveglow_grad_ref.py) and max |g64|.  The gradients themselves (``{tag}_g{n}/{key}``) are a quarter of a megabyte per
tensor-set for the upsample weight alone, so, to stay under the size limit of a committed file, they are stored for "a" on the
first case and for "deep" on the second, and of ``upsample.weight`` every 5th element of the flattened tensor (5 is coprime to
the 1024 taps: every channel pair, phase and tap group appears); the deviations cover every element of all four runs.

Run in the build container only (needs /root/reference); writes waveglow_grad.npz next to this file."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import waveglow_grad_ref as GR  # noqa: E402

CASES = [(2, 4, 1024), (3, 2, 1027)]
FORWARD_CASE = [1, 3]            # their index in waveglow_forward.npz
SIGMA = 0.7
STORED = {"a": 0, "deep": 1}     # the case whose gradients are stored in full
UP_STRIDE = 5


def main():
    sys.path.insert(0, "/root/reference")
    import glow as ref  # noqa
    base, fwd = np.load(os.path.join(HERE, "waveglow.npz")), np.load(os.path.join(HERE, "waveglow_forward.npz"))
    configs = json.loads(str(base["configs"]))
    out = dict(cases=np.array(CASES, dtype=np.int64), forward_case=np.array(FORWARD_CASE, dtype=np.int64), sigma=np.array(SIGMA),
               stored=np.array(json.dumps(STORED)), up_stride=np.array(UP_STRIDE))
    for tag, cfg in configs.items():
        keys = json.loads(str(base[f"{tag}_keys"]))
        sd = {k: torch.from_numpy(base[k if k.startswith("upsample.") else f"{tag}/{k}"]) for k in keys}
        sd = {k: torch.from_numpy(fwd[f"{tag}/{k}"]) if k.startswith("convinv.") else v for k, v in sd.items()}
        out[f"{tag}_keys"] = np.array(json.dumps(keys))
        for n, (case, fc) in enumerate(zip(CASES, FORWARD_CASE)):
            assert tuple(int(v) for v in fwd["cases"][fc]) == case
            mel, audio = torch.from_numpy(fwd[f"mel{fc}"]), torch.from_numpy(fwd[f"audio{fc}"])
            model = ref.WaveGlow(**cfg).train()
            model.load_state_dict(sd)
            z, log_s, logdet = model((mel, audio))
            loss = ref.WaveGlowLoss(SIGMA)((z, log_s, logdet))
            loss.backward()
            got = {k: p.grad.detach() for k, p in model.named_parameters()}
            assert sorted(got) == sorted(keys)
            g64, loss64, _ = GR.grads(sd, cfg, mel, audio, torch.float64, sigma=SIGMA)
            dev, mag = [], []
            for k in keys:
                assert got[k].shape == sd[k].shape == g64[k].shape
                if n == STORED[tag]:
                    out[f"{tag}_g{n}/{k}"] = got[k].flatten()[::UP_STRIDE].numpy() if k == "upsample.weight" else got[k].numpy()
                dev.append(float((got[k].double() - g64[k]).abs().max()))
                mag.append(float(g64[k].abs().max()))
                assert mag[-1] > 0, (tag, n, k)
            out[f"{tag}_dev{n}"], out[f"{tag}_mag{n}"] = np.array(dev), np.array(mag)
            out[f"{tag}_loss{n}"] = np.array([float(loss), loss64])
            rel = [d / (2.0 ** -23 * m) for d, m in zip(dev, mag)]
            print(tag, case, "loss", float(loss), "fp64", loss64, len(keys), "tensors, min max|g64|", min(mag),
                  "fp32 deviation in units of 2^-23 max|g64|:", min(rel), "..", max(rel))
    path = os.path.join(HERE, "waveglow_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
