#!/usr/bin/env python3
"""Golden vectors for the HiFi-GAN generator's backward: the per-parameter gradients and the mel's gradient of sum(audio * gy),
recorded on the CPU in fp32 from the reference's own hifigan_infer.hifigan_model.Generator and torch's autograd.

The two small generators of hifigan.npz's configurations (ResBlock1 and ResBlock2, two upsampling stages), with seeded
tests/hifigan_ref.make_state_dict weights calibrated by tests/hifigan_ref.calibrate (neither is stored: the test makes them again
from the seeds below); inputs are (B, T) = (2, 5) and (2, 33), mels hifigan_ref.make_mel, upstream gradients
hifigan_grad_ref.upstream.  Per generator and case the file holds, per tensor of the weight-normed state dict (in the order of
``{tag}_keys``, the mel's gradient last), the recording's max deviation from the fp64 restatement (tests/hifigan_grad_ref.py) and
max |g64|, and the gradients themselves (``{tag}_g{n}/{key}``) of all four runs.  Data only.

Run in the build container only (needs /root/reference); writes hifigan_grad.npz next to this file."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hifigan_grad_ref as GR  # noqa: E402
import hifigan_ref as R  # noqa: E402
from make_golden_hifigan import import_reference  # noqa: E402

CASES = [(2, 5), (2, 33)]
SEEDS = dict(weights=3100, calibrate_mel=3200, mel=3300, upstream=3400)      # + the generator's index, + the case's for mel and upstream


def main():
    ref = import_reference()
    configs = json.loads(str(np.load(os.path.join(HERE, "hifigan.npz"))["configs"]))
    out = dict(cases=np.array(CASES, dtype=np.int64), seeds=np.array(json.dumps(SEEDS)))
    for gi, (tag, cfg) in enumerate(configs.items()):
        h = R.H(cfg)
        sd = R.calibrate(R.make_state_dict(h, SEEDS["weights"] + gi), h, R.make_mel(2, 16, SEEDS["calibrate_mel"] + gi))
        keys = list(sd)
        out[f"{tag}_keys"] = np.array(json.dumps(keys + ["mel"]))
        for n, (B, T) in enumerate(CASES):
            mel = R.make_mel(B, T, SEEDS["mel"] + 10 * gi + n)
            gen = ref.Generator(h).train()
            gen.load_state_dict(sd)
            assert list(gen.state_dict()) == keys
            m = mel.clone().requires_grad_(True)
            audio = gen(m)
            gy = GR.upstream(B, audio.shape[2], SEEDS["upstream"] + 10 * gi + n)
            (audio * gy).sum().backward()
            got = {k: p.grad.detach() for k, p in gen.named_parameters()}
            assert sorted(got) == sorted(keys)
            got["mel"] = m.grad.detach()
            g64, m64, a64 = GR.grads(sd, h, mel, gy, torch.float64)
            g64 = dict(g64, mel=m64)
            dev, mag = [], []
            for k in keys + ["mel"]:
                assert got[k].shape == g64[k].shape
                out[f"{tag}_g{n}/{k}"] = got[k].numpy()
                dev.append(float((got[k].double() - g64[k]).abs().max()))
                mag.append(float(g64[k].abs().max()))
                assert mag[-1] > 0, (tag, n, k)
            out[f"{tag}_dev{n}"], out[f"{tag}_mag{n}"] = np.array(dev), np.array(mag)
            rel = [d / (2.0 ** -23 * m_) for d, m_ in zip(dev, mag)]
            print(tag, (B, T), len(keys), "tensors, audio fp32 vs fp64", float((audio.detach().double() - a64).abs().max()), "min max|g64|", min(mag),
                  "fp32 deviation in units of 2^-23 max|g64|:", min(rel), "..", max(rel))
    path = os.path.join(HERE, "hifigan_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
