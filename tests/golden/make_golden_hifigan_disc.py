#!/usr/bin/env python3
"""Golden vectors for the HiFi-GAN multi-period discriminator: feature maps, scores and gradients recorded on the CPU in fp32 from
the reference's own hifigan_infer.hifigan_model.MultiPeriodDiscriminator and torch's autograd.

Weights (tests/hifigan_disc_ref.make_state_dict), audio (make_clean_audio) and upstream gradients (make_upstream) are made again
from the seeds below, not stored.  The scalar differentiated is sum over the five discriminators of weighted_sum on the real and on
the generated side: a random weight on every feature map and on the score.  Per case n the file holds
  keys                   the 90 parameter keys in state-dict order, then "y" and "y_hat"
  dev{n}, mag{n}         per gradient tensor, over every element: the recording's max deviation from the fp64 restatement
                         (tests/hifigan_disc_ref.py) and max |g64|
  g{n}/{key}             the recorded gradient, flattened, every GRAD_STRIDE-th element
  fdev{n}, fmag{n}       the same two figures per forward tensor, in the order discriminator, (real, generated), the six maps
  f{n}/{d}/{r|g}/{l}     the recorded feature map, flattened, at a stride that leaves at most FMAP_KEEP elements (the score, l = 5, whole)
Data only.  Run in the build container only (needs /root/reference); writes hifigan_disc.npz next to this file."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hifigan_disc_ref as R  # noqa: E402
from make_golden_hifigan import import_reference  # noqa: E402

CASES = [(1, 2051), (2, 700)]      # small enough that make_clean_audio finds its seeds in under a minute
SEEDS = dict(weights=5100, y=5200, y_hat=5300, upstream=5400)       # + the case's index; upstream + 10 * discriminator (+ 5 generated)
GRAD_STRIDE = 997
FMAP_KEEP = 512


def fmap_stride(t):
    return max(1, -(-t.numel() // FMAP_KEEP))


def main():
    ref = import_reference()
    sd = R.make_state_dict(SEEDS["weights"])
    keys = list(sd)
    out = dict(cases=np.array(CASES, dtype=np.int64), seeds=np.array(json.dumps(SEEDS)), keys=np.array(json.dumps(keys + ["y", "y_hat"])),
               grad_stride=np.array(GRAD_STRIDE), fmap_keep=np.array(FMAP_KEEP))
    for n in range(len(CASES)):
        y, y_hat, ups = R.mpd_inputs(sd, SEEDS, n, *CASES[n])
        mpd = ref.MultiPeriodDiscriminator().train()
        mpd.load_state_dict(sd)
        assert list(mpd.state_dict()) == keys
        yl, hl = y.clone().requires_grad_(True), y_hat.clone().requires_grad_(True)
        outs = mpd(yl, hl)
        R.mpd_total(outs, ups).backward()
        got = {k: p.grad.detach() for k, p in mpd.named_parameters()}
        got["y"], got["y_hat"] = yl.grad.detach(), hl.grad.detach()
        g64, _, o64 = R.autograd(sd, y, y_hat, torch.float64, lambda o: R.mpd_total(o, ups))
        dev, mag = [], []
        for k in keys + ["y", "y_hat"]:
            assert got[k].shape == g64[k].shape
            out[f"g{n}/{k}"] = got[k].flatten()[::GRAD_STRIDE].numpy()
            dev.append(float((got[k].double() - g64[k]).abs().max()))
            mag.append(float(g64[k].abs().max()))
            assert mag[-1] > 0, (n, k)
        out[f"dev{n}"], out[f"mag{n}"] = np.array(dev), np.array(mag)
        fdev, fmag = [], []
        for d in range(len(R.PERIODS)):
            for side, fm, f64 in (("r", outs[2][d], o64[2][d]), ("g", outs[3][d], o64[3][d])):
                for l, (a, b) in enumerate(zip(fm, f64)):
                    a = a.detach()
                    out[f"f{n}/{d}/{side}/{l}"] = (a.flatten() if l == 5 else a.flatten()[::fmap_stride(a)]).numpy()
                    fdev.append(float((a.double() - b).abs().max()))
                    fmag.append(float(b.abs().max()))
        out[f"fdev{n}"], out[f"fmag{n}"] = np.array(fdev), np.array(fmag)
        print("case", n, CASES[n], "worst gradient dev / mag", max(a / b for a, b in zip(dev, mag)), "worst forward dev", max(fdev))
    path = os.path.join(HERE, "hifigan_disc.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
