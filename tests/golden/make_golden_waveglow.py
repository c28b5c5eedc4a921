#!/usr/bin/env python3
"""Golden vectors for WaveGlow inference, recorded from the reference's own glow.WaveGlow on the CPU: two small models
("a": 3 layers of 8 channels; "deep": 8 layers of 16 channels, dilations up to 128; both 4 flows, n_group 8, an early output
of 2 channels every 2 flows, 8 mel channels -- at 80 the upsampling weight alone is 26 MB), each with its weight-normed state
dict (the tests fold it), and for three (B, T) cases at sigma = 0.666 and sigma = 0 the mel, the noise planes, the reference's
fp32 audio, the upsampled and regrouped mel (`spect`), the z that the reference's forward returns for that audio, and the
reference's own fp32 deviation from the fp64 restatement (tests/waveglow_ref.py) on the audio and on `spect`.

The reference's infer allocates its noise as torch.cuda.FloatTensor(...).normal_(); a stand-in on torch.cuda.FloatTensor hands
out seeded CPU draws instead and records them (a harness shim, like the matplotlib one in make_golden_hifigan.py).  The
reference starts `end` at zero, which would pin nothing (s = b = 0): end.weight and end.bias are drawn from N(0, 0.05).

To keep the file under the repository's limit for a committed file, both models share one upsampling layer (so `spect`, the
mels and the noise are stored once per case), and the two large tensors -- upsample.weight and cond_layer.weight_v -- are
rounded to 8 mantissa bits before they are loaded into the reference, so that they compress; products with fp32
activations stay inexact in fp32, which is all the tests need of them.

The script refuses to write unless, for every model, max |s| over the flows lies in [0.1, 1.0], the audio's deviation lies in
[0.05, 5] and the fp64 restatement's forward(infer(noise)) returns the noise to 1e-10.  Run in the build container only
(needs /root/reference); writes waveglow.npz next to this file."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import waveglow_ref as R  # noqa: E402

BASE = dict(n_mel_channels=8, n_flows=4, n_group=8, n_early_every=2, n_early_size=2)
CONFIGS = {
    "a": dict(BASE, WN_config=dict(n_layers=3, n_channels=8, kernel_size=3)),
    "deep": dict(BASE, WN_config=dict(n_layers=8, n_channels=16, kernel_size=3)),
}
CASES = [(2, 5), (1, 1), (1, 4)]
SIGMAS = [0.666, 0.0]


def round_mantissa(t, bits=8):
    """t with its mantissa rounded to `bits` bits (bf16's grid): still fp32, but the low 16 bits are zero."""
    return t.to(torch.bfloat16).to(torch.float32) if bits == 8 else t


class NoiseStandIn:
    """torch.cuda.FloatTensor(B, C, L).normal_() -> the next prepared plane."""

    def __init__(self):
        self.planes, self.used = [], []

    def __call__(self, *shape):
        stand_in = self

        class _Plane:
            def normal_(self):
                z = stand_in.planes.pop(0)
                assert tuple(z.shape) == tuple(shape), (z.shape, shape)
                stand_in.used.append(z)
                return z
        return _Plane()


def main():
    sys.path.insert(0, "/root/reference")
    import glow as ref  # noqa
    stand_in = NoiseStandIn()
    torch.cuda.FloatTensor = stand_in
    out = dict(cases=np.array(CASES, dtype=np.int64), sigmas=np.array(SIGMAS), configs=np.array(json.dumps(CONFIGS)))
    mels = [R.make_mel(B, T, 700 + n, n_mel=BASE["n_mel_channels"]) for n, (B, T) in enumerate(CASES)]
    noises = []
    for n, (B, T) in enumerate(CASES):
        g = torch.Generator().manual_seed(800 + n)
        noises.append([torch.randn(s, generator=g) for s in R.noise_shapes(CONFIGS["a"], B, T)])
        out[f"mel{n}"] = mels[n].numpy()
        for j, z in enumerate(noises[n]):
            out[f"noise{n}_{j}"] = z.numpy()
    upsample = None
    for gi, (tag, cfg) in enumerate(CONFIGS.items()):
        torch.manual_seed(2026 + gi)
        model = ref.WaveGlow(**cfg).eval()
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        g = torch.Generator().manual_seed(90 + gi)
        for k in sd:
            if ".end." in k:
                sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
            if k.endswith("cond_layer.weight_v"):
                sd[k] = round_mantissa(sd[k])
        if upsample is None:
            upsample = {k: round_mantissa(v) if k.endswith("weight") else v for k, v in sd.items() if k.startswith("upsample.")}
        sd.update(upsample)
        model.load_state_dict(sd)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        assert list(sd) == R.state_dict_keys(cfg)
        out[f"{tag}_keys"] = np.array(json.dumps(list(sd)))
        for k, v in sd.items():
            if not (k.startswith("upsample.") and gi > 0):
                out[("" if k.startswith("upsample.") else tag + "/") + k] = v.numpy()
        folded = R.fold(sd)
        spects = []
        model.WN[0].register_forward_pre_hook(lambda mod, inp: spects.append(inp[0][1].detach().clone()))
        s_max = 0.0
        for n, (B, T) in enumerate(CASES):
            for si, sigma in enumerate(SIGMAS):
                stand_in.planes, stand_in.used = [z.clone() for z in noises[n]], []
                del spects[:]
                with torch.no_grad():
                    audio = model.infer(mels[n], sigma=sigma)
                    z = model((mels[n], audio))[0]
                assert not stand_in.planes and all(torch.equal(u, v) for u, v in zip(stand_in.used, noises[n]))
                d = {}
                a64 = R.infer(folded, cfg, mels[n], noises[n], sigma, details=d)
                back = R.planes_from_z(cfg, R.forward(folded, cfg, mels[n], a64))
                inv_err = max(float((p - sigma * z0.double()).abs().max()) for p, z0 in zip(back, noises[n]))
                err, serr = float((audio.double() - a64).abs().max()), float((spects[0].double() - d["spect"]).abs().max())
                s_max = max(s_max, d["s_max"])
                print(tag, "case", (B, T), "sigma", sigma, "audio", tuple(audio.shape), "std", float(audio.std()), "max |s|", d["s_max"],
                      "reference fp32 vs fp64 restatement", err, "on spect", serr, "forward(infer(noise)) - noise", inv_err)
                assert 0.05 <= float(audio.std()) <= 5.0, (tag, n, sigma, float(audio.std()))
                assert inv_err <= 1e-10, (tag, n, sigma, inv_err)
                out[f"{tag}_audio{n}_s{si}"], out[f"{tag}_z{n}_s{si}"] = audio.numpy(), z.numpy()
                out[f"{tag}_ref_fp32_err{n}_s{si}"] = np.array(err)
                if gi == 0 and si == 0:
                    out[f"spect{n}"], out[f"spect_ref_fp32_err{n}"] = spects[0].numpy(), np.array(serr)
                else:
                    assert np.array_equal(out[f"spect{n}"], spects[0].numpy()), "both models share the upsampling layer"
        print(tag, "max |s| over all flows and cases", s_max)
        assert 0.1 <= s_max <= 1.0, (tag, s_max)
    path = os.path.join(HERE, "waveglow.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
