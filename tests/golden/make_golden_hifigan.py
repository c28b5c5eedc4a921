#!/usr/bin/env python3
"""Golden vectors for the HiFi-GAN generator, recorded from the reference's own hifigan_infer.hifigan_model.Generator: two
small generators (ResBlock1 and ResBlock2, 32 -> 8 channels), each with its weight-normed state dict, the folded one after
remove_weight_norm(), and for three (B, T) cases the mel, conv_post's output before the tanh (forward hook) and the audio.

The reference's initialisation (sigma = 0.01) gives outputs near 0, which would pin nothing, and a uniform gain saturates
the tanh; so biases are drawn from N(0, 0.1) and tests/hifigan_ref.calibrate rescales every layer in execution order
(weight_g and bias together) to unit output deviation, 0.5 and zero mean for conv_post.  The script refuses to write unless, over a
generator's cases together, fewer than 1 % of the samples are saturated (|y| > 0.99) and the pre-tanh deviation lies in
[0.3, 1.5].

The reference's hifigan_utils imports matplotlib for its plotting helper; where that is not installed a stand-in module
lets the import pass (nothing here plots).  Run in the build container only (needs /root/reference); writes hifigan.npz
next to this file."""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hifigan_ref as R  # noqa: E402

CONFIGS = {
    "rb1": dict(resblock="1", upsample_rates=[8, 2], upsample_kernel_sizes=[16, 4], upsample_initial_channel=32,
                resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]]),
    "rb2": dict(resblock="2", upsample_rates=[8, 4], upsample_kernel_sizes=[16, 8], upsample_initial_channel=32,
                resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]]),
}
CASES = [(2, 9), (1, 33), (1, 1)]


def import_reference():
    try:
        importlib.import_module("matplotlib.pylab")
    except ImportError:
        mpl, pylab = types.ModuleType("matplotlib"), types.ModuleType("matplotlib.pylab")
        mpl.use = lambda *a, **k: None
        mpl.pylab = pylab
        sys.modules["matplotlib"], sys.modules["matplotlib.pylab"] = mpl, pylab
    sys.path.insert(0, "/root/reference")
    from hifigan_infer import hifigan_model as ref  # noqa
    return ref


def main():
    ref = import_reference()
    out = dict(cases=np.array(CASES, dtype=np.int64), configs=np.array(json.dumps(CONFIGS)))
    for gi, (tag, cfg) in enumerate(CONFIGS.items()):
        h = R.H(cfg)
        torch.manual_seed(2025 + gi)
        gen = ref.Generator(h).eval()
        sd = {k: v.detach().clone() for k, v in gen.state_dict().items()}
        g = torch.Generator().manual_seed(77 + gi)
        for k in sd:
            if k.endswith(".bias"):
                sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
        sd = R.calibrate(sd, h, R.make_mel(2, 16, 900 + gi))
        gen.load_state_dict(sd)
        normed = {k: v.detach().clone() for k, v in gen.state_dict().items()}
        pre = []
        gen.conv_post.register_forward_hook(lambda mod, inp, res: pre.append(res.detach().clone()))
        with torch.no_grad():
            audio_normed = gen(R.make_mel(2, 9, 500))
        gen.remove_weight_norm()
        folded = {k: v.detach().clone() for k, v in gen.state_dict().items()}
        out[f"{tag}_normed_keys"], out[f"{tag}_folded_keys"] = np.array(json.dumps(list(normed))), np.array(json.dumps(list(folded)))
        for k, v in normed.items():
            out[f"{tag}_normed/{k}"] = v.numpy()
        for k, v in folded.items():
            out[f"{tag}_folded/{k}"] = v.numpy()
        pooled = []
        for n, (B, T) in enumerate(CASES):
            mel = R.make_mel(B, T, 500 + n)
            del pre[:]
            with torch.no_grad():
                audio = gen(mel)
            if n == 0:
                assert torch.allclose(audio, audio_normed, atol=1e-6), "the reference disagrees with itself across remove_weight_norm"
            sat, std = float((audio.abs() > 0.99).float().mean()), float(pre[0].std())
            a64, _ = R.generator_forward(folded, h, mel)
            print(tag, "case", (B, T), "audio", tuple(audio.shape), "saturated", sat, "pre-tanh std", std, "|max|", float(pre[0].abs().max()),
                  "reference fp32 vs fp64 restatement", float((audio.double() - a64).abs().max()))
            pooled.append(pre[0].flatten())
            out[f"{tag}_mel{n}"], out[f"{tag}_pre{n}"], out[f"{tag}_audio{n}"] = mel.numpy(), pre[0].numpy(), audio.numpy()
        # over the generator's cases together: the single-frame case alone is 16 or 32 samples, not a distribution
        pooled = torch.cat(pooled)
        sat, std = float((torch.tanh(pooled).abs() > 0.99).float().mean()), float(pooled.std())
        print(tag, "all cases: saturated", sat, "pre-tanh std", std)
        assert sat < 0.01 and 0.3 <= std <= 1.5, (tag, sat, std)
    path = os.path.join(HERE, "hifigan.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
