#!/usr/bin/env python3
"""Golden vectors for WaveGlow's forward direction (audio -> z, log_s, log det W, loss), recorded on the CPU from the
reference's own glow.WaveGlow.forward and glow.WaveGlowLoss.

The two models are those of waveglow.npz ("a" and "deep"); their state dicts are read from that file and not stored again,
but for the 1x1 mixes: the recorded ones are orthonormal, so log det W = 0 would pin nothing.  They are replaced by Q * diag(d),
d in [0.5, 2] (waveglow_fwd_ref.skew_mixes), and only those are stored (``{tag}/convinv.k.conv.weight``).

Per case (B, T, N) -- L = 1; N = T*256 with L one 128-column tile; audio that reaches into the trailing samples of the transposed
conv; a dropped tail; L = 127; all 768 trailing samples -- the file holds the mel and the audio (N(0, 0.3)) once, and per model
the reference's fp32 z, every log_s, log_det_W_list, the loss at sigma = 1.0 and 0.7, and the reference's own fp32 deviation
from the fp64 restatement (tests/waveglow_fwd_ref.py) on each of them.

The script refuses to write unless max |log_s| lies in [0.1, 1.0] for every model and case.  Run in the build container only
(needs /root/reference); writes waveglow_forward.npz next to this file."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import waveglow_fwd_ref as FR  # noqa: E402
import waveglow_ref as R  # noqa: E402

CASES = [(1, 1, 8), (2, 4, 1024), (2, 4, 1500), (3, 2, 1027), (1, 5, 1021), (1, 1, 1024)]
SIGMAS = [1.0, 0.7]


def main():
    sys.path.insert(0, "/root/reference")
    import glow as ref  # noqa
    base = np.load(os.path.join(HERE, "waveglow.npz"))
    configs = json.loads(str(base["configs"]))
    out = dict(cases=np.array(CASES, dtype=np.int64), sigmas=np.array(SIGMAS))
    inputs = []
    for n, (B, T, N) in enumerate(CASES):
        mel = R.make_mel(B, T, 900 + n, n_mel=8)
        audio = torch.randn(B, N, generator=torch.Generator().manual_seed(950 + n)) * 0.3
        inputs.append((mel, audio))
        out[f"mel{n}"], out[f"audio{n}"] = mel.numpy(), audio.numpy()
    for gi, (tag, cfg) in enumerate(configs.items()):
        keys = json.loads(str(base[f"{tag}_keys"]))
        sd = {k: torch.from_numpy(base[k if k.startswith("upsample.") else f"{tag}/{k}"]) for k in keys}
        sd = FR.skew_mixes(sd, cfg, 60 + gi)
        model = ref.WaveGlow(**cfg).eval()
        model.load_state_dict(sd)
        folded = R.fold(sd)
        for k in range(cfg["n_flows"]):
            W = sd[f"convinv.{k}.conv.weight"]
            assert float(torch.det(W.squeeze(-1).double())) > 0
            out[f"{tag}/convinv.{k}.conv.weight"] = W.numpy()
        for n, (B, T, N) in enumerate(CASES):
            mel, audio = inputs[n]
            with torch.no_grad():
                z, log_s, logdet = model((mel, audio))
                logdet = [t.clone() for t in logdet]                # the reference's loss adds into log_det_W_list[0] in place
                losses = [ref.WaveGlowLoss(s)((z, log_s, [t.clone() for t in logdet])) for s in SIGMAS]
            L = N // cfg["n_group"]
            z64, s64, ld64 = FR.forward(folded, cfg, mel, audio)
            assert z.shape == (B, cfg["n_group"], L) == z64.shape
            s_max = max(float(t.abs().max()) for t in s64)
            assert 0.1 <= s_max <= 1.0, (tag, n, s_max)
            out[f"{tag}_z{n}"], out[f"{tag}_z_err{n}"] = z.numpy(), np.array(float((z.double() - z64).abs().max()))
            for k, (a, b) in enumerate(zip(log_s, s64)):
                assert a.shape == b.shape == (B, R.flow_channels(cfg)[k] // 2, L)
                out[f"{tag}_log_s{n}_{k}"] = a.contiguous().numpy()
            out[f"{tag}_log_s_err{n}"] = np.array([float((a.double() - b).abs().max()) for a, b in zip(log_s, s64)])
            out[f"{tag}_logdet{n}"] = np.array([float(t) for t in logdet], dtype=np.float32)
            assert all(abs(float(t) - B * L * float(d)) <= 1e-5 * abs(B * L * float(d)) + 1e-6 for t, d in zip(logdet, ld64))
            out[f"{tag}_loss{n}"] = np.array([float(v) for v in losses], dtype=np.float32)
            out[f"{tag}_loss_err{n}"] = np.array([abs(float(v) - float(FR.loss(z64, s64, ld64, s))) for v, s in zip(losses, SIGMAS)])
            print(tag, "case", (B, T, N), "L", L, "max |log_s|", s_max, "z std", float(z.std()), "loss", out[f"{tag}_loss{n}"],
                  "reference fp32 vs fp64 restatement: z", float(out[f"{tag}_z_err{n}"]), "log_s", out[f"{tag}_log_s_err{n}"].max(),
                  "loss", out[f"{tag}_loss_err{n}"])
    path = os.path.join(HERE, "waveglow_forward.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
