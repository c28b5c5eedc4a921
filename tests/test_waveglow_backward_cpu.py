"""CPU-only checks of WaveGlow's training direction: the differentiable fp64 restatement (tests/waveglow_grad_ref.py) against the
gradients recorded from the reference's own forward and torch's autograd (tests/golden/waveglow_grad.npz), the pure-host plan of
the backward (t2_waveglow_backward_plan) at the training shape of waveglow/config.json, and the surface without a GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import waveglow_grad_ref as GR
import waveglow_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FULL = dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2, WN_config=dict(n_layers=8, n_channels=256, kernel_size=3))
SMALL = dict(n_mel_channels=8, n_flows=2, n_group=8, n_early_every=1, n_early_size=2, WN_config=dict(n_layers=2, n_channels=8, kernel_size=3))


def _L():
    from tacotron2_subword_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def gold():
    z, fwd, base = (np.load(os.path.join(GOLDEN, f)) for f in ("waveglow_grad.npz", "waveglow_forward.npz", "waveglow.npz"))
    out = {k: z[k] for k in z.files}
    out["fwd"], out["base"], out["configs"] = {k: fwd[k] for k in fwd.files}, {k: base[k] for k in base.files}, json.loads(str(base["configs"]))
    return out


@pytest.mark.parametrize("tag", ["a", "deep"])
def test_restatement_agrees_with_the_recording(gold, tag):
    """fp64 autograd through the restatement against the reference's fp32 gradients: within the recorded deviation of every tensor
    (the recording's own fp32 error), on the case whose gradients are stored; the recorded max |g64| is met on both cases."""
    base, fwd, cfg = gold["base"], gold["fwd"], gold["configs"][tag]
    keys = json.loads(str(gold[f"{tag}_keys"]))
    sd = {k: torch.from_numpy(base[k if k.startswith("upsample.") else f"{tag}/{k}"]) for k in keys}
    sd = {k: torch.from_numpy(fwd[f"{tag}/{k}"]) if k.startswith("convinv.") else v for k, v in sd.items()}
    stored, stride = json.loads(str(gold["stored"]))[tag], int(gold["up_stride"])
    assert [tuple(int(v) for v in c) for c in gold["cases"]] == [(2, 4, 1024), (3, 2, 1027)]
    for n in range(2):
        fc = int(gold["forward_case"][n])
        mel, audio = torch.from_numpy(fwd[f"mel{fc}"]), torch.from_numpy(fwd[f"audio{fc}"])
        g64, loss64, _ = GR.grads(sd, cfg, mel, audio, torch.float64, sigma=float(gold["sigma"]))
        assert abs(loss64 - float(gold[f"{tag}_loss{n}"][1])) <= 1e-12 * abs(loss64)
        for i, k in enumerate(keys):
            mag = float(g64[k].abs().max())
            assert mag > 0 and abs(mag - float(gold[f"{tag}_mag{n}"][i])) <= 1e-9 * mag, k
            if n == stored:
                rec, got = torch.from_numpy(gold[f"{tag}_g{n}/{k}"]).double(), g64[k]
                got = got.flatten()[::stride] if k == "upsample.weight" else got
                assert rec.shape == got.shape
                # the fp64 run itself moves in its last bits with the host's thread count: 2^-52 times a few thousand terms
                assert float((rec - got).abs().max()) <= float(gold[f"{tag}_dev{n}"][i]) + 1e-12 * mag, k


def test_backward_plan_at_the_training_shape():
    L = _L()
    cfg = L.waveglow_config(**FULL)
    B, T, N = 12, 63, 16000
    plan, fplan = L.waveglow_backward_plan(cfg, B, T, N), L.waveglow_forward_plan(cfg, B, T, N)
    cols, nc, nl = N // 8, 256, 8
    assert plan.L == cols == fplan.L == 2000
    per = (B * cols + 3) // 4 * 4
    # spect once; per flow the mixed audio_in and out; per flow and layer x_i, tanh(u_a), sigmoid(u_b)
    assert plan.saved_bytes == 4 * per * (80 * 8 + sum(c + nc * (1 + 3 * nl) for c in R.flow_channels(FULL)))
    assert abs(plan.saved_bytes - (3 * B * nc * cols * 4 * 96 + 0.4e9)) < 0.1e9             # 3 * 24.6 MB * 96 = 7.1 GB, plus about 0.4 GB
    sd = R.fold(R.make_state_dict(dict(FULL, WN_config=dict(FULL["WN_config"], n_channels=8)), 1))
    n_tensors = 2 + 12 * (7 + 4 * nl)
    assert plan.n_tensors == fplan.n_tensors == n_tensors == len(sd)
    n_cond, count = 640, 80 * 80 * 1024 + 80
    for c in R.flow_channels(FULL):
        count += nc * (c // 2) + nc + 2 * nc * nl * n_cond + 2 * nc * nl + nl * (2 * nc * nc * 3 + 2 * nc) + (nl - 1) * (2 * nc * nc + 2 * nc) + nc * nc + nc
        count += c * nc + c + c * c
    assert plan.grad_floats == count
    offs = L.waveglow_grad_offsets(cfg, n_tensors)
    assert offs[0] == 0 and offs[1] == 80 * 80 * 1024 and offs[2] == offs[1] + 80 and sorted(offs) == offs and offs[-1] + 4 * 4 == count
    assert plan.packed_bwd_bytes > 0 and plan.workspace_bytes > 0 and plan.n_slots == B * 8 * 4


def test_grad_floats_is_the_parameter_count_of_the_folded_model():
    L = _L()
    for cfg in (SMALL, dict(SMALL, n_flows=5, n_early_every=2, WN_config=dict(n_layers=3, n_channels=24, kernel_size=3))):
        folded = R.fold(R.make_state_dict(cfg, 3))
        plan = L.waveglow_backward_plan(L.waveglow_config(**cfg), 2, 3, 700)
        assert plan.grad_floats == sum(t.numel() for t in folded.values())


def test_backward_plan_refuses_what_the_forward_plan_refuses():
    L = _L()
    cfg = L.waveglow_config(**SMALL)
    for args, needle in (((0, 2, 512), "B=0"), ((1, 0, 512), "T=0"), ((1, 2, 7), "n_samples=7"), ((1, 2, 1281), "n_samples=1281")):
        for plan in (L.waveglow_backward_plan, L.waveglow_forward_plan):
            with pytest.raises(RuntimeError, match=needle):
                plan(cfg, *args)
    bad = L.waveglow_config(**dict(SMALL, WN_config=dict(n_layers=9, n_channels=8, kernel_size=3)))
    info = L.WaveglowBackwardInfo()
    assert L.lib().t2_waveglow_backward_plan(C.byref(bad), 1, 2, 512, C.byref(info)) != 0
    assert "n_layers=9" in L.lib().t2_last_error().decode()
    offs = (C.c_size_t * 3)()
    assert L.lib().t2_waveglow_grad_offsets(C.byref(cfg), offs, 3) != 0 and "3 tensors" in L.lib().t2_last_error().decode()


def test_surface_on_the_cpu():
    from tacotron2_subword_amd.waveglow import glow
    model = glow.WaveGlow(**SMALL)
    mel, audio = R.make_mel(1, 2, 1, n_mel=8), torch.zeros(1, 512)
    with pytest.raises(RuntimeError, match="inference only"):
        model((mel, audio))
    assert not getattr(model, "_trainable", False)
    assert model.trainable() is model and model._trainable is True
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        model((mel, audio))
    assert model.trainable(False) is model
    with pytest.raises(RuntimeError, match="inference only"):
        model((mel, audio))
