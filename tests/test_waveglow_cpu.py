"""CPU-only checks around WaveGlow: the fp64 restatement (tests/waveglow_ref.py) against the vectors recorded from the
reference, the module's parameter names and folding, what t2_waveglow_plan accepts and refuses, and a pickled module under
the reference's module name ``glow``."""
import ctypes as C
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import waveglow_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "waveglow.npz"))
    return {k: z[k] for k in z.files}


def load_sd(gold, tag):
    keys = json.loads(str(gold[f"{tag}_keys"]))
    return {k: torch.from_numpy(gold[k if k.startswith("upsample.") else f"{tag}/{k}"]) for k in keys}


def load_case(gold, n):
    B, T = (int(v) for v in gold["cases"][n])
    mel = torch.from_numpy(gold[f"mel{n}"])
    noise = [torch.from_numpy(gold[f"noise{n}_{j}"]) for j in range(sum(k.startswith(f"noise{n}_") for k in gold))]
    return B, T, mel, noise


def configs(gold):
    return json.loads(str(gold["configs"]))


@pytest.mark.parametrize("tag", ["a", "deep"])
def test_restatement_matches_the_recording(gold, tag):
    cfg, folded = configs(gold)[tag], R.fold(load_sd(gold, tag))
    for n in range(len(gold["cases"])):
        B, T, mel, noise = load_case(gold, n)
        assert [tuple(z.shape) for z in noise] == R.noise_shapes(cfg, B, T)
        for si, sigma in enumerate(gold["sigmas"]):
            d = {}
            a64 = R.infer(folded, cfg, mel, noise, float(sigma), details=d)
            ref = torch.from_numpy(gold[f"{tag}_audio{n}_s{si}"])
            assert ref.shape == (B, T * 256)
            err, bound = float((ref.double() - a64).abs().max()), 5 * float(gold[f"{tag}_ref_fp32_err{n}_s{si}"])
            serr, sbound = float((torch.from_numpy(gold[f"spect{n}"]).double() - d["spect"]).abs().max()), 5 * float(gold[f"spect_ref_fp32_err{n}"])
            print(tag, (B, T), float(sigma), "audio err", err, "bound", bound, "spect err", serr, "bound", sbound)
            assert err <= bound and serr <= sbound
            assert float(ref.std()) > 0.05                      # the recording pins something
            # the recorded z is what the reference's forward makes of its own audio: the restatement's forward agrees
            z = R.forward(folded, cfg, mel, ref)
            assert float((z - torch.from_numpy(gold[f"{tag}_z{n}_s{si}"]).double()).abs().max()) <= 1e-5


@pytest.mark.parametrize("tag", ["a", "deep"])
def test_module_state_dict_keys_and_folding(gold, tag):
    from tacotron2_subword_amd.waveglow import glow
    cfg, sd = configs(gold)[tag], load_sd(gold, tag)
    keys = json.loads(str(gold[f"{tag}_keys"]))
    model = glow.WaveGlow(**cfg)
    assert list(model.state_dict()) == keys == R.state_dict_keys(cfg)
    assert all(float(t.abs().max()) == 0.0 for k, t in model.state_dict().items() if ".end." in k)      # glow.py:129-130
    model.load_state_dict(sd)
    assert model.n_remaining_channels == R.flow_channels(cfg)[-1]
    normed = model._tensors()
    glow.WaveGlow.remove_weightnorm(model)
    assert list(model.state_dict()) == R.state_dict_keys(cfg, normed=False)
    folded = R.fold(sd)
    for k, v in model.state_dict().items():
        assert torch.allclose(v, folded[k], rtol=1e-6, atol=1e-8), k
    after = model._tensors()
    assert len(normed) == len(after) == 2 + cfg["n_flows"] * (7 + 4 * cfg["WN_config"]["n_layers"])
    assert all(torch.equal(a, b) for a, b in zip(normed, after))            # folded == weight-normed, bit for bit
    with pytest.raises(ValueError):
        glow.WaveGlow.remove_weightnorm(model)
    with pytest.raises(RuntimeError, match="inference only"):
        model((torch.zeros(1, 8, 1), torch.zeros(1, 256)))


def _plan(cfg, B=1, T=4):
    from tacotron2_subword_amd import _lib as L
    return L.waveglow_plan(L.waveglow_config(**cfg), B, T)


FULL = dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2, WN_config=dict(n_layers=8, n_channels=256, kernel_size=3))


def test_plan_accepts_supported_shapes(gold):
    p = _plan(FULL, 3, 775)
    assert (p.L, p.out_len, p.n_remaining_channels, p.n_noise_planes, p.time_tile) == (775 * 32, 775 * 256, 4, 3, 128)
    assert p.n_tensors == 2 + 12 * (7 + 4 * 8)
    assert p.workspace_bytes >= 3 * 775 * 32 * (640 + 3 * 256 + 16) * 4
    for cfg in configs(gold).values():
        p = _plan(cfg, 2, 5)
        assert (p.L, p.out_len, p.n_remaining_channels, p.n_noise_planes) == (160, 1280, 6, 2)
    _plan(dict(FULL, WN_config=dict(n_layers=1, n_channels=512, kernel_size=3)))
    _plan(dict(FULL, n_group=2, n_early_size=0, n_mel_channels=4))
    assert _plan(dict(FULL, n_group=4, n_early_size=2, n_early_every=6), 65535, 1).L == 64


def wn(**k):
    return dict(FULL["WN_config"], **k)


@pytest.mark.parametrize("change, B, T, needle", [
    (dict(WN_config=wn(kernel_size=5)), 1, 4, "kernel_size=5"),
    (dict(WN_config=wn(n_layers=9)), 1, 4, "n_layers=9"),
    (dict(WN_config=wn(n_layers=0)), 1, 4, "n_layers=0"),
    (dict(WN_config=wn(n_channels=12)), 1, 4, "n_channels=12"),
    (dict(WN_config=wn(n_channels=520)), 1, 4, "n_channels=520"),
    (dict(n_group=10), 1, 4, "n_group=10"),
    (dict(n_group=3), 1, 4, "n_group=3"),
    (dict(n_early_size=1), 1, 4, "n_early_size=1"),
    (dict(n_mel_channels=3, n_group=2), 1, 4, "= 6 is not a multiple of 8"),
    (dict(n_early_every=0), 1, 4, "n_early_every=0"),
    (dict(n_early_size=4, n_early_every=2), 1, 4, "n_early_size=4"),        # runs out of channels
    (dict(), 65536, 4, "B=65536"),
    (dict(), 0, 4, "B=0"),
    (dict(), 1, 0, "T=0"),
])
def test_plan_refuses_with_the_value(change, B, T, needle):
    with pytest.raises(RuntimeError) as e:
        _plan(dict(FULL, **change), B, T)
    assert needle in str(e.value), str(e.value)


def test_constructor_refuses_what_the_plan_refuses():
    from tacotron2_subword_amd.waveglow import glow
    with pytest.raises(RuntimeError, match="n_channels=12"):
        glow.WaveGlow(**dict(FULL, n_mel_channels=8, WN_config=wn(n_channels=12)))


def test_pickled_module_loads_under_the_glow_alias(gold, tmp_path, monkeypatch):
    """The published checkpoint is a pickled module whose classes live in a top-level ``glow``.  No such checkpoint is at hand,
    so the stand-in is a pickle of this package's own classes written under that module name."""
    from tacotron2_subword_amd.waveglow import glow
    cfg, sd = configs(gold)["a"], load_sd(gold, "a")
    model = glow.WaveGlow(**cfg)
    model.load_state_dict(sd)
    model._packed = torch.zeros(3)                                            # a stale cache must not travel
    monkeypatch.setitem(sys.modules, "glow", glow)
    for cls in (glow.WaveGlow, glow.WN, glow.Invertible1x1Conv, glow._Conv):
        monkeypatch.setattr(cls, "__module__", "glow")
    path = str(tmp_path / "waveglow.pt")
    torch.save({"model": model}, path)
    assert b"glow" in pickle.dumps(model) and b"tacotron2_subword_amd" not in pickle.dumps(model)
    loaded = torch.load(path, weights_only=False)["model"]
    assert isinstance(loaded, glow.WaveGlow) and getattr(loaded, "_packed", None) is None
    assert list(loaded.state_dict()) == list(sd)
    assert all(torch.equal(a, b) for a, b in zip(loaded._tensors(), model._tensors()))
    c = loaded._config()
    assert (c.n_mel_channels, c.n_flows, c.n_layers, c.n_channels, c.kernel_size) == (8, 4, 3, 8, 3)
