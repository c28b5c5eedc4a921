"""CPU-only checks around WaveGlow's forward direction (audio -> z, log_s, log det W, loss): the fp64 restatement
(tests/waveglow_fwd_ref.py) against the vectors recorded from the reference, WaveGlowLoss on the recorded tuples, what
t2_waveglow_forward_plan returns and refuses, and the cache of packed weights staying out of a pickle."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import waveglow_fwd_ref as FR
import waveglow_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FULL = dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2, WN_config=dict(n_layers=8, n_channels=256, kernel_size=3))
CASES = [(1, 1, 8), (2, 4, 1024), (2, 4, 1500), (3, 2, 1027), (1, 5, 1021), (1, 1, 1024)]


@pytest.fixture(scope="module")
def gold():
    """The forward recording; ``base`` holds waveglow.npz (the models' state dicts and configurations), ``configs`` its configs."""
    z, base = np.load(os.path.join(GOLDEN, "waveglow_forward.npz")), np.load(os.path.join(GOLDEN, "waveglow.npz"))
    out = {k: z[k] for k in z.files}
    out["base"], out["configs"] = {k: base[k] for k in base.files}, base["configs"]
    return out


def load_sd(gold, tag):
    """The recorded model with the skewed mixes of the forward recording."""
    base = gold["base"]
    sd = {k: torch.from_numpy(base[k if k.startswith("upsample.") else f"{tag}/{k}"]) for k in json.loads(str(base[f"{tag}_keys"]))}
    for k in sd:
        if k.startswith("convinv."):
            sd[k] = torch.from_numpy(gold[f"{tag}/{k}"])
    return sd


def recorded(gold, tag, n):
    cfg = json.loads(str(gold["configs"]))[tag]
    z = torch.from_numpy(gold[f"{tag}_z{n}"])
    log_s = [torch.from_numpy(gold[f"{tag}_log_s{n}_{k}"]) for k in range(cfg["n_flows"])]
    return z, log_s, torch.from_numpy(gold[f"{tag}_logdet{n}"])


def test_the_recording_holds_the_cases_of_the_issue(gold):
    assert [tuple(int(v) for v in c) for c in gold["cases"]] == CASES and list(gold["sigmas"]) == [1.0, 0.7]


@pytest.mark.parametrize("tag", ["a", "deep"])
def test_restatement_matches_the_recording(gold, tag):
    cfg, folded = json.loads(str(gold["configs"]))[tag], R.fold(load_sd(gold, tag))
    for n, (B, T, N) in enumerate(CASES):
        mel, audio = torch.from_numpy(gold[f"mel{n}"]), torch.from_numpy(gold[f"audio{n}"])
        assert mel.shape == (B, 8, T) and audio.shape == (B, N)
        z, log_s, logdet = recorded(gold, tag, n)
        L = N // cfg["n_group"]
        z64, s64, ld64 = FR.forward(folded, cfg, mel, audio)
        zerr, zbound = float((z.double() - z64).abs().max()), 25 * float(gold[f"{tag}_z_err{n}"])
        serr = [float((a.double() - b).abs().max()) for a, b in zip(log_s, s64)]
        sbound = [25 * float(v) for v in gold[f"{tag}_log_s_err{n}"]]
        print(tag, (B, T, N), "z err", zerr, "bound", zbound, "log_s err", serr, "bound", sbound)
        assert z.shape == (B, cfg["n_group"], L) and [t.shape[1] for t in log_s] == [c // 2 for c in R.flow_channels(cfg)]
        assert zerr <= zbound and all(e <= b for e, b in zip(serr, sbound))
        assert 0.1 <= max(float(t.abs().max()) for t in log_s) <= 1.0             # the recording pins something
        # torch.logdet in fp32 is an fp32 LU: with c <= 8 and a condition of at most 4 its error on log|det| stays below
        # c * cond * 2^-23 = 4e-6, whatever the size of the logarithm itself; the recording holds B * L times that
        ref = B * L * ld64
        assert float(ld64.abs().max()) > 0.3 and bool(((logdet.double() - ref).abs() <= B * L * 4e-6 + 1e-6 * ref.abs()).all())
        for si, sigma in enumerate(gold["sigmas"]):
            err = abs(float(gold[f"{tag}_loss{n}"][si]) - float(FR.loss(z64, s64, ld64, float(sigma))))
            assert err <= 25 * max(float(gold[f"{tag}_loss_err{n}"][si]), 2.0 ** -23 * FR.loss_magnitude(z64, s64, ld64, float(sigma)))
        # the per-item values average to the loss
        items = FR.nll_items(z64, s64, ld64, 0.7)
        assert items.shape == (B,) and abs(float(items.mean()) - float(FR.loss(z64, s64, ld64, 0.7))) < 1e-12


@pytest.mark.parametrize("tag", ["a", "deep"])
def test_waveglow_loss_on_the_recorded_tuples(gold, tag):
    from tacotron2_subword_amd.waveglow import glow
    for n in range(len(CASES)):
        z, log_s, logdet = recorded(gold, tag, n)
        before = logdet.clone()
        for si, sigma in enumerate(gold["sigmas"]):
            loss = glow.WaveGlowLoss(float(sigma))((z, log_s, list(logdet.unbind(0))))
            ref = float(gold[f"{tag}_loss{n}"][si])
            ld = torch.from_numpy(gold[f"{tag}_logdet{n}"]).double() / (z.shape[0] * z.shape[2])
            assert loss.dim() == 0 and loss.dtype == torch.float32
            assert abs(float(loss) - ref) <= 4 * 2.0 ** -23 * FR.loss_magnitude(z, log_s, ld, float(sigma)), (tag, n, si, float(loss), ref)
        assert torch.equal(logdet, before)                                          # the tuple is left as it was


def _plan(cfg, B, T, N):
    from tacotron2_subword_amd import _lib as L
    return L.waveglow_forward_plan(L.waveglow_config(**cfg), B, T, N)


def test_plan_returns_the_sizes(gold):
    for cfg in json.loads(str(gold["configs"])).values():
        for B, T, N in CASES:
            p = _plan(cfg, B, T, N)
            L = N // 8
            assert (p.L, p.n_log_s_rows, p.n_blocks, p.n_partials) == (L, 14, (L + 255) // 256, 2 * 4 * B * ((L + 255) // 256))
            floats = B * L * (64 + 3 * cfg["WN_config"]["n_channels"] + 16)
            assert p.workspace_bytes >= floats * 4 + (p.n_partials + B * 6) * 8
    p = _plan(FULL, 12, 63, 16000)                                                  # the reference's training shape
    assert (p.L, p.n_log_s_rows, p.n_blocks, p.n_partials, p.n_tensors) == (2000, 4 * 4 + 4 * 3 + 4 * 2, 8, 2 * 12 * 12 * 8, 2 + 12 * (7 + 4 * 8))
    p = _plan(FULL, 1, 775, 775 * 256)
    assert (p.L, p.n_blocks) == (775 * 32, 97)
    from tacotron2_subword_amd import _lib as L
    assert p.packed_bytes == L.waveglow_plan(L.waveglow_config(**FULL), 1, 775).packed_bytes
    assert _plan(FULL, 1, 1, 1024).L == 128 and _plan(FULL, 65535, 1, 8).L == 1


@pytest.mark.parametrize("change, B, T, N, needles", [
    (dict(), 1, 4, 7, ["n_samples=7", "n_group=8"]),
    (dict(n_group=4, n_early_size=0), 1, 4, 3, ["n_samples=3", "n_group=4"]),
    (dict(), 1, 4, 3 * 256 + 1025, ["n_samples=1793", "1792"]),
    (dict(), 2, 1, 1025, ["n_samples=1025", "1024"]),
    (dict(), 0, 4, 1024, ["B=0"]),
    (dict(), 65536, 4, 1024, ["B=65536"]),
    (dict(), 1, 0, 8, ["T=0"]),
    (dict(WN_config=dict(n_layers=9, n_channels=256, kernel_size=3)), 1, 4, 1024, ["n_layers=9"]),
])
def test_plan_refuses_with_the_value(change, B, T, N, needles):
    with pytest.raises(RuntimeError) as e:
        _plan(dict(FULL, **change), B, T, N)
    assert all(n in str(e.value) for n in needles), str(e.value)


def test_pickled_module_does_not_carry_the_caches(gold, tmp_path):
    from tacotron2_subword_amd.waveglow import glow
    cfg = json.loads(str(gold["configs"]))["a"]
    model = glow.WaveGlow(**cfg)
    model.load_state_dict(load_sd(gold, "a"))
    stale = dict(_packed=torch.zeros(3), _packed_key=1, _packed_fwd=torch.zeros(5), _packed_fwd_key=2, _logdet_fwd=torch.zeros(4))
    assert set(stale) == set(glow._CACHES)

    def plant():
        for k, v in stale.items():
            setattr(model, k, v)

    plant()
    assert not any(k in pickle.loads(pickle.dumps(model)).__dict__ for k in stale)
    path = str(tmp_path / "waveglow.pt")
    torch.save({"model": model}, path)
    loaded = torch.load(path, weights_only=False)["model"]
    assert all(getattr(loaded, k, None) is None for k in stale)
    assert all(torch.equal(a, b) for a, b in zip(loaded._tensors(True), model._tensors(True)))
    # every way the parameters change drops them
    for change in (lambda: model.load_state_dict(load_sd(gold, "a")), lambda: model.float(), lambda: glow.WaveGlow.remove_weightnorm(model)):
        plant()
        change()
        assert all(getattr(model, k, None) is None for k in stale)
    # the forward table holds W_k where inference's holds its inverse, and nothing else differs
    inv, fwd = model._tensors(), model._tensors(forward=True)
    differ = [i for i, (a, b) in enumerate(zip(inv, fwd)) if not torch.equal(a, b)]
    per = 7 + 4 * cfg["WN_config"]["n_layers"]
    assert len(inv) == len(fwd) and differ == [2 + per * (k + 1) - 1 for k in range(cfg["n_flows"])]
    for k, i in enumerate(differ):
        assert torch.equal(fwd[i], model.convinv[k].conv.weight.detach().squeeze(-1))


def test_loss_class_is_reachable_as_the_reference_names_it():
    from tacotron2_subword_amd.waveglow import glow
    assert glow.WaveGlowLoss().sigma == 1.0 and glow.WaveGlowLoss(0.7).sigma == 0.7
