"""CPU-only checks of the HiFi-GAN vocoder: the test restatement against the vectors recorded from the reference's
Generator, the checkpoint contract of the package's Generator (keys, shapes, folded weights), the host-side plan query
and its refusals, and the absence of a CPU path."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import hifigan_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ["rb1", "rb2"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "hifigan.npz"))


def _config(gold, tag):
    return R.H(json.loads(str(gold["configs"]))[tag])


def _sd(gold, tag, state):
    return {k: torch.from_numpy(gold[f"{tag}_{state}/{k}"]) for k in json.loads(str(gold[f"{tag}_{state}_keys"]))}


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_the_reference_recording(gold, tag):
    h, folded = _config(gold, tag), _sd(gold, tag, "folded")
    for n, (B, T) in enumerate(gold["cases"]):
        mel = torch.from_numpy(gold[f"{tag}_mel{n}"])
        assert mel.shape == (B, 80, T)
        for dtype in (torch.float64, torch.float32):
            audio, pre = R.generator_forward(folded, h, mel, dtype)
            ea = float((audio.double() - torch.from_numpy(gold[f"{tag}_audio{n}"]).double()).abs().max())
            ep = float((pre.double() - torch.from_numpy(gold[f"{tag}_pre{n}"]).double()).abs().max())
            print(tag, (int(B), int(T)), dtype, "audio", ea, "pre-tanh", ep)
            assert ea < 2e-5 and ep < 2e-5
    # the fold of the restatement is the reference's
    refold = R.fold(_sd(gold, tag, "normed"))
    for k, v in folded.items():
        torch.testing.assert_close(refold[k], v, rtol=1e-6, atol=0)


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_keys_and_shapes_in_both_weight_norm_states(gold, tag):
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import Generator
    gen = Generator(_config(gold, tag))
    normed, folded = _sd(gold, tag, "normed"), _sd(gold, tag, "folded")
    sd = gen.state_dict()
    assert list(sd) == list(normed)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in normed.values()]
    gen.load_state_dict(normed)
    gen.eval()
    gen.remove_weight_norm()
    sd = gen.state_dict()
    assert list(sd) == list(folded)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in folded.values()]
    for k, v in folded.items():
        torch.testing.assert_close(sd[k], v, rtol=1e-6, atol=0)
    gen.load_state_dict(folded)                      # a checkpoint saved after remove_weight_norm loads too
    with pytest.raises(ValueError):
        gen.remove_weight_norm()                     # as torch: nothing left to remove


def test_utils_surface():
    from tacotron2_subword_amd.hifigan_infer import hifigan_utils as U
    from tacotron2_subword_amd import hifigan_infer
    h = U.AttrDict({"resblock": "1", "upsample_rates": [8]})
    assert h.resblock == "1" and h["upsample_rates"] == [8]
    assert [U.get_padding(k, d) for k, d in ((3, 1), (7, 12), (11, 5))] == [1, 36, 25]
    assert callable(U.load_checkpoint) and hifigan_infer.Generator is not None
    assert not hasattr(U, "plt")


def _v1():
    return R.load_config(os.path.join(GOLDEN, "hifigan_config_v1.json"))


def test_plan_query_without_gpu():
    from tacotron2_subword_amd import _lib as L
    for v, rate in ((1, 256), (2, 256), (3, 256)):
        cfg = L.hifigan_config(R.load_config(os.path.join(GOLDEN, f"hifigan_config_v{v}.json")))
        plan = L.hifigan_plan(cfg, 1, 6000)
        assert plan.out_len == 6000 * rate
        assert plan.n_layers == len(R.layer_names(R.load_config(os.path.join(GOLDEN, f"hifigan_config_v{v}.json"))))
        assert plan.time_tile == L.VOCODER_TIME_TILE
        assert 0 < plan.workspace_bytes < 4 << 30 and plan.packed_bytes > 0
    plan = L.hifigan_plan(L.hifigan_config(_v1()), 3, 7)
    assert plan.out_len == 7 * 256


@pytest.mark.parametrize("change,needle", [
    (dict(upsample_initial_channel=72), b"72"),                                  # 72 / 16 = 4.5 channels at the end
    (dict(upsample_initial_channel=176), b"176"),                                # 176 / 16 = 11: not a multiple of 8
    (dict(upsample_kernel_sizes=[16, 15, 4, 4]), b"15"),                         # k - u = 7 is odd
    (dict(resblock="3"), b"\"3\""),
    (dict(resblock_kernel_sizes=[3, 9, 11]), b"9"),
    (dict(resblock_dilation_sizes=[[1, 3, 5], [1, 4, 5], [1, 3, 5]]), b"4"),
    (dict(upsample_kernel_sizes=[24, 16, 4, 4]), b"24"),                         # k = 3u: even difference, not implemented
])
def test_plan_refuses_by_name(change, needle):
    from tacotron2_subword_amd import _lib as L
    cfg = L.hifigan_config(R.H(_v1(), **change))
    info = L.HifiganPlanInfo()
    rc = L.lib().t2_hifigan_plan(C.byref(cfg), 1, 10, C.byref(info))
    msg = L.lib().t2_last_error()
    assert rc != 0 and needle in msg, msg
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import Generator
    with pytest.raises(RuntimeError):
        Generator(R.H(_v1(), **change))


def test_forward_refuses_cpu_tensors(gold):
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import Generator
    gen = Generator(_config(gold, "rb1")).eval()
    with pytest.raises(RuntimeError, match="GPU"):
        gen(torch.zeros(1, 80, 4))
