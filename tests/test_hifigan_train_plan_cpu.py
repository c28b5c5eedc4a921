"""CPU-only: the host-side plan of HiFi-GAN generator training (csrc/vocoder_bwd.hip: hifigan_train_plan) through the pure-host
entry points t2_hifigan_train_plan and t2_hifigan_grad_offsets, which launch nothing and ask no device.

tests/golden/hifigan_train_plans.jsonl holds, per (configuration, B, T), every field of the plan's info struct in the order of
its fields, and per configuration the gradient offsets; every row must come out the same, exactly.  The tape, the gradient
arena and the launch counts are also worked out here from the configuration alone and held against the plan."""
import ctypes as C
import json
import os

import pytest
import torch

import hifigan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "hifigan_train_plans.jsonl")

TINY = {
    "tiny_rb1": dict(resblock="1", upsample_rates=[2], upsample_kernel_sizes=[4], upsample_initial_channel=16,
                     resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]]),
    "tiny_rb2": dict(resblock="2", upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
                     resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 2], [2, 6]]),
}
SHAPES = [(1, 1), (1, 2), (2, 5), (3, 33), (16, 32), (1, 400)]


def configurations():
    out = {f"config_v{v}": dict(R.load_config(os.path.join(GOLDEN, f"hifigan_config_v{v}.json"))) for v in (1, 2, 3)}
    out.update(TINY)
    return out


def round4(n):
    return (n + 3) // 4 * 4


def fields(info):
    return [list(v) if hasattr(v, "__len__") else v for v in (getattr(info, n) for n, _ in info._fields_)]


def rows():
    """What the library answers now, in the fixture's form."""
    from tacotron2_subword_amd import _lib as L
    out = []
    for tag, cfg in configurations().items():
        c = L.hifigan_config(R.H(cfg))
        n = L.hifigan_plan(c, 1, 1).n_layers
        w, b = L.hifigan_grad_offsets(c, n)
        out.append(dict(config=tag, grad_w_offsets=w, grad_b_offsets=b))
        for B, T in SHAPES:
            out.append(dict(config=tag, B=B, T=T, plan=fields(L.hifigan_train_plan(c, B, T))))
    return out


def test_plans_match_the_recording():
    want = [json.loads(line) for line in open(FIXTURE)]
    got = rows()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g.get("config"), g.get("B"), g.get("T"))


@pytest.mark.parametrize("tag", sorted(configurations()))
def test_tape_arena_and_launches_follow_from_the_configuration(tag):
    from tacotron2_subword_amd import _lib as L
    cfg = configurations()[tag]
    c = L.hifigan_config(R.H(cfg))
    layers = R.layer_names(cfg)
    kind1 = str(cfg["resblock"]) == "1"
    nk, nu, c0 = len(cfg["resblock_kernel_sizes"]), len(cfg["upsample_rates"]), cfg["upsample_initial_channel"]
    nd = len(cfg["resblock_dilation_sizes"][0])
    # the arena: dw in torch's layout, then db, each kept to 16 bytes, in layer order
    w, b = L.hifigan_grad_offsets(c, len(layers))
    off = 0
    for i, (_, _, cin, cout, k, _) in enumerate(layers):
        assert w[i] == off
        off += round4(cin * cout * k)
        assert b[i] == off
        off += round4(cout)
    for B, T in SHAPES:
        p = L.hifigan_train_plan(c, B, T)
        assert p.grad_floats == off and p.n_layers == len(layers)
        # the tape: conv_pre's output; per stage X and XS; per block the r_m (m >= 1) and, ResBlock1, the t_m
        tape, length, widest = round4(B * c0 * T), T, B * c0 * T
        for i, u in enumerate(cfg["upsample_rates"]):
            length *= u
            n = B * (c0 >> (i + 1)) * length
            widest = max(widest, n)
            tape += round4(n) * (2 + nk * ((nd - 1) + (nd if kind1 else 0)))
        assert p.out_len == length and p.tape_bytes == 4 * tape
        convs = len(layers) - 1
        counts = dict(zip(L.HIFIGAN_TRAIN_OPS, p.launches))
        assert counts == dict(conv=convs, conv_post=1, conv_post_backward=1, weight_gradient=convs, data_gradient=convs)
        assert p.n_forward_launches == len(layers)
        assert p.n_backward_launches == convs + 2 * (convs + 1)
        post = B * ((length + 255) // 256) * (7 * (c0 >> nu) + 1)
        assert p.workspace_bytes == 4 * 5 * round4(widest) + p.part_bytes + 4 * round4(2 * post)
        assert p.part_bytes % 16 == 0 and p.part_bytes > 0
        assert p.packed_bytes == L.hifigan_plan(c, B, T).packed_bytes
    # the plan does not depend on anything but the sizes: asking twice gives the same answer
    assert fields(L.hifigan_train_plan(c, 3, 33)) == fields(L.hifigan_train_plan(c, 3, 33))


def test_tape_at_the_published_training_shape():
    """config_v1, B = 16, 32 frames (segment 8192): the figure DESIGN.md states."""
    from tacotron2_subword_amd import _lib as L
    c = L.hifigan_config(R.H(configurations()["config_v1"]))
    p = L.hifigan_train_plan(c, 16, 32)
    assert p.out_len == 8192
    assert p.tape_bytes == 4 * 16 * (512 * 32 + 17 * (256 * 256 + 128 * 2048 + 64 * 4096 + 32 * 8192)) == 927989760


def test_refusals_by_name():
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import Generator
    bad = dict(TINY["tiny_rb2"], upsample_kernel_sizes=[24, 4])
    with pytest.raises(RuntimeError, match="not implemented"):
        L.hifigan_train_plan(L.hifigan_config(R.H(bad)), 1, 4)
    with pytest.raises(RuntimeError, match="dilation 4"):
        L.hifigan_train_plan(L.hifigan_config(R.H(dict(TINY["tiny_rb2"], resblock_dilation_sizes=[[1, 4], [2, 6]]))), 1, 4)
    c = L.hifigan_config(R.H(TINY["tiny_rb2"]))
    with pytest.raises(RuntimeError, match="T=0"):
        L.hifigan_train_plan(c, 1, 0)
    w = (C.c_size_t * 3)()
    assert L.lib().t2_hifigan_grad_offsets(C.byref(c), w, w, 3) != 0 and b"3 layers given" in L.lib().t2_last_error()
    gen = Generator(R.H(TINY["tiny_rb2"])).trainable()
    with pytest.raises(RuntimeError, match="lengths= together with a gradient"):
        gen(torch.zeros(2, 80, 4), lengths=[4, 3])
    # without the opt-in (or with it taken back) the refusal is the inference path's own
    for g in (Generator(R.H(TINY["tiny_rb2"])), gen.trainable(False)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            g(torch.zeros(2, 80, 4))


def test_new_structs_are_bound():
    """The header-against-binding test of test_abi.py walks every Structure of _lib.py; this only says the new ones are there."""
    from tacotron2_subword_amd import _lib as L
    for name in ("HifiganTrainPlanInfo", "HifiganTrainFwdArgs", "HifiganBwdArgs", "VocoderDgradArgs", "VocoderWgradArgs", "VocoderPostBwdArgs"):
        assert issubclass(getattr(L, name), C.Structure)
    assert L.ABI_VERSION == 4 and L.lib().t2_version() == 4


if __name__ == "__main__":                           # records the fixture
    with open(FIXTURE, "w") as f:
        for row in rows():
            f.write(json.dumps(row) + "\n")
    print("wrote", FIXTURE)
