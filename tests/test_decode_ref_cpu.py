"""Pins tests/decode_ref.py (the batched fp64 reference of the decode loop that the GPU decode-loop tests compare against)
to what the project already trusts: the oracle's own B == 1 decoder_inference, the golden vectors recorded from the
reference, and the two properties that define a batch with lengths.  CPU only."""
import pytest
import torch

from decode_ref import decode_ref, first_crossing
from helpers import DCA, FA2, GMM, LSA, SMA, hp_for, load_golden, maxabs, tiny_hp
from oracle import recipe
from oracle import tacotron2_oracle as O

KINDS = [SMA, LSA, FA2, GMM, DCA]


def _memories(hp, P, B, Tin, Tsub, seed):
    b = recipe.make_batch(hp, B, Tin, Tsub, 8, seed=seed, ragged=False)
    with torch.no_grad():
        return O.front_end(P, hp, b[0], None, b[7], "phone", False), O.front_end(P, hp, b[6], None, b[8], "sub", False)


def _keep(steps, B, Pn, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(steps, B, Pn, generator=g) < 0.5).float() for _ in range(4)]


def _close(r, ref, tol):
    for name, a, b in zip(("mel", "gate", "align", "align_sub"), r[:4], ref):
        assert maxabs(a, b) <= tol, name


@pytest.mark.parametrize("att", KINDS)
@pytest.mark.parametrize("dropout", [False, True])
def test_single_item_equals_oracle_inference(att, dropout):
    """B = 1, no lengths, fp32: the oracle's decoder_inference, with and without its keep-mask replay."""
    hp = tiny_hp(att)
    P = recipe.make_weights(hp, seed=5)
    steps, Pn = 14, hp["prenet_dim"]
    mem, mem_sub = _memories(hp, P, 1, 21, 7, seed=3)
    keep = _keep(steps, 1, Pn, 8) if dropout else None
    kw = dict(prenet_keep=torch.stack((keep[0], keep[1]), 1), prenet_bert_keep=torch.stack((keep[2], keep[3]), 1)) if dropout else {}
    with torch.no_grad():
        mel, gate, al, alb, flag = O.decoder_inference(mem, mem_sub, P, hp, max_decoder_steps=steps, gate_threshold=2.0, **kw)
    r = decode_ref(mem, mem_sub, P, hp, steps, keep=keep, dtype=torch.float32)
    _close(r, (mel.transpose(1, 2), gate.squeeze(-1), al, alb), 1e-6)
    if dropout:             # the activations obey their masks, and row 0 is the go frame's (no bias: zero)
        for v, k in zip(r[4:], keep):
            assert bool((v[k == 0] == 0).all()) and float(v[0].abs().max()) == 0.0


@pytest.mark.parametrize("att,name", [(SMA, "sma_infer"), (LSA, "lsa_infer")])
def test_golden_inference(att, name):
    g = load_golden(name)
    _, Tin, Tsub, steps = (int(v) for v in g["meta"])
    hp = hp_for(att)
    P = recipe.make_weights(hp)
    b = recipe.make_batch(hp, 1, Tin, Tsub, 8, seed=4321, ragged=False)
    with torch.no_grad():
        mem, mem_sub = O.front_end(P, hp, b[0], None, b[7], "phone", False), O.front_end(P, hp, b[6], None, b[8], "sub", False)
    r = decode_ref(mem, mem_sub, P, hp, steps)
    assert maxabs(r.mel.transpose(1, 2), g["fixed_mel"]) < 1e-5
    assert maxabs(r.gate.unsqueeze(-1), g["fixed_gate"]) < 1e-5
    assert maxabs(r.align, g["fixed_align"]) < 1e-5
    assert maxabs(r.align_sub, g["fixed_align_bert"]) < 1e-5
    k = int(g["stop_index"])
    long = r if k < steps else decode_ref(mem, mem_sub, P, hp, k + 1)
    assert int(first_crossing(long.gate, float(g["stop_threshold"]))[0]) == k


@pytest.mark.parametrize("att", KINDS)
def test_batch_equals_items_alone(att):
    hp = tiny_hp(att)
    P = recipe.make_weights(hp, seed=6)
    B, Tin, Tsub, steps = 4, 37, 9, 12
    mem, mem_sub = _memories(hp, P, B, Tin, Tsub, seed=9)
    keep = _keep(steps, B, hp["prenet_dim"], 2)
    li, ls = [37, 20, 1, 33], [9, 4, 1, 6]
    r = decode_ref(mem, mem_sub, P, hp, steps, li, ls, keep)
    for i in range(B):
        one = decode_ref(mem[i:i + 1], mem_sub[i:i + 1], P, hp, steps, li[i:i + 1], ls[i:i + 1], [k[:, i:i + 1] for k in keep])
        for name, a, b in zip(r._fields, r, one):
            sel = a[:, i:i + 1] if name.startswith("p") else a[i:i + 1]
            assert maxabs(sel, b) <= 1e-12, (name, i)


@pytest.mark.parametrize("att", [LSA, GMM])
def test_length_equals_truncated_memory(att):
    """A softmax over -inf-masked scores is the softmax of the truncated row: an item of length l equals the same item
    with its memories cut to l positions (LSA's location convolution pads with zeros, which is what the masked weights are)."""
    hp = tiny_hp(att)
    P = recipe.make_weights(hp, seed=7)
    Tin, Tsub, steps, l, ls = 37, 9, 12, 20, 4
    mem, mem_sub = _memories(hp, P, 1, Tin, Tsub, seed=10)
    keep = _keep(steps, 1, hp["prenet_dim"], 3)
    a = decode_ref(mem, mem_sub, P, hp, steps, [l], [ls], keep)
    b = decode_ref(mem[:, :l], mem_sub[:, :ls], P, hp, steps, None, None, keep)
    assert maxabs(a.mel, b.mel) <= 1e-12 and maxabs(a.gate, b.gate) <= 1e-12
    assert maxabs(a.align[:, :, :l], b.align) <= 1e-12 and maxabs(a.align_sub[:, :, :ls], b.align_sub) <= 1e-12
    assert float(a.align[:, :, l:].abs().max()) == 0.0 and float(a.align_sub[:, :, ls:].abs().max()) == 0.0
