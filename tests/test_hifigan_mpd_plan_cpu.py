"""CPU-only: the pure plan of the multi-period discriminator (t2_hifigan_mpd_plan, csrc/vocoder_disc.hip) for every period at every
edge length of tests/hifigan_disc_ref.edge_lengths, pinned to tests/golden/hifigan_mpd_plans.jsonl and held against the row
arithmetic of the reference's convolutions restated in hifigan_disc_ref.rows; and the refusal of a T too short for the reflect pad.

`python tests/test_hifigan_mpd_plan_cpu.py` writes the pin again from the plan as it then is."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan_disc_ref as R  # noqa: E402

PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hifigan_mpd_plans.jsonl")
TILE = 128


def _plan_dict(period, B, T):
    from tacotron2_subword_amd import _lib as L
    info = L.hifigan_mpd_plan(period, B, T)
    out = {}
    for name, _ in info._fields_:
        v = getattr(info, name)
        out[name] = list(v) if hasattr(v, "__len__") else int(v)
    return out


def _cases():
    for p in R.PERIODS:
        for what, (B, T) in R.edge_lengths(p).items():
            yield p, what, 2 * B, T                     # real and generated items run as one batch
        yield p, "training shape", 32, 8192


def test_plans_match_the_pin_and_the_row_arithmetic():
    pinned = [json.loads(line) for line in open(PIN)]
    cases = list(_cases())
    assert len(pinned) == len(cases) and len(cases) >= 50
    for (p, what, B, T), pin in zip(cases, pinned):
        assert (pin["period"], pin["what"], pin["B"], pin["T"]) == (p, what, B, T)
        plan = _plan_dict(p, B, T)
        assert plan == pin["plan"], (p, what)
        H = R.rows(p, T)
        assert plan["H"] == H and plan["C"] == list(R.WIDTHS) and plan["pad"] == (p - T % p) % p
        for i in range(R.N_LAYERS):
            assert plan["fmap_floats"][i] == B * R.WIDTHS[i + 1] * H[i + 1] * p
            assert plan["tiles"][i] == (-(-H[i + 1] * p // TILE) if 1 <= i <= 4 else 0)
            assert plan["splits"][i] >= 1
        assert plan["workspace_bytes"] >= 2 * 4 * max(plan["fmap_floats"]) + plan["part_bytes"]
        assert plan["n_forward_launches"] == 6 and plan["n_backward_launches"] == 18


def test_edge_lengths_probe_what_they_say():
    for p in R.PERIODS:
        e = R.edge_lengths(p)
        assert e["H1"][1] == p and R.rows(p, p)[0] == 1
        assert (e["pad_p-1"][1] % p, e["pad_1"][1] % p) == (1, p - 1)
        assert sorted(R.rows(p, e[k][1])[0] % 3 for k in ("phase_H0=8", "phase_H0=9", "phase_H0=10")) == [0, 1, 2]
        assert sorted(R.rows(p, e[k][1])[1] % 3 for k in ("phase_H0=9", "phase_H0=10", "phase_H0=13")) == [0, 1, 2]
        ns = sorted(R.rows(p, T)[2] * p for k, (_, T) in e.items() if k.startswith("tile_N="))
        assert ns[0] == 127 // p * p <= 127 and ns[-1] == -(-129 // p) * p >= 129       # conv 1's N on both sides of one tile
        assert (128 in ns) == (p == 2) and (129 in ns) == (p == 3)
        several = _plan_dict(p, 4, e["several_tiles"][1])["tiles"]
        assert several[1] >= 2 and (R.rows(p, 2051)[1] * p > 256)                       # conv 1, and conv 0's positions, span several tiles
        assert R.rows(p, e["pad_p-1"][1])[4] == 1
    assert R.rows(7, 1000)[4] == 2 and R.rows(11, 1000)[4] == 2


@pytest.mark.parametrize("p,T", [(5, 2), (11, 5), (7, 3), (3, 1)])
def test_a_length_too_short_for_the_reflect_pad_is_refused(p, T):
    from tacotron2_subword_amd import _lib as L
    assert p - T % p > T - 1
    with pytest.raises(RuntimeError, match="too short for period"):
        L.hifigan_mpd_plan(p, 2, T)
    with pytest.raises(ValueError):
        R.rows(p, T)


def test_the_shortest_legal_lengths_are_taken():
    from tacotron2_subword_amd import _lib as L
    for p, T in [(5, 3), (11, 6), (2, 2), (3, 2), (7, 7), (7, 8)]:
        assert p - T % p <= T - 1 or T % p == 0
        assert list(L.hifigan_mpd_plan(p, 2, T).H) == R.rows(p, T)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(PIN, "w") as f:
        for p, what, B, T in _cases():
            f.write(json.dumps({"period": p, "what": what, "B": B, "T": T, "plan": _plan_dict(p, B, T)}) + "\n")
    print("wrote", PIN)
