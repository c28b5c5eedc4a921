"""CPU-only: pins the yardstick of the GPU tests of t2_lstm_seq_forward / _backward (tests/lstm_seq_ref.py).

Anchor: the plain statement against torch's own bidirectional nn.LSTM in fp64 through pack_padded_sequence /
pad_packed_sequence with unsorted lengths (weight_ih = I and zero biases make its input the pre-activations).
Sensitivity: five deliberate mistakes in the fp64 statement, each of which the bound function the GPU tests import must
reject on at least one compared quantity of every case tried."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import lstm_seq_ref as R


def test_statement_matches_torch_lstm_packed_unsorted():
    H, B, T = 64, 5, 7
    lengths = torch.tensor([7, 1, 4, 7, 2])
    g = torch.Generator().manual_seed(0)
    pre = [1.5 * torch.randn(T, B, 4 * H, generator=g, dtype=torch.float64) for _ in range(2)]
    w = [torch.randn(4 * H, H, generator=g, dtype=torch.float64) / H ** 0.5 for _ in range(2)]
    dh = [torch.randn(T, B, H, generator=g, dtype=torch.float64) for _ in range(2)]
    lstm = torch.nn.LSTM(4 * H, H, bidirectional=True).double()
    with torch.no_grad():
        for sfx, wd in (("", w[0]), ("_reverse", w[1])):
            getattr(lstm, "weight_ih_l0" + sfx).copy_(torch.eye(4 * H, dtype=torch.float64))
            getattr(lstm, "weight_hh_l0" + sfx).copy_(wd)
            getattr(lstm, "bias_ih_l0" + sfx).zero_()
            getattr(lstm, "bias_hh_l0" + sfx).zero_()
    # one input per direction: the two directions of nn.LSTM share theirs, so each is run with its own and read on its half
    for d in range(2):
        x = pre[d].clone().requires_grad_(True)
        out, _ = pad_packed_sequence(lstm(pack_padded_sequence(x, lengths, enforce_sorted=False))[0], total_length=T)
        h_t = out[:, :, d * H:(d + 1) * H]
        wp = getattr(lstm, "weight_hh_l0" + ("_reverse" if d else ""))
        dx, dw = torch.autograd.grad((h_t * dh[d]).sum(), (x, wp))
        mine = R.run(pre[d], w[d], bool(d), lengths, dh[d], torch.float64)
        for what, a, b in (("h", mine["h"], h_t.detach()), ("dpre", mine["dpre"], dx), ("dw_hh", mine["dw_hh"], dw)):
            err = float((a - b).abs().max())
            print(f"direction {d} {what}: {err:.3e}")
            assert err <= 1e-12, (d, what, err)
        for t in range(T):                                                # padding: everything saved is exactly zero
            dead = t >= lengths
            assert not mine["h"][t][dead].any() and not mine["c"][t][dead].any() and not mine["gates"][t][dead].any()
            assert not mine["dpre"][t][dead].any()


def test_unpacked_statement_is_lengths_all_T():
    x = R.inputs("h64_b5_t2")
    full = torch.full((5,), 2)
    for rev in (False, True):
        a = R.run(x.pre[0], x.w_hh[0], rev, None, x.dh[0], torch.float64)
        b = R.run(x.pre[0], x.w_hh[0], rev, full, x.dh[0], torch.float64)
        assert all(torch.equal(a[q], b[q]) for q in R.QUANTITIES)


def test_cases_are_what_the_tables_say():
    for z in R.PER_STEP + R.CHAIN:
        n = R.inputs(z.name).lengths
        assert all(r in (0, 1) for r in z.reverse) and 1 <= len(z.reverse) <= 4
        if isinstance(z.lengths, str):
            assert n.tolist() != sorted(n.tolist(), reverse=True), z.name          # not sorted descending
        if z.lengths in ("unsorted", "tail_group_1", "group1_short"):
            assert int(n.max()) == z.T and int(n.min()) == 1, z.name
        if z.lengths == "below_T":
            assert int(n.max()) == (47 if z.T == 50 else z.T - 1), z.name
        if z.lengths == "tail_group_1":
            first = (z.B - 1) // 32 * 32
            assert n[first:].tolist() == [1] * (z.B - first) and int(n[:first].max()) == z.T, z.name
        if z.lengths == "group1_short":
            assert int(n[32:64].max()) <= 2 and int(n[64:].max()) > 2 and int(n[:32].max()) > 2, z.name
    assert all(z.H == 256 and z.B <= 128 and len(z.reverse) <= 2 and z.chain for z in R.CHAIN)
    assert all(R.CASES[n].lengths is not None and 1 in R.CASES[n].reverse for n in R.SENSITIVITY)
    assert any(R.CASES[n] in R.CHAIN for n in R.SENSITIVITY) and any(R.CASES[n] in R.PER_STEP for n in R.SENSITIVITY)


@pytest.mark.parametrize("name", R.SENSITIVITY)
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_bound_rejects_defect(name, defect):
    """The defective fp64 statement must lie outside the bound the GPU tests use (both routes' factors: the larger one
    decides) on at least one compared quantity of at least one stream."""
    t64, dev = R.truth(name)
    bad = R.statement(name, torch.float64, defect)
    worst = 0.0
    for s in range(len(t64)):
        for q in R.QUANTITIES:
            err = float((bad[s][q] - t64[s][q]).abs().max())
            b = max(R.bound(route, q, dev[s][q], t64[s][q]) for route in R.F)
            print(f"{name} {defect} stream {s} {q}: err {err:.3e} bound {b:.3e} err/bound {err / b:.3g}")
            worst = max(worst, err / b)
    assert worst > 1.0, (name, defect, worst)


@pytest.mark.parametrize("name", R.SENSITIVITY)
def test_state_kept_past_length_shows_only_on_reverse_streams(name):
    """Why the cases need a reverse stream: on a forward stream the state past an item's length feeds nothing."""
    t64, _ = R.truth(name)
    bad = R.statement(name, torch.float64, "state_kept_past_length")
    for s, rev in enumerate(R.CASES[name].reverse):
        same = all(torch.equal(bad[s][q], t64[s][q]) for q in R.QUANTITIES)
        assert same == (not rev), (name, s, rev)
