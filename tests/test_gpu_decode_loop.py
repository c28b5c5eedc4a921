"""The autoregressive decode loop (t2_decoder_infer) as production runs it: prenet dropout ON, padded batches with valid
lengths, every attention kind, in each of its three bodies:

  A  fp32, per-step launches           against the batched fp64 reference (decode_ref.py), 1e-4 max-abs (the project's contract)
  B  the stop rule (fp32)              stop index = the reference's first crossing; the rule perturbs no frame
  C  bf16 per-step loop                (use16 && !teacher: whole-cell weight shadows, bf16 ping-pong rows) against the fp32 HIP run
  D  bf16 persistent decode chain      against the fp32 HIP run; the dropout masks through a mask-swap distance

The keep bits of the HIP RNG are exported (ops.rng_keep_mask) and replayed through the reference; row t of a [steps,B,P]
mask belongs to the prenets that feed step t (keep-bit index t*B*P + b*P + n, written by the tail of step t-1)."""
import math

import pytest
import torch

from decode_ref import KEEP_SITES, decode_ref, first_crossing
from helpers import DCA, FA2, GMM, LSA, SMA, hp_for, maxabs, tiny_hp, to_dev
from oracle import recipe
from oracle import tacotron2_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4
KINDS = [SMA, LSA, FA2, GMM, DCA]
VIEWS = ("p1", "p2", "p1s", "p2s")
BF16_BOUNDS = dict(mel=0.05, gate=0.025, align=0.005, align_sub=0.005)     # test_config4_decode_b32_default_dims
TINY = dict(B=5, Tin=37, Tsub=9)
RAGGED = ([37, 1, 33, 20, 12], [9, 1, 4, 6, 2])    # full length; length 1 in each stream; an end inside the second 32-position tile


@pytest.fixture(scope="module")
def env():
    from tacotron2_subword_amd import _lib as L, ops
    L.lib()
    L.set_precision("f32")
    yield L, ops
    L.set_precision("f32")
    L.set_chain(True)


_CASES = {}


def case(att, B, Tin, Tsub, tiny=True, wseed=11, gate_shift=0.0, gate_scale=1.0, prenet2_scale=1.0, **over):
    """(hp, P, mem, mem_sub) on the CPU, built once per distinct request and never modified."""
    key = (att, B, Tin, Tsub, tiny, wseed, gate_shift, gate_scale, prenet2_scale, tuple(sorted(over.items())))
    if key not in _CASES:
        hp = tiny_hp(att) if tiny else hp_for(att)
        hp.update(over)
        P = recipe.make_weights(hp, seed=wseed)
        b = recipe.make_batch(hp, B, Tin, Tsub, 8, seed=77 + B, ragged=False)
        with torch.no_grad():
            mem = O.front_end(P, hp, b[0], None, b[7], "phone", False)
            mem_sub = O.front_end(P, hp, b[6], None, b[8], "sub", False)
        if gate_shift:
            P["decoder.gate_layer.linear_layer.bias"] = P["decoder.gate_layer.linear_layer.bias"] + gate_shift
        if gate_scale != 1.0:
            P["decoder.gate_layer.linear_layer.weight"] = P["decoder.gate_layer.linear_layer.weight"] * gate_scale
        if prenet2_scale != 1.0:
            for n in ("prenet", "prenet_bert"):
                k = f"decoder.{n}.layers.1.linear_layer.weight"
                P[k] = P[k] * prenet2_scale
        _CASES[key] = (hp, P, mem, mem_sub)
    return _CASES[key]


_DEV = {}


def dev_weights(P):
    if id(P) not in _DEV:
        _DEV[id(P)] = (P, to_dev(P))                       # (P kept alive: the id stays its own)
    return _DEV[id(P)][1]


def keep_masks(env, seed, steps, B, Pn):
    L, ops = env
    return [ops.rng_keep_mask(seed, L.SITE[s], steps * B * Pn, 0.5).view(steps, B, Pn).float().cpu() for s in KEEP_SITES]


class Run:
    pass


def run_hip(env, c, steps, *, dropout, seed=0, lengths=None, thr=2.0, poll=0):
    L, ops = env
    hp, P, mem, mem_sub = c
    dims = L.dims_from_hparams(hp)
    Pd = dev_weights(P)
    W = L.decoder_weights(Pd, dims.attention_kind)
    ml, sl = (None, None) if lengths is None else (torch.tensor(lengths[0]).cuda(), torch.tensor(lengths[1]).cuda())
    L.step_counts(reset=True)
    dp, n, stop = ops.decoder_infer(W, dims, mem.cuda(), mem_sub.cuda(), max_steps=steps, gate_threshold=thr, prenet_dropout=dropout,
                                    seed=seed, poll_every=poll, mem_lengths=ml, sub_lengths=sl)
    torch.cuda.synchronize()
    r = Run()
    B, Pn = mem.shape[0], hp["prenet_dim"]
    r.n, r.stop, r.counts, r.status = n, stop.cpu().long(), L.step_counts()[:3], dp.chain_status()
    r.mel, r.gate, r.align, r.align_sub = dp.mel.cpu(), dp.gate.cpu(), dp.align.cpu(), dp.align_sub.cpu()
    r.views = [dp.view(v, steps, B, Pn).cpu() for v in VIEWS]
    return r


def check_keep_bits(views, refs, keep, names=VIEWS):
    """Exact: 0 wherever the keep bit is 0, non-zero wherever it is 1 and the reference's value is well above zero; the go
    frame's row is zero (no bias)."""
    for name, v, ref, k in zip(names, views, refs, keep):
        assert bool((v[k == 0] == 0).all()), name
        assert bool((v[(k == 1) & (ref > 1e-3)] != 0).all()), name
        assert float(v[0].abs().max()) == 0.0, name
        assert v.shape[0] == 1 or int(((k == 1) & (ref > 1e-3)).sum()) > 0, name


def check_vs_ref(env, c, steps, *, dropout, seed=0, lengths=None, poll=0):
    hp, P, mem, mem_sub = c
    B, Pn = mem.shape[0], hp["prenet_dim"]
    r = run_hip(env, c, steps, dropout=dropout, seed=seed, lengths=lengths, poll=poll)
    keep = keep_masks(env, seed, steps, B, Pn) if dropout else None
    li, ls = (None, None) if lengths is None else lengths
    ref = decode_ref(mem, mem_sub, P, hp, steps, li, ls, keep)
    assert r.n == steps and bool((r.stop == -1).all())
    assert r.counts == (2 * steps, 0, 0), r.counts                  # two exact-family LSTM launches per frame: the per-step fp32 body
    errs = dict(mel=maxabs(r.mel, ref.mel), gate=maxabs(r.gate, ref.gate), align=maxabs(r.align, ref.align),
                align_sub=maxabs(r.align_sub, ref.align_sub))
    errs.update({n: maxabs(v, w) for n, v, w in zip(VIEWS, r.views, ref[4:])})
    print("decode loop fp32 vs fp64 reference:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < TOL for v in errs.values()), errs
    if dropout:
        check_keep_bits(r.views, ref[4:], keep)
    return r, ref, errs


# ------------------------------------------------------------------------------------------------ A: fp32 per-step loop
@pytest.mark.parametrize("att", KINDS)
@pytest.mark.parametrize("dropout", [False, True])
def test_fp32_every_kind(env, att, dropout):
    """Tiny dims, B = 5, 37 / 9 positions, 24 frames, no lengths (the reference's behaviour).  Observed over every case of
    section A: mel <= 7.5e-7, gate <= 3.0e-7, alignments <= 1.5e-7, prenet views <= 8.3e-7 (the reference's own fp32-vs-fp64
    distance at these shapes is <= 1.2e-6)."""
    check_vs_ref(env, case(att, **TINY), 24, dropout=dropout, seed=20250117)


@pytest.mark.parametrize("att", KINDS)
def test_fp32_every_kind_with_lengths(env, att):
    """The same batch padded: ragged mem_lengths / sub_lengths (RAGGED), dropout on."""
    r, ref, _ = check_vs_ref(env, case(att, **TINY), 24, dropout=True, seed=314159, lengths=RAGGED)
    if att != SMA:                    # the softmax kinds put exactly nothing on padding (SMA's recurrence walks its mass through it, as the reference's does)
        for b, (l, ls) in enumerate(zip(*RAGGED)):
            assert l == 37 or float(r.align[b, :, l:].abs().max()) == 0.0
            assert ls == 9 or float(r.align_sub[b, :, ls:].abs().max()) == 0.0


def test_mask_swap_moves_the_reference(env):
    """Power of the comparison above, on CPU arithmetic: in the fp64 reference another seed's masks move mel by more than
    100 x TOL (observed 4.9e-2 at this shape), so a wrong keep-bit index, site or scale cannot hide inside TOL."""
    c = case(SMA, **TINY)
    hp, P, mem, mem_sub = c
    a = decode_ref(mem, mem_sub, P, hp, 24, keep=keep_masks(env, 1, 24, 5, hp["prenet_dim"]))
    b = decode_ref(mem, mem_sub, P, hp, 24, keep=keep_masks(env, 2, 24, 5, hp["prenet_dim"]))
    d = maxabs(a.mel, b.mel)
    print("mask swap moves the reference mel by", d)
    assert d > 100 * TOL


@pytest.mark.parametrize("B", [1, 16, 17, 33, 65, 129])
def test_fp32_step_tail_workgroups_per_item(env, B):
    """proj_stop_kernel spreads an item over G = 16, 8, 4, 2, 1 workgroups; G changes at B = 16/17, 32/33, 64/65, 128/129."""
    check_vs_ref(env, case(SMA, B, 11, 6), 6, dropout=True, seed=5 + B)


STEP_TAIL_DIMS = {
    "prenet_320": dict(tiny=True, prenet_dim=320),           # layer 2: ragged second row pass (80 rows / slice) and column pass
    "prenet_512": dict(tiny=True, prenet_dim=512),           # two full passes of each
    "mel_128": dict(tiny=True, n_mel_channels=128),          # layer 1: MAXK values per thread, all used
    "wo_2112": dict(tiny=True, encoder_embedding_dim=1024, symbols_embedding_dim=1024),     # WO = 64 + 2*1024: second projection pass of 64 columns
    "default_dims": dict(tiny=False),                        # WO = 2048, P = 256, M = 80: exactly one pass of each
}


@pytest.mark.parametrize("name", list(STEP_TAIL_DIMS))
def test_fp32_step_tail_dims(env, name):
    kw = dict(STEP_TAIL_DIMS[name])
    B = 2 if name == "default_dims" else 3
    c = case(SMA, B, 11, 6, **kw)
    hp = c[0]
    if name == "wo_2112":
        assert hp["decoder_rnn_dim"] + 2 * hp["encoder_embedding_dim"] == 2112
    check_vs_ref(env, c, 6, dropout=True, seed=99)


def test_step_tail_refuses_132_mel_channels(env):
    """Layer 1 of the step tail holds n_mel <= 128 values in registers: 132 is an error (Python raises), never a run."""
    L, ops = env
    c = case(SMA, 3, 11, 6, n_mel_channels=132)
    with pytest.raises(RuntimeError, match=r"step_tail: M=132"):
        run_hip(env, c, 6, dropout=True, seed=1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("steps,poll", [(1, 0), (2, 0), (6, 1), (5, 9)])
def test_fp32_short_runs_and_polling(env, steps, poll):
    """max_steps = 1 (no prenet launch after the only frame), 2, one poll per frame, a polling interval longer than the run."""
    check_vs_ref(env, case(SMA, **TINY), steps, dropout=True, seed=7, poll=poll)


# ------------------------------------------------------------------------------------------------ B: stop rule
def _gap(s, thr, stop):
    """Smallest |sigmoid(gate) - thr| over the frames up to each item's stop (all frames of an item that never stops)."""
    T = s.shape[1]
    upto = torch.where(stop >= 0, stop, torch.full_like(stop, T - 1))
    live = torch.arange(T).unsqueeze(0) <= upto.unsqueeze(1)
    return float((s - thr).abs()[live].min())


def _thresholds(gate):
    """From the reference's gates: a threshold every item crosses at a different frame, and one that some item never
    crosses (and some item does); of the candidates, the one farthest from every sigmoid it is compared with (>= 1e-3)."""
    s = torch.sigmoid(gate)
    best = {True: (1e-3, None), False: (1e-3, None)}
    for thr in torch.linspace(float(s.min()), float(s.max()), 1001, dtype=torch.float64).tolist():
        stop = first_crossing(gate, thr)
        ncross = int((stop >= 0).sum())
        every = ncross == len(stop) and len(set(stop.tolist())) == len(stop)
        if every or 0 < ncross < len(stop):
            g = _gap(s, thr, stop)
            if g >= best[every][0]:
                best[every] = (g, thr)
    return best[True][1], best[False][1]


def test_stop_rule_fp32(env):
    """Tiny SMA, B = 6, dropout on, max_steps = 64, poll_every = 2.  Random weights give gates that are flat in time and differ
    by item, so no threshold is crossed by every item: the six items share one memory and differ by their dropout masks alone,
    and the second prenet layers and the gate weights are scaled by 8, which makes the masks move sigmoid(gate) by tenths."""
    steps, poll, B, seed = 64, 2, 6, 4242
    hp, P, mem, mem_sub = case(SMA, B, 37, 9, gate_scale=8.0, prenet2_scale=8.0)
    c = (hp, P, mem[:1].expand(B, -1, -1).contiguous(), mem_sub[:1].expand(B, -1, -1).contiguous())
    hp, P, mem, mem_sub = c
    keep = keep_masks(env, seed, steps, B, hp["prenet_dim"])
    ref = decode_ref(mem, mem_sub, P, hp, steps, keep=keep)
    s = torch.sigmoid(ref.gate)
    thr_all, thr_some = _thresholds(ref.gate)
    assert thr_all is not None and thr_some is not None, s
    free = run_hip(env, c, steps, dropout=True, seed=seed, thr=2.0, poll=poll)
    assert maxabs(free.gate, ref.gate) < TOL and maxabs(free.mel, ref.mel) < TOL

    def unperturbed(r, want):
        for b in range(B):
            k = int(want[b]) + 1 if want[b] >= 0 else r.n
            assert torch.equal(r.mel[b, :k], free.mel[b, :k]) and torch.equal(r.gate[b, :k], free.gate[b, :k])
            assert torch.equal(r.align[b, :k], free.align[b, :k]) and torch.equal(r.align_sub[b, :k], free.align_sub[b, :k])

    want = first_crossing(ref.gate, thr_all)
    assert _gap(s, thr_all, want) >= 1e-3 and len(set(want.tolist())) == B and int(want.min()) >= 0
    r = run_hip(env, c, steps, dropout=True, seed=seed, thr=thr_all, poll=poll)
    print("stop rule: threshold", thr_all, "stops", want.tolist(), "frames run", r.n)
    assert torch.equal(r.stop, want), (r.stop, want)
    assert int(want.max()) + 1 <= r.n <= min(steps, int(want.max()) + 1 + 3 * poll)
    unperturbed(r, want)

    want = first_crossing(ref.gate, thr_some)
    assert _gap(s, thr_some, want) >= 1e-3 and bool((want == -1).any())
    r = run_hip(env, c, steps, dropout=True, seed=seed, thr=thr_some, poll=poll)
    print("stop rule: threshold", thr_some, "stops", want.tolist(), "frames run", r.n)
    assert r.n == steps and torch.equal(r.stop, want), (r.n, r.stop, want)
    unperturbed(r, want)


# ------------------------------------------------------------------------------------------------ C: bf16 per-step loop
def _bf16_errs(rb, rf, frames=slice(None)):
    return dict(mel=maxabs(rb.mel[:, frames], rf.mel[:, frames]), gate=maxabs(rb.gate[:, frames], rf.gate[:, frames]),
                align=maxabs(rb.align[:, frames], rf.align[:, frames]), align_sub=maxabs(rb.align_sub[:, frames], rf.align_sub[:, frames]))


def _within(errs, bounds=BF16_BOUNDS):
    return all(errs[k] < bounds[k] for k in bounds)


def _own_threshold(gate):
    """Midway between two adjacent values of a run's own sigmoid(gate): the widest gap of the middle half of the values."""
    v = torch.unique(torch.sigmoid(gate).flatten())
    lo, hi = len(v) // 4, max(len(v) // 4 + 2, 3 * len(v) // 4)
    w = v[lo:hi]
    i = int((w[1:] - w[:-1]).argmax())
    return float((w[i] + w[i + 1]) / 2)


def _self_consistent_stop(env, c, first, steps, poll, **kw):
    """Rerun with a threshold between two of the first run's own gate values: every item stops on that run's first crossing,
    and the frames up to it are the first run's, bit for bit."""
    thr = _own_threshold(first.gate)
    want = first_crossing(first.gate, thr)
    r = run_hip(env, c, steps, thr=thr, poll=poll, **kw)
    if bool((want >= 0).all()):
        assert int(want.max()) + 1 <= r.n <= min(steps, int(want.max()) + 1 + 3 * poll)
    else:
        assert r.n == steps
    assert torch.equal(r.stop, want), (thr, r.stop, want)
    for b in range(len(want)):
        k = int(want[b]) + 1 if want[b] >= 0 else r.n
        assert torch.equal(r.mel[b, :k], first.mel[b, :k]) and torch.equal(r.gate[b, :k], first.gate[b, :k])
    return r


def _prenet_views_follow_own_mel(c, r, keep, steps):
    """p2 / p2s stay fp32 in the bf16 loop and come from the fp32 step tail reading the run's OWN mel frames: the reference's
    prenet of those frames pins them at TOL, and the keep bits exactly."""
    hp, P, mem, mem_sub = c
    B = mem.shape[0]
    x = torch.cat((torch.zeros(1, B, hp["n_mel_channels"]), r.mel.transpose(0, 1)[:steps - 1]), 0).double()
    refs = []
    for n, (k1, k2) in (("prenet", keep[:2]), ("prenet_bert", keep[2:])):
        w1, w2 = (P[f"decoder.{n}.layers.{i}.linear_layer.weight"].double() for i in (0, 1))
        refs.append(O.prenet(x, w1, w2, k1.double(), k2.double()))
    got = [r.views[1], r.views[3]]
    for name, v, ref in zip(("p2", "p2s"), got, refs):
        assert maxabs(v, ref) < TOL, name
    check_keep_bits(got, refs, [keep[1], keep[3]], ("p2", "p2s"))


BF16_STEP_CASES = {
    # name: (attention, B, tiny (decoder_rnn_dim 128: Ka = 256, Kd = 512) or default dims, frames, dropout, lengths, chain switch)
    "tiny_sma": (SMA, 5, True, 16, True, None, True), "tiny_lsa": (LSA, 5, True, 16, True, None, True),
    "tiny_fa2": (FA2, 5, True, 16, True, None, True), "tiny_gmm": (GMM, 5, True, 16, True, None, True),
    "tiny_dca": (DCA, 5, True, 16, True, None, True),
    "tiny_sma_no_dropout": (SMA, 5, True, 16, False, None, True),
    "tiny_gmm_lengths": (GMM, 5, True, 16, True, RAGGED, True),
    "tiny_sma_b33": (SMA, 33, True, 16, True, None, True),
    "tiny_sma_b129": (SMA, 129, True, 16, True, None, True),       # above 128 rows the loop keeps fp32 operands
    "default_sma_b33": (SMA, 33, False, 8, True, None, True),      # past the persistent chain's 32 rows
    "default_lsa_b33_lengths": (LSA, 33, False, 8, False, "ragged33", True),
    "default_sma_b3_chain_off": (SMA, 3, False, 8, True, None, False),
}


@pytest.mark.parametrize("name", list(BF16_STEP_CASES))
def test_bf16_per_step_loop(env, name):
    """bf16 operands, one launch per phase and frame, against the fp32 HIP run of the same seed (pinned by A).  Bounds: the
    bf16-mode bounds of test_config4_decode_b32_default_dims."""
    L, ops = env
    att, B, tiny, steps, dropout, lengths, chain_on = BF16_STEP_CASES[name]
    Tin, Tsub = 37, 9
    c = case(att, B, Tin, Tsub, decoder_rnn_dim=128) if tiny else case(att, B, Tin, Tsub, tiny=False, wseed=1234)
    if lengths == "ragged33":
        lengths = ([37, 1, 33, 20, 12] + [37 - (i % 30) for i in range(28)], [9, 1, 4, 6, 2] + [9 - (i % 8) for i in range(28)])
    seed = 77001
    kw = dict(dropout=dropout, seed=seed, lengths=lengths)
    rf = run_hip(env, c, steps, **kw)
    assert rf.counts == (2 * steps, 0, 0)
    L.set_precision("bf16")
    try:
        L.set_chain(chain_on)
        rb = run_hip(env, c, steps, **kw)
        assert rb.counts == ((2 * steps, 0, 0) if B > 128 else (0, 2 * steps, 0)), rb.counts       # the family that took the LSTM steps
        rs = _self_consistent_stop(env, c, rb, steps, 2, **kw)
        assert rs.counts[2] == 0 and rs.counts[0 if B > 128 else 1] == 2 * rs.n
    finally:
        L.set_chain(True)
        L.set_precision("f32")
    assert rb.n == steps and not any(rb.status)
    errs = _bf16_errs(rb, rf)
    print(f"bf16 per-step decode loop [{name}] vs fp32 HIP:", {k: f"{v:.2e}" for k, v in errs.items()})
    # observed, tiny dims: mel <= 1.1e-3, gate <= 1.1e-3, alignments <= 1.7e-4; default dims: 2.4e-3 / 1.2e-3 / 1.5e-3; B = 129: all 0
    assert _within(errs), errs
    if lengths is not None and att != SMA:          # a softmax kind puts exactly nothing on padding, in either mode
        for r in (rf, rb):
            for b, (l, ls) in enumerate(zip(*lengths)):
                assert l == Tin or float(r.align[b, :, l:].abs().max()) == 0.0
                assert ls == Tsub or float(r.align_sub[b, :, ls:].abs().max()) == 0.0
    if dropout:
        _prenet_views_follow_own_mel(c, rb, keep_masks(env, seed, steps, B, c[0]["prenet_dim"]), steps)


# ------------------------------------------------------------------------------------------------ D: persistent decode chain
def _run_chain(env, c, steps, **kw):
    """One bf16 run that must go through the persistent decode chain: ceil(steps / 32) launches, clean status, no per-step LSTM."""
    L, ops = env
    L.set_precision("bf16")
    try:
        L.prof_enable(64)
        r = run_hip(env, c, steps, **kw)
        prof = L.prof_collect()
    finally:
        L.set_precision("f32")
    poll = kw.get("poll", 0) or 32
    launches = math.ceil(r.n / poll)
    assert prof["chain_dec"][1] == launches, prof
    assert not any(r.status) and r.counts == (0, 0, 0), (r.status, r.counts)
    return r


def _chain_case(att, B, **kw):
    return case(att, B, 37, 9, tiny=False, wseed=1234, **kw)


@pytest.mark.parametrize("att", [SMA, LSA])
@pytest.mark.parametrize("B", [1, 3, 32])
@pytest.mark.parametrize("steps", [1, 33, 40])
def test_chain_without_dropout(env, att, B, steps):
    """Launches of 1, 32 + 1 and 32 + 8 frames, default dims, against the fp32 HIP run under the bf16-mode bounds."""
    c = _chain_case(att, B)
    rf = run_hip(env, c, steps, dropout=False)
    rb = _run_chain(env, c, steps, dropout=False)
    assert rb.n == steps and bool((rb.stop == -1).all())
    errs = _bf16_errs(rb, rf)
    print(f"persistent decode chain [{att} B={B} steps={steps}] vs fp32 HIP:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert _within(errs), errs          # observed over the 18 cases: mel <= 9.3e-3, gate <= 8.0e-3, align <= 2.0e-3, align_sub <= 1.8e-3


@pytest.mark.parametrize("att", [SMA, LSA])
def test_chain_with_lengths(env, att):
    """Ragged lengths at default dims.  Both sides of the comparison take their lengths through the same entry point, so
    the fp32 HIP side is first pinned to the fp64 reference with those lengths."""
    c = _chain_case(att, 3)
    lengths = ([37, 33, 1], [9, 1, 4])
    hp, P, mem, mem_sub = c
    rf = run_hip(env, c, 40, dropout=False, lengths=lengths)
    ref = decode_ref(mem, mem_sub, P, hp, 40, *lengths)
    assert max(maxabs(rf.mel, ref.mel), maxabs(rf.gate, ref.gate), maxabs(rf.align, ref.align), maxabs(rf.align_sub, ref.align_sub)) < TOL
    rb = _run_chain(env, c, 40, dropout=False, lengths=lengths)
    errs = _bf16_errs(rb, rf)
    print(f"persistent decode chain [{att} ragged lengths] vs fp32 HIP:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert _within(errs), errs          # observed: mel 9.0e-3, gate 4.0e-3, align 1.2e-3, align_sub 1.4e-4
    if att != SMA:                    # (SMA's recurrence walks its mass through the padding, as the reference's does)
        assert float(rb.align[1, :, 33:].abs().max()) == 0.0 and float(rb.align[2, :, 1:].abs().max()) == 0.0
        assert float(rb.align_sub[1, :, 1:].abs().max()) == 0.0 and float(rb.align_sub[2, :, 4:].abs().max()) == 0.0


@pytest.mark.parametrize("att", [SMA, LSA])
@pytest.mark.parametrize("B", [1, 3, 32])
def test_chain_dropout_masks(env, att, B):
    """Dropout on.  The bf16 bounds cannot see a wrong mask (another seed's masks move mel by about 0.06 at these weights), so
    the second prenet layers are scaled by 8 and frames 1-8 compared: per item, the chain must stay within a quarter of the
    distance by which another seed's masks move the fp32 HIP run."""
    c = _chain_case(att, B, prenet2_scale=8.0)
    steps, f = 33, slice(1, 9)
    fa = run_hip(env, c, steps, dropout=True, seed=1001)
    fb = run_hip(env, c, steps, dropout=True, seed=2002)
    ch = _run_chain(env, c, steps, dropout=True, seed=1001)
    d_chain = (ch.mel[:, f] - fa.mel[:, f]).abs().flatten(1).max(1).values
    d_swap = (fb.mel[:, f] - fa.mel[:, f]).abs().flatten(1).max(1).values
    print(f"chain with dropout [{att} B={B}] frames 1-8: chain vs fp32", [f"{v:.3f}" for v in d_chain.tolist()],
          "mask swap in fp32", [f"{v:.3f}" for v in d_swap.tolist()])
    # observed over all items: chain vs fp32 0.005 .. 0.009, mask swap 0.175 .. 0.334
    assert bool((d_chain <= 0.25 * d_swap).all()), (d_chain, d_swap)


@pytest.mark.parametrize("att", [SMA, LSA])
def test_chain_stop_rule_and_determinism(env, att):
    """Two identical runs are bit-equal; a rerun with a threshold between two of the first run's own gate values (launches
    of 4 frames) stops every item on that run's first crossing and leaves the frames up to it untouched."""
    c = _chain_case(att, 3)
    kw = dict(dropout=True, seed=31337)
    a = _run_chain(env, c, 40, **kw)
    b = _run_chain(env, c, 40, **kw)
    for x, y in ((a.mel, b.mel), (a.gate, b.gate), (a.align, b.align), (a.align_sub, b.align_sub)):
        assert torch.equal(x, y)

    thr = _own_threshold(a.gate)
    want = first_crossing(a.gate, thr)
    r = _run_chain(env, c, 40, thr=thr, poll=4, **kw)
    assert torch.equal(r.stop, want), (thr, r.stop, want)
    if bool((want >= 0).all()):
        assert int(want.max()) + 1 <= r.n <= min(40, int(want.max()) + 1 + 3 * 4)
    else:
        assert r.n == 40
    for i in range(3):
        k = int(want[i]) + 1 if want[i] >= 0 else r.n
        assert torch.equal(r.mel[i, :k], a.mel[i, :k]) and torch.equal(r.gate[i, :k], a.gate[i, :k])
