"""GPU: the backward chains store dG as bf16 rows in place of the fp32 rows (t2_set_dg_handoff, csrc/chain_bwd.hip P phase) against
the fp32 rows and the three casts they replace.  Small model of test_gpu_chain.py: default dims, bf16 mode, chains on, one
forward + backward per switch setting on the same inputs and RNG keys.

The bf16 rows are what the cast would have made of the fp32 rows (round to nearest even, before the step tag goes into the
exchange fragment), the carves are unchanged, so every product reads the same operand bits from another address with the same
kernel, split-K factor and K chunks: every gradient must be bit-identical (torch.equal), not close.

Shapes.  The memories are 40 / 36 positions, those of test_gpu_chain.py's backward case, and not 7 / 5: the persistent backward
chains need at least 16 positions per memory (SMA: two position splits, LSA: 15-row halos), and below that the plan takes the
per-step launches, for which the switch changes nothing.
The chains may drop the fp32 rows only where no product reads them, and a product takes the shared bf16 copy only as whole tiles
(gemm_dispatch.hip plan_gemm): the input gradients need B*T % 128 == 0, the k-major weight gradients K >= 128 and K % 64 == 0 for
K = B*T and, the shifted ones, K = B*T - B.  So B is a multiple of 64 wherever rows are handed off, and the shapes first meant for
this test, (8, 8) with 24 padding rows (B*T - B = 56), (40, 8) with a partly filled second row tile (280) and (64, 2) (64 < 128), each
keep a product that converts the fp32 rows itself: there the plan keeps the rows and the casts.  They are run as what they are,
fallbacks (test_shapes_that_keep_the_fp32_rows); a run with the fp32 rows dropped at (8, 8) differed in every gradient.
Handed off:
  (64, 4)  the smallest: B*T = 256, B*T - B = 192; both row tiles full
  (64, 6)  B*T = 384 = 3 * 128, B*T - B = 320: an odd number of 128-row tiles and of 64-row K tiles
Before each run the plan is asked (t2_decoder_pass_plan with this device's facts); after it the profile says which chains ran
and t2_dg_handoff_counts how many casts were skipped and how many ran."""
import pytest
import torch

from helpers import LSA, SMA, hp_for, to_dev
from oracle import recipe

pytestmark = pytest.mark.gpu

TIN, TSUB = 40, 36
SHAPES = [(64, 4), (64, 6)]
KEPT = [(8, 8), (40, 8), (64, 2)]


@pytest.fixture(scope="module")
def env():
    from tacotron2_subword_amd import _lib as L, ops
    L.lib()
    handoff = L.get_dg_handoff()
    yield L, ops
    L.set_precision("f32")
    L.set_chain(True)
    L.set_chain_bwd(True)
    L.set_dg_handoff(handoff)
    _results.clear(); _weights.clear()


_weights, _results = {}, {}


def _model(L, att):
    if att not in _weights:
        hp = hp_for(att)
        P = to_dev(recipe.make_weights(hp))
        dims = L.dims_from_hparams(hp)
        _weights[att] = (P, dims, L.decoder_weights(P, dims.attention_kind))
    return _weights[att]


def _plan(L, dims, B, T, mode, chain, handoff):
    return L.decoder_pass_plan(dims, "backward", B, T, TIN, TSUB, precision=mode, split_steps=L.get_split_steps(), chain=chain, chain_bwd=True,
                               overlap=True, cus=torch.cuda.get_device_properties(0).multi_processor_count, claimed=bool(L.lib().t2_chain_claimed()),
                               saved_tiles=chain, dg_handoff=handoff)


def _pass(env, att, B, T, training, handoff, mode="bf16", chain=True, poison=False):
    """One forward + backward -> dict(loss, grads, counts = (skipped, ran), chains = launches of (B, A), plan, rows = the three dG
    regions).  The plain runs are kept: the tests share them, a reference is computed once."""
    key = (att, B, T, training, handoff, mode, chain, poison)
    if key in _results:
        return _results[key]
    L, ops = env
    P, dims, W = _model(L, att)
    g = torch.Generator().manual_seed(5)
    mem, mems = (torch.randn(B, TIN, 512, generator=g) * 0.5).cuda(), (torch.randn(B, TSUB, 512, generator=g) * 0.5).cuda()
    mels = torch.randn(B, 80, T, generator=g).cuda()
    tl = torch.randint(TIN // 2, TIN + 1, (B,), generator=g); tl[0] = TIN
    bl_ = torch.randint(TSUB // 2, TSUB + 1, (B,), generator=g); bl_[0] = TSUB
    dmel, dgate = torch.randn(B, T, 80, generator=g).cuda(), torch.randn(B, T, generator=g).cuda()
    dal, dals = (0.1 * torch.randn(B, T, TIN, generator=g)).cuda(), (0.1 * torch.randn(B, T, TSUB, generator=g)).cuda()
    L.set_precision(mode); L.set_chain(chain); L.set_chain_bwd(True); L.set_dg_handoff(handoff)
    try:
        plan = _plan(L, dims, B, T, mode, chain, handoff)
        dp = ops.decoder_forward(W, dims, mem, mems, tl.cuda(), bl_.cuda(), mels, training=training, prenet_dropout=training, seed=11)
        loss = (dp.mel * dmel).sum() + (dp.gate * dgate).sum() + (dp.align * dal).sum() + (dp.align_sub * dals).sum()
        bl = L.decoder_bwd_layout(dims, B, T, TIN, TSUB)
        bws = torch.empty(bl.total_floats, dtype=torch.float32, device="cuda")
        if poison:
            bws.fill_(float("nan"))
        L.prof_enable(8 * T + 64)
        L.dg_handoff_counts(reset=True)
        G, dm, dms = ops.decoder_backward(W, P, dims, dp, mem, mems, dmel, dgate, training=training, prenet_dropout=training, seed=11,
                                          d_align=dal, d_align_sub=dals, bws=bws)
        torch.cuda.synchronize()
        counts, prof = L.dg_handoff_counts(reset=True), L.prof_collect()
        assert not any(dp.chain_status()), dp.chain_status()
    finally:
        L.set_precision("f32"); L.set_chain(True); L.set_dg_handoff(True)
    BT = B * T
    rows = {k: bws[off:off + BT * 4096].clone() for k, off in (("dgd", bl.dgd), ("dga", bl.dga), ("dgas", bl.dgas))}
    out = dict(loss=loss.clone(), grads=dict(G, d_memory=dm, d_memory_sub=dms), counts=counts, plan=plan, rows=rows,
               chains=(prof["chain_b_bwd"][1], prof["chain_a_bwd"][1]))
    if mode == "bf16" and chain and not poison:
        _results[key] = out
    return out


def _same_gradients(a, b):
    assert torch.equal(a["loss"], b["loss"])
    assert a["grads"].keys() == b["grads"].keys() and len(a["grads"]) > 20
    for k, v in a["grads"].items():
        assert bool(torch.isfinite(v).all()), k
        assert torch.equal(v, b["grads"][k]), (k, float((v - b["grads"][k]).abs().max()))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("att", [SMA, LSA])
def test_switch_on_against_off(env, att, B, T, training):
    """(a) loss and every gradient bit-identical; 3 casts skipped and none run with the switch on, none skipped and 3 run with it off;
    both persistent backward chains ran, once each, under both settings."""
    on, off = _pass(env, att, B, T, training, True), _pass(env, att, B, T, training, False)
    for r, rows in ((on, True), (off, False)):
        p = r["plan"]
        assert p["chain_a"]["on"] and p["chain_b"]["on"] and p["share"] and p["chunk_cast"] and p["tail_share"], p
        assert (p["dg_rows_d"], p["dg_rows_a"]) == (rows, rows)
        assert r["chains"] == (1, 1), r["chains"]
    assert on["counts"] == (3, 0) and off["counts"] == (0, 3), (on["counts"], off["counts"])
    _same_gradients(on, off)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("att", [SMA, LSA])
def test_poisoned_workspace(env, att, B, T, training):
    """(b) the whole backward workspace is NaN beforehand: nothing reads the fp32 halves the chains no longer write (nor anything
    else it did not write itself): finite gradients, the bits of (a); and the chains left the upper halves of the three dG
    regions alone."""
    got, ref = _pass(env, att, B, T, training, True, poison=True), _pass(env, att, B, T, training, True)
    assert got["counts"] == (3, 0) and got["chains"] == (1, 1)
    _same_gradients(got, ref)
    half = B * T * 4096 // 2
    for k, v in got["rows"].items():
        assert bool(torch.isnan(v[half:]).all()), k                      # no fp32 row, no stray store
        assert bool(torch.isfinite(v[:half].view(torch.bfloat16).float()).all()), k


@pytest.mark.parametrize("B,T", KEPT)
@pytest.mark.parametrize("att", [SMA, LSA])
def test_shapes_that_keep_the_fp32_rows(env, att, B, T):
    """Both chains run and a copy is shared, but a product over B*T - B rows (or B*T < 128) would not take it: nothing is skipped,
    three casts run under either setting, and the gradients are equal.  (Padding rows and a partly filled row tile are only ever
    seen by the fp32 row stores: the guard of the bf16 row store is never false where it runs, B being a multiple of 64 there.)"""
    on, off = _pass(env, att, B, T, True, True), _pass(env, att, B, T, True, False)
    for r in (on, off):
        p = r["plan"]
        assert p["chain_a"]["on"] and p["chain_b"]["on"] and p["share"] and p["chunk_cast"] and p["tail_share"], p
        assert not p["dg_rows_d"] and not p["dg_rows_a"]
        assert r["chains"] == (1, 1) and r["counts"] == (0, 3), (r["chains"], r["counts"])
    _same_gradients(on, off)


@pytest.mark.parametrize("case", ["B33", "f32", "chains_off"])
def test_fallbacks(env, case):
    """(c) where the plan keeps the fp32 rows, no cast is skipped under either setting, as many run as the plan has shared copies
    (the chunk cast of the one step range + one per attention stream), and the gradients are those of the other setting."""
    B, T, mode, chain = {"B33": (33, 8, "bf16", True), "f32": (8, 8, "f32", True), "chains_off": (8, 8, "bf16", False)}[case]
    on, off = _pass(env, SMA, B, T, True, True, mode=mode, chain=chain), _pass(env, SMA, B, T, True, False, mode=mode, chain=chain)
    for r in (on, off):
        p = r["plan"]
        assert not p["dg_rows_d"] and not p["dg_rows_a"], p
        assert p["share"] == p["tail_share"] == (case == "chains_off") and len(p["bounds"]) == 2
        assert r["counts"] == (0, 3 if p["share"] else 0), (case, r["counts"])
        assert r["chains"] == ((1, 1) if case == "B33" else (0, 0)), r["chains"]
    _same_gradients(on, off)


@pytest.mark.parametrize("att", [SMA, LSA])
def test_rows_are_the_cast_of_the_fp32_rows(env, att):
    """(d) (64, 4): the bf16 rows the chains left at the head of the three dG regions against the library's own cast (t2_stage_bf16,
    the kernel behind the skipped casts) of the fp32 rows of the run with the switch off, as 16-bit integers: every word equal.
    A row copy taken after the step tag had replaced the lowest mantissa bit of a unit's first element would differ in about
    half of every eighth word."""
    L, _ = env
    B, T = 64, 4
    on, off = _pass(env, att, B, T, True, True), _pass(env, att, B, T, True, False)
    assert on["counts"] == (3, 0) and off["counts"] == (0, 3)
    for k in ("dgd", "dga", "dgas"):
        f32 = off["rows"][k].view(B * T, 4096)
        assert bool(torch.isfinite(f32).all()) and float(f32.abs().max()) > 0
        want = L.stage_bf16(f32).view(torch.int16)
        got = on["rows"][k][:B * T * 2048].view(torch.int16).view(B * T, 4096)
        torch.cuda.synchronize()
        assert torch.equal(want, f32.to(torch.bfloat16).view(torch.int16)), k          # the cast is plain round-to-nearest-even
        bad = int((got != want).sum())
        assert bad == 0, (k, bad, int((got[:, ::8] != want[:, ::8]).sum()))
