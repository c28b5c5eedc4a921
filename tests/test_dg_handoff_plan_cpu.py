"""CPU-only: the two dG hand-off decisions of the backward plan (csrc/decoder_plan.hip, t2_decoder_pass_plan: nothing is launched).

dg_rows_d: the decoder-LSTM chain stores dG as bf16 rows  <=>  switch on, chain B on, chunk_cast, and every product over that dG
           (dDIN of each range, dW_ih, the shifted dW_hh) takes the shared bf16 copy.
dg_rows_a: the attention chain does, for both streams     <=>  switch on, chain A on, tail_share, and the same of its four products.
The last condition is plan_gemm's answer for each product: whole 128-tiles of rows for the input gradients, and for the weight
gradients the k-major 256-tile kernel, K >= 128 and K % 64 == 0, K being B*T and, for the shifted ones, B*T - B.  With B*T % 64 == 0
that makes B a multiple of 64: a product that ignores the copy converts the fp32 rows itself, and those must then exist.
Each row below names the one condition it is on the far side of; its neighbour on the near side is in the table too.  Whatever
the switch says, the scratch carves (and with them every product's scratch, kernel, split-K factor and K chunks) stay as they are."""
import pytest

from helpers import LSA, SMA, hp_for

BASE = dict(att=SMA, B=64, T=4, Tin=40, Tsub=36, precision="bf16", chain=True, chain_bwd=True, cus=256, claimed=True, saved_tiles=True, dg_handoff=True,
            gemm_staging=True)

#        what differs from BASE                         dg_rows_d, dg_rows_a   why
ROWS = [(dict(),                                        True, True,   "everything holds: B = 64, B*T = 256, B*T - B = 192, both chains"),
        (dict(dg_handoff=False),                        False, False, "the switch"),
        (dict(gemm_staging=False),                      False, False, "products stage no copies: none takes the shared one"),
        (dict(T=6),                                     True, True,   "B*T = 384 = 3 * 128, B*T - B = 320"),
        (dict(T=3),                                     False, False, "B*T = 192 is no whole number of 128-row tiles: the input gradients convert fp32 rows"),
        (dict(T=2),                                     False, False, "T > 1 but B*T - B = 64 < 128: the shifted products are not k-major 256-tile ones"),
        (dict(T=1),                                     False, False, "T == 1: no shared copy"),
        (dict(B=8, T=8),                                False, False, "B*T = 64 shares a copy, B*T - B = 56 is no multiple of 64"),
        (dict(B=8, T=9),                                False, False, "B*T = 72 is no multiple of 64: no shared copy"),
        (dict(B=40, T=8),                               False, False, "B*T = 320 shares, B*T - B = 280"),
        (dict(B=60, T=16),                              False, False, "B % 8 != 0 at B*T = 960 = 15 * 64: no shared copy"),
        (dict(B=56, T=16),                              False, False, "B % 8 == 0, B*T = 896 = 7 * 128, B*T - B = 840"),
        (dict(B=33, T=8),                               False, False, "B % 8 != 0 and B*T % 64 != 0"),
        (dict(precision="f32"),                         False, False, "fp32 mode"),
        (dict(precision="bf16x3"),                      False, False, "split-bf16 mode"),
        (dict(chain=False),                             False, False, "chains off"),
        (dict(chain_bwd=False),                         False, False, "backward chains off"),
        (dict(cus=255),                                 False, False, "the device cannot hold a persistent grid"),
        (dict(claimed=False),                           False, False, "another process holds the claim"),
        (dict(Tsub=12),                                 False, False, "a 12-position memory: no attention chain, so no decoder-LSTM chain"),
        (dict(att=LSA),                                 True, True,   "LSA after a chain forward"),
        (dict(att=LSA, saved_tiles=False),              False, False, "LSA without saved tiles: the chain is refused"),
        (dict(T=400, Tin=100, Tsub=60),                 True, True,   "the benchmark's shape")]
SHARES = {"B*T = 64 shares a copy, B*T - B = 56 is no multiple of 64": True, "B*T = 72 is no multiple of 64: no shared copy": False,
          "B*T = 320 shares, B*T - B = 280": True, "B % 8 != 0 at B*T = 960 = 15 * 64: no shared copy": False,
          "B % 8 == 0, B*T = 896 = 7 * 128, B*T - B = 840": True, "T == 1: no shared copy": False,
          "T > 1 but B*T - B = 64 < 128: the shifted products are not k-major 256-tile ones": True}


def _plan(L, **over):
    r = dict(BASE, **over)
    dims = L.dims_from_hparams(hp_for(r.pop("att")))
    return L.decoder_pass_plan(dims, "backward", r.pop("B"), r.pop("T"), r.pop("Tin"), r.pop("Tsub"), defer_weight_grads=True, **r)


@pytest.mark.parametrize("over,rows_d,rows_a,why", ROWS, ids=[r[3] for r in ROWS])
def test_the_booleans_follow_from_their_conditions(over, rows_d, rows_a, why):
    from tacotron2_subword_amd import _lib as L
    p = _plan(L, **over)
    on = dict(BASE, **over)["dg_handoff"]
    assert (p["dg_rows_d"], p["dg_rows_a"]) == (rows_d, rows_a), (why, p["share"], p["chunk_cast"], p["tail_share"], p["chain_a"], p["chain_b"])
    assert not p["dg_rows_d"] or (on and p["chain_b"]["on"] and p["chunk_cast"])
    assert not p["dg_rows_a"] or (on and p["chain_a"]["on"] and p["tail_share"])
    if why in SHARES:                                                           # the shape conditions of the shared copy, either side
        assert p["share"] == p["tail_share"] == SHARES[why] and p["chain_a"]["on"] and p["chain_b"]["on"]
    # the switch moves nothing else: same carves, same chains, same places for the weight gradients
    q = _plan(L, **dict(over, dg_handoff=not on))
    strip = lambda d: {k: v for k, v in d.items() if k not in ("layout", "bwd_layout", "dg_rows_d", "dg_rows_a")}
    assert strip(p) == strip(q)
    assert p["bwd_layout"].total_floats == q["bwd_layout"].total_floats and p["bwd_layout"].dgd == q["bwd_layout"].dgd
    if rows_d:
        assert p["scratch"]["dg16"][1] > 0 and p["dec_wgrads_staged"]          # the carve's part stays, nothing is cast later
    if rows_a:
        assert p["tail_scratch"]["dg16"][1] > 0


def test_the_switch_and_the_counters_without_a_device():
    from tacotron2_subword_amd import _lib as L
    assert {"t2_set_dg_handoff", "t2_get_dg_handoff", "t2_dg_handoff_counts"} <= set(L.EXPORTS)
    before = L.get_dg_handoff()
    try:
        for on in (False, True):
            L.set_dg_handoff(on)
            assert L.get_dg_handoff() is on
    finally:
        L.set_dg_handoff(before)
    assert L.dg_handoff_counts(reset=True) is not None and L.dg_handoff_counts() == (0, 0)
    assert L.lib().t2_dg_handoff_counts(None, 0) != 0
