"""CPU-only: the split-bf16 precision mode ("bf16x3", t2_set_precision(2)) at the binding level — the switch, the ABI
version, the GEMM kernel-family counters, the workspace layouts of the three modes, and the guard that keeps a pass
sized in one mode from being used in another."""
import ctypes

import pytest

from oracle import tacotron2_oracle as O

SMA, LSA = "StepwiseMonotonicAttention", "LSA"

# t2_decoder_layout_query / t2_decoder_bwd_layout_query at B=64, T=400, Tin=100, Tsub=60, default dims, as the commit
# before the split-bf16 mode answered them (modes 0 and 1 gave the same numbers): the new mode must not move them.
PARENT_FWD = {
    SMA: dict(total_floats=1052348488, din=553861120, gemm_ws=1033166856, gemm_ws_floats=16777216, chain=1049944072,
              usave=1052348488, locsaves=1052348488),
    LSA: dict(total_floats=1707708488, din=553861120, gemm_ws=1033166856, gemm_ws_floats=16777216, chain=1049944072,
              usave=1052348488, locsaves=1658556488),
}
PARENT_BWD = {
    SMA: dict(total_floats=715781384, ddin=52428800, colsum_ws=510751752, gemm_ws=511013896, gemm_ws_floats=201326592,
              chain=712340488),
    LSA: dict(total_floats=717598728, ddin=52428800, colsum_ws=512318472, gemm_ws=512580616, gemm_ws_floats=201326592,
              chain=713907208),
}


def _dims(att):
    from tacotron2_subword_amd import _lib as L
    hp = O.default_hparams()
    hp["attention"] = att
    return L.dims_from_hparams(hp)


def test_precision_switch_version_and_counters():
    from tacotron2_subword_amd import _lib as L
    assert L.lib().t2_version() == 4 and L.ABI_VERSION == 4
    try:
        for name, code in (("bf16x3", 2), ("bf16", 1), ("f32", 0), ("fp32", 0)):
            L.set_precision(name)
            assert L.lib().t2_get_precision() == code
            assert L.get_precision() == ("f32" if name == "fp32" else name)
        L.set_precision("bf16x3")
        assert L.lib().t2_set_precision(3) != 0                      # refused, with a message, and nothing changes
        assert b"t2_set_precision" in L.lib().t2_last_error() and b"3" in L.lib().t2_last_error()
        assert L.get_precision() == "bf16x3"
        with pytest.raises(KeyError):
            L.set_precision("bf16x2")
    finally:
        L.set_precision("f32")
    L.gemm_counts(reset=True)
    assert L.gemm_counts() == (0, 0, 0, 0)
    assert L.lib().t2_gemm_counts(None, 0) != 0


@pytest.mark.parametrize("att", [SMA, LSA])
def test_layouts_of_modes_0_and_1_are_the_parents_and_mode_2_grows_only_the_scratch(att):
    from tacotron2_subword_amd import _lib as L
    dims = _dims(att)
    try:
        for mode in ("f32", "bf16"):
            L.set_precision(mode)
            f, b = L.decoder_layout(dims, 64, 400, 100, 60), L.decoder_bwd_layout(dims, 64, 400, 100, 60)
            assert {k: getattr(f, k) for k in PARENT_FWD[att]} == PARENT_FWD[att], mode
            assert {k: getattr(b, k) for k in PARENT_BWD[att]} == PARENT_BWD[att], mode
        L.set_precision("bf16x3")
        f, b = L.decoder_layout(dims, 64, 400, 100, 60), L.decoder_bwd_layout(dims, 64, 400, 100, 60)
    finally:
        L.set_precision("f32")
    assert f.total_floats * 4 < 8 << 30                                 # the bound tests/test_abi.py holds the default mode to
    # everything in front of the scratch stays where it was; the scratch holds the staged operands of the products that
    # must take the split path at this shape: the chunked decoder-LSTM input product (3328 x 4096 x 3072: 6 bytes per
    # operand element) forward, dW_ih of the decoder LSTM (4096 x 3072 x 25600) plus its split-K partials backward
    assert f.din == PARENT_FWD[att]["din"] and f.gemm_ws == PARENT_FWD[att]["gemm_ws"]
    assert f.gemm_ws_floats * 4 >= 6 * (3328 + 4096) * 3072 + (64 << 20)
    assert f.total_floats - PARENT_FWD[att]["total_floats"] == f.gemm_ws_floats - PARENT_FWD[att]["gemm_ws_floats"]
    assert b.ddin == PARENT_BWD[att]["ddin"] and b.gemm_ws == PARENT_BWD[att]["gemm_ws"]
    assert b.gemm_ws_floats * 4 >= 6 * 25600 * (4096 + 3072) + 4 * 4096 * 3072 * 4
    assert b.total_floats - PARENT_BWD[att]["total_floats"] == b.gemm_ws_floats - PARENT_BWD[att]["gemm_ws_floats"]
    assert (f.total_floats + b.total_floats) * 4 < 16 << 30


def test_a_pass_sized_in_one_mode_is_refused_in_another():
    """The drivers recompute the layout from the mode in force and the C ABI carries no workspace size, so a pass keeps
    the mode it was sized in and every entry point compares (before it touches a pointer: this runs without a GPU)."""
    import torch
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd import ops
    dims = _dims(SMA)
    try:
        L.set_precision("f32")
        dp = ops.DecoderPass(dims, 2, 4, 5, 3, torch.device("cpu"))
        assert dp.precision == "f32"
        dp.check_precision("test")
        L.set_precision("bf16x3")
        big = ops.DecoderPass(dims, 2, 4, 5, 3, torch.device("cpu"))
        assert big.precision == "bf16x3" and big.ws.numel() > dp.ws.numel()
        mem, mels = torch.zeros(2, 5, 512), torch.zeros(2, 80, 4)
        with pytest.raises(RuntimeError, match="precision mode"):
            ops.decoder_forward(None, dims, mem, torch.zeros(2, 3, 512), None, None, mels, training=False, prenet_dropout=False,
                                seed=0, dp=dp)
        with pytest.raises(RuntimeError, match="precision mode"):
            ops.decoder_prologue(None, dims, dp, mels, training=False, prenet_dropout=False, seed=0)
        with pytest.raises(RuntimeError, match="precision mode"):
            ops.decoder_backward(None, {}, dims, dp, mem, None, None, None, training=False, prenet_dropout=False, seed=0)
        L.set_precision("bf16")
        with pytest.raises(RuntimeError, match="precision mode"):
            big.check_precision("test")
    finally:
        L.set_precision("f32")
    assert ctypes.sizeof(L.DecoderLayout) == 8 * len(L._LAYOUT_FIELDS)
