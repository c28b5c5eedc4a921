"""CPU-only: the split-bf16 recurrent steps (t2_set_split_steps; they act in precision mode "bf16x3" alone) at the
binding level — the switch, the ABI version, the per-step launch counters, the workspace layouts per (mode, switch), the
guard that keeps a pass sized under one switch state from being used under the other — and the error bound the GPU
tests hold the kernels to, checked against a torch emulation of the kernels' product."""
import pytest
import torch

from oracle import tacotron2_oracle as O

from split_steps_ref import error_ratio, split_product

SMA, LSA = "StepwiseMonotonicAttention", "LSA"
SHAPE = (64, 400, 100, 60)          # B, T, Tin, Tsub
HA, HD, E = 1024, 1024, 512
NA, ND = 4 * HA * (HA + E) // 2, 4 * HD * HD // 2            # floats one bf16 plane of an attention / decoder shadow takes
FRONT = ["x", "p1", "p2", "p1s", "p2s", "pm", "pms", "prea", "preas", "ga", "gas", "cna", "cnas", "ca", "cas", "din", "psel",
         "psels", "wcum", "wcums", "pred", "gd", "cnd", "cd", "dout", "qs", "qss", "qpart", "w1t", "w16a"]
BEHIND = ["din16", "dh16", "gemm_ws", "chain", "usave", "usaves", "locsave", "locsaves", "total_floats"]
SIZES = ["gemm_ws_floats", "chain_floats"]


def _dims(att):
    from tacotron2_subword_amd import _lib as L
    hp = O.default_hparams()
    hp["attention"] = att
    return L.dims_from_hparams(hp)


def _fwd(L, dims):
    lay = L.decoder_layout(dims, *SHAPE)
    return {k: getattr(lay, k) for k in L._LAYOUT_FIELDS}


def _bwd(L, dims):
    lay = L.decoder_bwd_layout(dims, *SHAPE)
    return {k: getattr(lay, k) for k in L._BWD_LAYOUT_FIELDS}


def test_switch_version_and_step_counters():
    from tacotron2_subword_amd import _lib as L
    assert L.lib().t2_version() == 4 and L.ABI_VERSION == 4
    assert {"t2_set_split_steps", "t2_get_split_steps", "t2_step_counts"} <= set(L.EXPORTS)
    before = L.get_split_steps()
    try:
        for on in (True, False, True):
            L.set_split_steps(on)
            assert L.get_split_steps() is on and L.lib().t2_get_split_steps() == int(on)
        assert L.get_precision() == "f32"                                # the switch leaves the mode alone
    finally:
        L.set_split_steps(before)
    L.step_counts(reset=True)
    assert L.step_counts() == (0,) * 6
    assert L.lib().t2_step_counts(None, 0) != 0
    assert b"null" in L.lib().t2_last_error()
    assert L.lib().t2_version() == 4


@pytest.mark.parametrize("att", [SMA, LSA])
def test_layouts_per_mode_and_switch(att):
    from tacotron2_subword_amd import _lib as L
    dims = _dims(att)
    off, on = {}, {}
    try:
        for mode in ("f32", "bf16", "bf16x3"):
            L.set_precision(mode)
            L.set_split_steps(False)
            off[mode] = (_fwd(L, dims), _bwd(L, dims))
            L.set_split_steps(True)
            on[mode] = (_fwd(L, dims), _bwd(L, dims))
            L.set_split_steps(False)
            assert (_fwd(L, dims), _bwd(L, dims)) == off[mode], mode     # off again: the earlier answers, exactly
    finally:
        L.set_split_steps(False)
        L.set_precision("f32")
    assert on["f32"] == off["f32"] and on["bf16"] == off["bf16"]        # the switch acts in mode 2 alone
    f0, b0 = off["bf16x3"]
    f1, b1 = on["bf16x3"]
    extra = 4 * NA + 2 * ND                                              # one lo plane per shadow: 4 attention, 2 decoder
    assert b1 == b0                                                      # the gradient kernel splits dg on the fly
    for k in FRONT + SIZES:
        assert f1[k] == f0[k], k
    for k in BEHIND:
        assert f1[k] == f0[k] + extra, k
    # hi plane, lo plane, next shadow
    assert f1["w16as"] - f1["w16a"] == 2 * NA and f1["w16d"] - f1["w16as"] == 2 * NA and f1["wt16a"] - f1["w16d"] == 2 * ND
    assert f1["wt16as"] - f1["wt16a"] == 2 * NA and f1["wt16d"] - f1["wt16as"] == 2 * NA and f1["din16"] - f1["wt16d"] == 2 * ND
    assert f0["w16as"] - f0["w16a"] == NA and f0["din16"] - f0["wt16d"] == ND
    assert f1["total_floats"] * 4 < 8 << 30


def test_a_pass_sized_under_one_switch_state_is_refused_under_the_other():
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd import ops
    dims = _dims(SMA)
    mem, sub, mels = torch.zeros(2, 5, 512), torch.zeros(2, 3, 512), torch.zeros(2, 80, 4)

    def refused(dp):
        with pytest.raises(RuntimeError, match="split steps"):
            ops.decoder_forward(None, dims, mem, sub, None, None, mels, training=False, prenet_dropout=False, seed=0, dp=dp)
        with pytest.raises(RuntimeError, match="split steps"):
            ops.decoder_prologue(None, dims, dp, mels, training=False, prenet_dropout=False, seed=0)
        with pytest.raises(RuntimeError, match="split steps"):
            ops.decoder_backward(None, {}, dims, dp, mem, None, None, None, training=False, prenet_dropout=False, seed=0)
    try:
        L.set_precision("bf16x3")
        L.set_split_steps(False)
        small = ops.DecoderPass(dims, 2, 4, 5, 3, torch.device("cpu"))
        assert small.precision == "bf16x3" and small.split_steps is False
        small.check_precision("test")
        L.set_split_steps(True)
        big = ops.DecoderPass(dims, 2, 4, 5, 3, torch.device("cpu"))
        assert big.precision == "bf16x3" and big.split_steps is True
        assert big.ws.numel() == small.ws.numel() + 4 * NA + 2 * ND
        big.check_precision("test")
        refused(small)
        L.set_split_steps(False)
        refused(big)
        L.set_precision("f32")                                          # the mode is still compared first
        with pytest.raises(RuntimeError, match="precision mode"):
            big.check_precision("test")
    finally:
        L.set_split_steps(False)
        L.set_precision("f32")


def _h_like(g, M, K):
    """rows like an LSTM's h = o * tanh(c): |x| < 1"""
    return (torch.sigmoid(torch.randn(M, K, generator=g)) * torch.tanh(torch.randn(M, K, generator=g))).float()


def _grad_like(g, M, K):
    """gate gradients: signed, magnitudes spread over five decades"""
    return (torch.randn(M, K, generator=g) * 10.0 ** (-1 - 5 * torch.rand(M, K, generator=g))).float()


@pytest.mark.parametrize("K,bkt,ksplit,kind", [(1536, 256, 1, "h"), (1536, 512, 1, "h"), (1536, 128, 1, "h"), (1024, 256, 1, "h"),
                                               (4096, 256, 8, "grad"), (4096, 128, 8, "grad")])
def test_the_bound_of_the_gpu_tests_holds_for_the_three_term_product_and_fails_a_broken_one(K, bkt, ksplit, kind):
    """bound = 8 * 2^-17 * sqrt(sum_k x_k^2 w_k^2) per output element, for the products of the step kernels (K = Ha + E and
    Hd, the stage widths of the three row-tile counts) and of the gradient kernel (K = 4H in eight spans): the three-term
    product stays below it, the product without the lo.hi term and the one-term product exceed it tenfold and more."""
    g = torch.Generator().manual_seed(K + bkt)
    M, N = 16, 64
    x = _h_like(g, M, K) if kind == "h" else _grad_like(g, M, K)
    w = ((torch.rand(N, K, generator=g) * 2 - 1) / 32).float()
    good = error_ratio(split_product(x, w, bkt, ksplit), x, w)
    dropped = error_ratio(split_product(x, w, bkt, ksplit, terms=("hh", "hl")), x, w)
    one = error_ratio(split_product(x, w, bkt, ksplit, terms=("hh",)), x, w)
    print(f"K={K} stage {bkt} spans {ksplit} {kind}: error / bound  three terms {good:.3f}  lo.hi dropped {dropped:.1f}  one term {one:.1f}")
    assert good < 1
    assert dropped > 10 and one > 10
