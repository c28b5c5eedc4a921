"""GPU: the whole model in the split-bf16 precision mode ("bf16x3") — the fp32 mode's arithmetic everywhere except the
large GEMMs, which run as three bf16 products with fp32 accumulation.  Yardsticks: the CPU oracle (the project's 1e-4
contract, the TOL of tests/test_gpu_model.py), the exact fp32 mode on the same inputs, and the recorded goldens."""
import numpy as np
import pytest
import torch

from oracle import recipe
from oracle import tacotron2_oracle as O

from helpers import LSA, SMA, hp_for, load_golden, maxabs

pytestmark = pytest.mark.gpu
TOL = 1e-4
NAMES = ("mel", "mel_postnet", "gate", "align", "align_bert")


def build_model(att, train=False):
    from tacotron2_subword_amd.hparams import create_hparams
    from tacotron2_subword_amd.model import BERT_Tacotron2
    hps = create_hparams()
    hps.attention = att
    m = BERT_Tacotron2(hps)
    m.load_state_dict(recipe.make_weights(hp_for(att)))
    m = m.cuda()
    m.train(train)
    m.decoder.prenet_dropout = False
    return m, hps


def predicted_forward_counts(B, Tin, Tsub, T):
    """(exact, split) products of one eval forward, from the shapes alone.  The dispatch rule (include/t2amd.h, mode 2): a
    product takes the split path iff it has scratch, batch 1, M and N whole 128-tiles and both >= 256, K % 64 == 0, an
    implicit-conv operand with C % 64 == 0, and 2*M*N*K >= 2^31; everything else runs the exact kernel.  The products
    (default dims: 512 encoder channels, 768-wide CLS rows, prenet 256, attention 128, LSTMs 1024, WD = 3072, 80 mels):"""
    E, CLS, P, A, H, WD, NM = 512, 768, 256, 128, 1024, 3072, 80
    prods = []                                                       # (what, count, M, N, K, scratch, conv channels or None)
    for name, rows in (("phone", B * Tin), ("sub-word", B * Tsub)):
        prods += [(name + " encoder conv", 3, rows, E, 5 * E, True, E),
                  (name + " BiLSTM input, per direction", 2, rows, 4 * (E // 2), E, True, None),
                  (name + " converter [enc | cls]", 1, rows, E, E + CLS, True, None),
                  (name + " processed memory", 1, rows, A, E, False, None)]
    BT = B * T
    prods += [("prenet layer 1 (two streams)", 2, BT, P, NM, False, None), ("prenet layer 2", 2, BT, P, P, False, None),
              ("attention-LSTM input", 2, BT, 4 * H, P, True, None),
              ("decoder-LSTM input, chunks of 16 steps", T // 16, 16 * B, 4 * H, WD, True, None),
              ("mel projection", 1, BT, NM, 2 * H, False, None), ("gate projection", 1, BT, 1, 2 * H, False, None),
              ("postnet conv 80 -> 512", 1, BT, E, 5 * NM, True, NM), ("postnet conv 512 -> 512", 3, BT, E, 5 * E, True, E),
              ("postnet conv 512 -> 80", 1, BT, NM, 5 * E, True, E)]
    exact = split = 0
    for what, n, M, N, K, scratch, convc in prods:
        ok = (scratch and M % 128 == 0 and N % 128 == 0 and K % 64 == 0 and M >= 256 and N >= 256
              and (convc is None or convc % 64 == 0) and 2 * M * N * K >= 2 ** 31)
        print(f"  {n} x {what}: {M} x {N} x {K} -> {'split' if ok else 'exact'}")
        split, exact = split + n * ok, exact + n * (not ok)
    return exact, split


@pytest.mark.parametrize("att", [SMA, LSA])
def test_forward_eval_split_vs_oracle_and_fp32_mode(att):
    """Eval forward at B=16, Tin=96, Tsub=64, T=128 (every B*T extent a whole 256-tile multiple; the decoder-LSTM input
    product comes in chunks of 16 steps x 16 = 256 rows), ragged lengths: all five outputs within 1e-4 of the oracle
    computed here AND of the exact fp32 mode, no product on a single-bf16 kernel, and the numbers of products on the exact
    and on the split path EQUAL what the shapes predict (predicted_forward_counts: 16 exact, 19 split — the six encoder
    convolutions, the two attention-LSTM input products, the eight decoder-LSTM input chunks, three postnet layers)."""
    from tacotron2_subword_amd import _lib as L
    hp = hp_for(att)
    B, Tin, Tsub, T = 16, 96, 64, 128
    m, hps = build_model(att)
    batch = recipe.make_batch(hp, B, Tin, Tsub, T)
    x, y = m.parse_batch(batch)
    with torch.no_grad():
        L.gemm_counts(reset=True)
        out0 = [o.detach().clone() for o in m(x)]
        c0 = L.gemm_counts(reset=True)
        L.set_precision("bf16x3")
        try:
            out3 = [o.detach().clone() for o in m(x)]
            c3 = L.gemm_counts(reset=True)
        finally:
            L.set_precision("f32")
        xo, _ = recipe.parse_batch(batch)
        ref = O.forward(recipe.make_weights(hp), hp, xo, training=False)
    e_or = {k: maxabs(a, b) for k, a, b in zip(NAMES, out3, ref)}
    e_32 = {k: maxabs(a, b) for k, a, b in zip(NAMES, out3, out0)}
    e_0 = {k: maxabs(a, b) for k, a, b in zip(NAMES, out0, ref)}
    print(att, "gemm counts (exact, converting, single-bf16 source, split source): f32 mode", c0, " bf16x3 mode", c3)
    print(att, "bf16x3 vs oracle:", e_or)
    print(att, "bf16x3 vs f32 mode:", e_32)
    print(att, "f32 mode vs oracle:", e_0)
    assert c0[1] == c0[2] == c0[3] == 0
    exact, split = predicted_forward_counts(B, Tin, Tsub, T)
    assert c0 == (exact + split, 0, 0, 0), (c0, exact, split)
    assert c3 == (exact, 0, 0, split), (c3, exact, split)
    for k in NAMES:
        assert e_or[k] < TOL, (k, e_or)
        assert e_32[k] < TOL, (k, e_32)


def test_goldens_in_split_mode():
    """sma_baseline_eval (B=2: hardly a whole tile anywhere) in mode bf16x3 at the existing TOL: the fallback really is
    the exact path."""
    from tacotron2_subword_amd import _lib as L
    g = load_golden("sma_baseline_eval")
    B, Tin, Tsub, T, _ = (int(v) for v in g["meta"])
    m, hps = build_model(SMA)
    x, y = m.parse_batch(recipe.make_batch(hp_for(SMA), B, Tin, Tsub, T))
    L.set_precision("bf16x3")
    try:
        L.gemm_counts(reset=True)
        with torch.no_grad():
            out = m(x)
        counts = L.gemm_counts()
    finally:
        L.set_precision("f32")
    print("sma_baseline_eval in bf16x3:", counts, {k: maxabs(v, g[k]) for k, v in zip(NAMES, out)})
    assert counts[1] == counts[2] == 0
    for k, v in zip(NAMES, out):
        assert maxabs(v, g[k]) < TOL, k


@pytest.mark.parametrize("att,name", [(SMA, "sma_infer"), (LSA, "lsa_infer")])
def test_inference_goldens_in_split_mode(att, name):
    """inference() is unaffected by the mode: fixed-length frames at TOL, stop frame bit-exact."""
    from tacotron2_subword_amd import _lib as L
    g = load_golden(name)
    _, Tin, Tsub, steps = (int(v) for v in g["meta"])
    m, hps = build_model(att)
    b = recipe.make_batch(hp_for(att), 1, Tin, Tsub, 8, seed=4321, ragged=False)
    ids, sub, pcls, bcls = b[0].cuda(), b[6].cuda(), b[7].cuda(), b[8].cuda()
    L.set_precision("bf16x3")
    try:
        L.gemm_counts(reset=True)
        m.decoder.gate_threshold, m.decoder.max_decoder_steps = 2.0, steps
        r = m.inference(ids, sub, pcls, bcls)
        m.decoder.gate_threshold, m.decoder.max_decoder_steps = float(g["stop_threshold"]), 1000
        r2 = m.inference(ids, sub, pcls, bcls)
        torch.cuda.synchronize()
        counts = L.gemm_counts()
    finally:
        L.set_precision("f32")
    assert counts[1] == counts[2] == 0
    assert r[5] is False and r2[5] is True
    for k, v in zip(NAMES, r[:5]):
        assert maxabs(v, g["fixed_" + k]) < TOL, k
    assert r2[0].shape[2] - 1 == int(g["stop_index"])
    assert maxabs(r2[0], g["stop_mel"]) < TOL and maxabs(r2[1], g["stop_mel_postnet"]) < TOL


@pytest.mark.parametrize("att", [SMA, LSA])
def test_backward_split_vs_oracle_autograd(att):
    """The recipe of test_backward_eval_mode_vs_oracle_autograd (fp64 oracle autograd as truth, max(5e-4, 3 x the fp32
    oracle's own error) relative per parameter) at a tile-aligned shape in mode bf16x3; the weight-gradient products go
    through the k-major split route (counter), the dead decoder_rnn_bert keeps grad None."""
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd.loss_function import Tacotron2Loss
    hp = hp_for(att)
    B, Tin, Tsub, T = 8, 64, 32, 64
    m, hps = build_model(att, train=False)
    batch = recipe.make_batch(hp, B, Tin, Tsub, T)
    x, y = m.parse_batch(batch)
    L.set_precision("bf16x3")
    try:
        out = m(x)
        loss = Tacotron2Loss()(out, y, x)[0]
        L.gemm_counts(reset=True)
        loss.backward()
        torch.cuda.synchronize()
        cb = L.gemm_counts()
    finally:
        L.set_precision("f32")

    def oracle_grads(dt):
        P = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in recipe.make_weights(hp).items()}
        for k, v in P.items():
            if v.is_floating_point() and "running" not in k:
                v.requires_grad_(True)
        cast = lambda ts: tuple(t.to(dt) if torch.is_tensor(t) and t.is_floating_point() else t for t in ts)
        xo, yo = recipe.parse_batch(batch)
        lo = O.loss(O.forward(P, hp, cast(xo), training=False), cast(yo))[0]
        lo.backward()
        return float(lo.detach()), {k: (None if v.grad is None else v.grad.double()) for k, v in P.items() if v.is_floating_point()}
    lo32, g32 = oracle_grads(torch.float32)
    _, g64 = oracle_grads(torch.float64)
    print(att, "backward gemm counts in bf16x3:", cb, " loss", float(loss.detach()), "oracle fp32 loss", lo32)
    assert cb[1] == cb[2] == 0 and cb[3] > 0, cb
    # (the loss is a sum of two means of order 50 at this shape, where one fp32 ulp is 3.8e-6: 1e-5 RELATIVE, the figure the
    # small-shape test applies to its order-one loss, i.e. the forward outputs' 1e-4 contract seen through the means)
    assert abs(float(loss.detach()) - lo32) < 1e-5 * max(1.0, abs(lo32))
    bad, worst = {}, (0.0, None)
    for k, p in m.named_parameters():
        ref = g64[k]
        if ref is None:
            assert p.grad is None, k
            continue
        scale = max(float(ref.abs().max()), 1e-7)
        err = float((p.grad.double().cpu() - ref).abs().max()) / scale
        noise = float((g32[k] - ref).abs().max()) / scale
        worst = max(worst, (err, k))
        if not err < max(5e-4, 3 * noise):
            bad[k] = (err, noise)
    print(att, "worst relative gradient error vs fp64 oracle:", worst)
    assert not bad, bad


def test_training_step_in_split_mode_tracks_fp32_mode():
    """One training step at B=16 / 96 / 64 / 128 in mode bf16x3 and in mode f32 from the same seed: finite, every live
    parameter moves, loss within 1e-3 relative of mode 0's (a guard against a wrong product: the forward errors predict
    about 1e-5)."""
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd import train as T
    from tacotron2_subword_amd.hparams import create_hparams
    losses = {}
    for mode in ("f32", "bf16x3"):
        hps = create_hparams()
        L.set_precision(mode)
        try:
            model, opt, crit = T.make_training_objects(hps)
            model.train()
            x, y = model.parse_batch(T.synthetic_batch(hps, 16, 96, 64, 128, seed=7))
            before = {k: v.detach().clone() for k, v in model.named_parameters()}
            L.gemm_counts(reset=True)
            losses[mode] = float(T.train_step(model, crit, opt, x, y, hps, 0))
            torch.cuda.synchronize()
            counts = L.gemm_counts()
        finally:
            L.set_precision("f32")
        print(mode, "training step: loss", losses[mode], "gemm counts", counts)
        assert np.isfinite(losses[mode])
        assert counts[1] == counts[2] == 0 and (counts[3] > 0) == (mode == "bf16x3")
        for k, v in model.named_parameters():
            moved = not torch.equal(v.detach(), before[k])
            assert moved == (not k.startswith("decoder.decoder_rnn_bert")), k
    rel = abs(losses["bf16x3"] - losses["f32"]) / abs(losses["f32"])
    print("relative loss difference bf16x3 vs f32:", rel)
    assert rel < 1e-3, losses
