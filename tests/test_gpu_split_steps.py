"""GPU: the split-bf16 recurrent steps (t2_set_split_steps in precision mode "bf16x3"): the per-step products of the
attention LSTMs and the decoder LSTM, and the recurrent-input gradients of their BPTT, as three bf16 MFMA terms with fp32
accumulation.  Yardsticks: fp64 on the CPU from the operands each run saved (the bound of tests/split_steps_ref.py, checked
without a GPU in tests/test_split_steps_cpu.py), the CPU oracle at the project's 1e-4, fp64 oracle autograd, and the exact
modes on the same inputs.  Every test restores the mode and the switch."""
import contextlib
import functools

import pytest
import torch

from oracle import recipe
from oracle import tacotron2_oracle as O

from helpers import LSA, SMA, hp_for, load_golden, maxabs, to_dev
from split_steps_ref import bf16_product_bound, product_bound, step_gates_fp64

pytestmark = pytest.mark.gpu
TOL = 1e-4
NAMES = ("mel", "mel_postnet", "gate", "align", "align_bert")
HA, HD, E, P = 1024, 1024, 512, 256
WD, WO = 2 * (HA + E), HD + 2 * E


class mode:
    """with mode("bf16x3", True): ... — precision mode and split-steps switch, restored on the way out"""

    def __init__(self, precision, split):
        self.precision, self.split = precision, split

    def __enter__(self):
        from tacotron2_subword_amd import _lib as L
        L.set_precision(self.precision)
        L.set_split_steps(self.split)

    def __exit__(self, *exc):
        from tacotron2_subword_amd import _lib as L
        L.set_split_steps(False)
        L.set_precision("f32")


@contextlib.contextmanager
def chain_off():
    """per-step launches instead of the persistent chains; the switch is back on afterwards, also on failure"""
    from tacotron2_subword_amd import _lib as L
    L.set_chain(False)
    try:
        yield
    finally:
        L.set_chain(True)


@functools.lru_cache(maxsize=None)
def weights(att):
    return recipe.make_weights(hp_for(att))


@functools.lru_cache(maxsize=None)
def device_weights(att):
    from tacotron2_subword_amd import _lib as L
    Pd = to_dev({k: v for k, v in weights(att).items() if k.startswith("decoder.")})
    return Pd, L.decoder_weights(Pd, L.dims_from_hparams(hp_for(att)).attention_kind)


def build_model(att, train=False):
    from tacotron2_subword_amd.hparams import create_hparams
    from tacotron2_subword_amd.model import BERT_Tacotron2
    hps = create_hparams()
    hps.attention = att
    m = BERT_Tacotron2(hps)
    m.load_state_dict(weights(att))
    m = m.cuda()
    m.train(train)
    m.decoder.prenet_dropout = False
    return m


# ------------------------------------------------------------------------------------------------ 1. forward kernel
def decoder_run(att, B, T, Tin, Tsub, training, seed):
    """One teacher-forced decoder pass on random memories with ragged lengths in the mode in force -> what it saved, on the
    CPU, and the counters of the pass."""
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd import ops
    g = torch.Generator().manual_seed(100 * B + T)
    mem, sub = torch.randn(B, Tin, E, generator=g) * 0.5, torch.randn(B, Tsub, E, generator=g) * 0.5
    mels = torch.randn(B, 80, T, generator=g)
    tl = torch.randint(1, Tin + 1, (B,), generator=g); tl[0] = Tin
    bl = torch.randint(1, Tsub + 1, (B,), generator=g); bl[0] = Tsub
    Pd, W = device_weights(att)
    dims = L.dims_from_hparams(hp_for(att))
    L.step_counts(reset=True); L.gemm_counts(reset=True)
    dp = ops.decoder_forward(W, dims, mem.cuda(), sub.cuda(), tl.cuda(), bl.cuda(), mels.cuda(), training=training,
                             prenet_dropout=False, seed=seed, keep=Pd)
    torch.cuda.synchronize()
    saved = {k: dp.view(k, T, B, w).cpu() for k, w in (("din", WD), ("dout", WO), ("prea", 4 * HA), ("preas", 4 * HA), ("pred", 4 * HD),
                                                       ("ga", 4 * HA), ("gas", 4 * HA), ("gd", 4 * HD), ("cna", HA), ("cnas", HA),
                                                       ("cnd", HD), ("ca", HA), ("cas", HA), ("cd", HD))}
    return saved, L.step_counts(), L.gemm_counts()


def gate_errors(att, S, T, family="split"):
    """Per cell (attention LSTM, its sub-word twin, decoder LSTM) and step: |saved activated gates - fp64 gates| and the bound
    of the recurrent product, both [B,4H]; the fp64 gates come from the run's OWN saved rows of step t-1 and hoisted
    pre-activations.  Also |saved cell - fp64 cell| from the fp64 gates and the saved previous cell, with its bound.
    family "bf16": the fp64 product is taken over the operands that kernel reads, the bf16 roundings (nearest even) of the
    saved rows and of the weights, under bf16_product_bound."""
    Wt = weights(att)
    cells = [("att", "prea", "ga", "cna", "ca", lambda t: S["din"][t][:, :HA + E],
              torch.cat([Wt["decoder.attention_rnn.weight_hh"], Wt["decoder.attention_rnn.weight_ih"][:, P:]], 1)),
             ("att_sub", "preas", "gas", "cnas", "cas", lambda t: S["din"][t][:, HA + E:],
              torch.cat([Wt["decoder.attention_rnn_bert.weight_hh"], Wt["decoder.attention_rnn_bert.weight_ih"][:, P:]], 1)),
             ("dec", "pred", "gd", "cnd", "cd", lambda t: S["dout"][t][:, :HD], Wt["decoder.decoder_rnn.weight_hh"])]
    operand = (lambda v: v.to(torch.bfloat16).float()) if family == "bf16" else (lambda v: v)
    bound_fn = bf16_product_bound if family == "bf16" else product_bound
    out = []
    for name, pre, gates, cnew, cout, rows, w in cells:
        w = operand(w)
        for t in range(T):
            g64, bound = step_gates_fp64(S[pre][t], operand(rows(t - 1)) if t > 0 else None, w, bound_fn)
            H = g64.shape[1] // 4
            cp = S[cout][t - 1].double() if t > 0 else torch.zeros_like(g64[:, :H])
            c64 = g64[:, H:2 * H] * cp + g64[:, :H] * g64[:, 2 * H:3 * H]
            # d(cell) <= |c_prev| d(f) + |g| d(i) + |i| d(g) <= (|c_prev| + 2) * the gates' bound (largest of the three columns)
            cb = (cp.abs() + 2) * torch.maximum(torch.maximum(bound[:, :H], bound[:, H:2 * H]), bound[:, 2 * H:3 * H])
            out.append((name, t, (S[gates][t].double() - g64).abs(), bound, (S[cnew][t].double() - c64).abs(), cb))
    return out


# the split cases keep the ids they had before the test took a family
@pytest.mark.parametrize("family,B,att,training", [
    pytest.param(family, B, att, training, id=("" if family == "split" else family + "-") + f"{B}-{att}-{training}")
    for family in ("split", "bf16") for B in (1, 33, 65) for att in (SMA, LSA) for training in (False, True)])
def test_forward_split_steps_against_fp64_step_by_step(family, B, att, training):
    """B = 1 / 33 / 65 (one row tile; a partly filled second; four with a partly filled third), T = 3, Tin / Tsub = 7 / 5,
    ragged lengths.  Every step's activated gates (t = 0 included: no recurrent operand, same kernel) within
    8 * 2^-17 * sqrt(sum x^2 w^2) of the recurrent product + a floor of twice the largest error the MODE-0 run shows against
    the same fp64 formula in this test; the counters prove which kernels ran; with dropout on, the zeros of h and c are the
    keep-bits of mode 0's RNG indices.
    family "bf16": the per-step launches of precision mode "bf16" with the persistent chains off (the bf16-operand step
    kernel, otherwise only ever compared with the chain).  Its operands are exactly the bf16 roundings of the saved fp32
    rows and of the weights (the shadows are cast_rows_bf16 of [W_hh | W_ih[:, P:]] / W_hh; the producing kernels store
    (__bf16)h and (__bf16)ctx next to the fp32 values), so the fp64 product is taken over those and the bound is the
    accumulation's alone: (K + 16) * 2^-23 * sum |x||w| + the same floor.  At the default dims the attention LSTMs run an
    odd number of 512-wide stages (K = 1536) and the decoder LSTM an even one (1024): both exits of the two-deep stage
    pipeline, and t = 0 runs none."""
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd import ops
    T, Tin, Tsub, seed = 3, 7, 5, 20240607
    with mode("f32", False):
        S0, sc0, _ = decoder_run(att, B, T, Tin, Tsub, training, seed)
    if family == "split":
        with mode("bf16x3", True):
            S2, sc2, gc2 = decoder_run(att, B, T, Tin, Tsub, training, seed)
    else:
        with mode("bf16", False), chain_off():
            S2, sc2, gc2 = decoder_run(att, B, T, Tin, Tsub, training, seed)
    assert sc0 == (2 * T, 0, 0, 0, 0, 0), sc0
    if family == "split":
        assert sc2 == (0, 0, 2 * T, 0, 0, 0), sc2                        # attention LSTMs (both streams in one launch) + decoder LSTM
        assert gc2[1] == gc2[2] == 0, gc2
    else:
        assert sc2 == (0, 2 * T, 0, 0, 0, 0), sc2
    e0 = gate_errors(att, S0, T)
    floor_g = 2 * max(float(eg.max()) for _, _, eg, _, _, _ in e0)
    floor_c = 2 * max(float(ec.max()) for _, _, _, _, ec, _ in e0)
    worst_g = worst_c = 0.0
    for name, t, eg, bound, ec, cb in gate_errors(att, S2, T, family):
        rg, rc = float((eg / (bound + floor_g)).max()), float((ec / (cb + floor_c)).max())
        print(f"{family} B={B} {att} training={training} {name} t={t}: gate error / bound {rg:.3f} (max error {float(eg.max()):.2e}, "
              f"floor {floor_g:.2e})  cell error / bound {rc:.3f}")
        worst_g, worst_c = max(worst_g, rg), max(worst_c, rc)
        assert rg < 1 and rc < 1, (name, t, rg, rc)
    print(f"{family} B={B} {att} training={training}: worst gate error / bound {worst_g:.3f}, worst cell error / bound {worst_c:.3f}")
    if training:
        for site, p, key, cols in (("ATT_H", 0.1, "din", slice(0, HA)), ("ATT_H_SUB", 0.1, "din", slice(HA + E, 2 * HA + E)),
                                   ("DEC_H", 0.1, "dout", slice(0, HD)), ("ATT_C", 0.1, "ca", slice(0, HA)),
                                   ("ATT_C_SUB", 0.1, "cas", slice(0, HA)), ("DEC_C", 0.1, "cd", slice(0, HD))):
            keep = ops.rng_keep_mask(seed, L.SITE[site], T * B * HA, p).view(T, B, HA).bool().cpu()
            assert torch.equal(S2[key][:, :, cols] != 0, keep), site
            assert torch.equal(S0[key][:, :, cols] != 0, keep), site


# ------------------------------------------------------------------------------------------------ 2. whole pass
@pytest.mark.parametrize("att", [SMA, LSA])
def test_whole_pass_split_steps_vs_oracle_and_fp32_mode(att):
    """Eval forward at B=16, Tin=96, Tsub=64, T=128 (the shape of tests/test_gpu_split_model.py), ragged lengths: all five
    outputs within 1e-4 of the oracle and of mode 0; every per-step LSTM launch of the pass was a split one."""
    from tacotron2_subword_amd import _lib as L
    hp = hp_for(att)
    B, Tin, Tsub, T = 16, 96, 64, 128
    m = build_model(att)
    batch = recipe.make_batch(hp, B, Tin, Tsub, T)
    x, y = m.parse_batch(batch)
    with torch.no_grad():
        with mode("f32", False):
            out0 = [o.detach().clone() for o in m(x)]
        with mode("bf16x3", True):
            L.step_counts(reset=True); L.gemm_counts(reset=True)
            out3 = [o.detach().clone() for o in m(x)]
            sc, gc = L.step_counts(), L.gemm_counts()
        xo, _ = recipe.parse_batch(batch)
        ref = O.forward(weights(att), hp, xo, training=False)
    e_or = {k: maxabs(a, b) for k, a, b in zip(NAMES, out3, ref)}
    e_32 = {k: maxabs(a, b) for k, a, b in zip(NAMES, out3, out0)}
    print(att, "step counts", sc, "gemm counts", gc)
    print(att, "split steps vs oracle:", e_or)
    print(att, "split steps vs f32 mode:", e_32)
    assert sc == (0, 0, 2 * T, 0, 0, 0), sc                              # the decoder's: the encoders' BiLSTMs are not counted
    assert gc[1] == gc[2] == 0 and gc[3] > 0, gc
    for k in NAMES:
        assert e_or[k] < TOL, (k, e_or)
        assert e_32[k] < TOL, (k, e_32)


# ------------------------------------------------------------------------------------------------ 3. backward
def oracle_grads(att, batch, dt):
    hp = hp_for(att)
    Pw = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in recipe.make_weights(hp).items()}
    for k, v in Pw.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    cast = lambda ts: tuple(t.to(dt) if torch.is_tensor(t) and t.is_floating_point() else t for t in ts)
    xo, yo = recipe.parse_batch(batch)
    lo = O.loss(O.forward(Pw, hp, cast(xo), training=False), cast(yo))[0]
    lo.backward()
    return float(lo.detach()), {k: (None if v.grad is None else v.grad.double()) for k, v in Pw.items() if v.is_floating_point()}


def model_grads(att, batch):
    """loss and gradients of the whole model in the mode in force, + the counters of the backward pass"""
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd.loss_function import Tacotron2Loss
    m = build_model(att, train=False)
    x, y = m.parse_batch(batch)
    out = m(x)
    loss = Tacotron2Loss()(out, y, x)[0]
    L.step_counts(reset=True); L.gemm_counts(reset=True)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), {k: (None if p.grad is None else p.grad.double().cpu()) for k, p in m.named_parameters()}, L.step_counts(), L.gemm_counts()


@pytest.mark.parametrize("att", [SMA, LSA])
def test_backward_split_steps_vs_oracle_autograd(att):
    """The recipe of test_backward_split_vs_oracle_autograd (fp64 oracle autograd as truth, max(5e-4, 3 x the fp32 oracle's
    own error) relative per parameter, loss within 1e-5 relative) at B=8 / 64 / 32 / 64 with the switch on: every
    recurrent-input gradient product of the BPTT was a split launch, the dead decoder_rnn_bert keeps grad None."""
    B, Tin, Tsub, T = 8, 64, 32, 64
    batch = recipe.make_batch(hp_for(att), B, Tin, Tsub, T)
    with mode("bf16x3", True):
        loss, grads, sc, gc = model_grads(att, batch)
    lo32, g32 = oracle_grads(att, batch, torch.float32)
    _, g64 = oracle_grads(att, batch, torch.float64)
    print(att, "backward step counts", sc, "gemm counts", gc, " loss", loss, "oracle fp32 loss", lo32)
    assert sc == (0, 0, 0, 0, 0, 2 * (T - 1)), sc                        # attention + decoder chain; step 0 has no recurrent input
    assert gc[1] == gc[2] == 0, gc
    assert abs(loss - lo32) < 1e-5 * max(1.0, abs(lo32))
    bad, worst = {}, (0.0, None)
    for k, g in grads.items():
        ref = g64[k]
        if ref is None:
            assert g is None, k
            continue
        scale = max(float(ref.abs().max()), 1e-7)
        err = float((g - ref).abs().max()) / scale
        noise = float((g32[k] - ref).abs().max()) / scale
        worst = max(worst, (err, k))
        if not err < max(5e-4, 3 * noise):
            bad[k] = (err, noise)
    print(att, "worst relative gradient error vs fp64 oracle:", worst)
    assert grads["decoder.decoder_rnn_bert.weight_hh"] is None
    assert not bad, bad


@pytest.mark.parametrize("B", [33, 65])
def test_backward_split_steps_at_row_tile_edges_track_the_switch_off_run(B):
    """B = 33 / 65 (a partly filled second / third row tile: the MT = 2 and MT = 4 gradient kernels), T = 3, SMA: every
    gradient of the switch-on run agrees with the switch-off mode-2 run on the same inputs under the criterion of the test
    above — relative to the fp64 oracle gradient's largest entry, below max(5e-4, 3 x the fp32 oracle's own error).  The
    encoders' gradients are d_memory / d_memory_sub carried on, so they cover those two."""
    Tin, Tsub, T = 7, 5, 3
    batch = recipe.make_batch(hp_for(SMA), B, Tin, Tsub, T)
    with mode("bf16x3", False):
        _, g_off, sc_off, _ = model_grads(SMA, batch)
    with mode("bf16x3", True):
        _, g_on, sc_on, _ = model_grads(SMA, batch)
    _, g32 = oracle_grads(SMA, batch, torch.float32)
    _, g64 = oracle_grads(SMA, batch, torch.float64)
    assert sc_off == (0, 0, 0, 2 * (T - 1), 0, 0) and sc_on == (0, 0, 0, 0, 0, 2 * (T - 1)), (sc_off, sc_on)
    bad, worst = {}, (0.0, None)
    for k, g in g_on.items():
        ref = g64[k]
        if ref is None:
            assert g is None and g_off[k] is None, k
            continue
        scale = max(float(ref.abs().max()), 1e-7)
        err = float((g - g_off[k]).abs().max()) / scale
        noise = float((g32[k] - ref).abs().max()) / scale
        worst = max(worst, (err, k))
        if not err < max(5e-4, 3 * noise):
            bad[k] = (err, noise)
    print(f"B={B}: worst relative gradient difference switch on vs off:", worst)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 4. nothing else moves
def test_nothing_else_moves():
    """At the B = 2 golden shape (no product qualifies for the split GEMM path): mode 2 with the switch off is bit-identical
    to mode 0; modes 0 and 1 with the switch ON are bit-identical to themselves with it off and launch no split step;
    inference() in mode 2 with the switch on reproduces the sma_infer golden's stop frame exactly."""
    from tacotron2_subword_amd import _lib as L
    g = load_golden("sma_small_eval")
    B, Tin, Tsub, T, _ = (int(v) for v in g["meta"])
    m = build_model(SMA)
    x, y = m.parse_batch(recipe.make_batch(hp_for(SMA), B, Tin, Tsub, T))

    def run(precision, split):
        with mode(precision, split), torch.no_grad():
            L.step_counts(reset=True)
            out = [o.detach().clone() for o in m(x)]
            torch.cuda.synchronize()
            return out, L.step_counts()
    base, _ = run("f32", False)
    off2, sc = run("bf16x3", False)
    assert sc[2] == sc[5] == 0
    for k, a, b in zip(NAMES, off2, base):
        assert torch.equal(a, b), k
    for precision in ("f32", "bf16"):
        a_off, _ = run(precision, False)
        a_on, sc = run(precision, True)
        assert sc[2] == sc[5] == 0, (precision, sc)
        for k, a, b in zip(NAMES, a_on, a_off):
            assert torch.equal(a, b), (precision, k)
    on2, sc = run("bf16x3", True)
    assert sc[2] == 2 * T
    for k, a in zip(NAMES, on2):
        assert maxabs(a, g[k]) < TOL, k

    gi = load_golden("sma_infer")
    _, Tin, Tsub, steps = (int(v) for v in gi["meta"])
    b = recipe.make_batch(hp_for(SMA), 1, Tin, Tsub, 8, seed=4321, ragged=False)
    ids, sub, pcls, bcls = b[0].cuda(), b[6].cuda(), b[7].cuda(), b[8].cuda()
    with mode("bf16x3", True):
        L.step_counts(reset=True)
        m.decoder.gate_threshold, m.decoder.max_decoder_steps = float(gi["stop_threshold"]), 1000
        r = m.inference(ids, sub, pcls, bcls)
        torch.cuda.synchronize()
        sc = L.step_counts()
    assert sc[2] == 0 and sc[0] > 0, sc                                  # the decode loop keeps the exact step kernel
    assert r[5] is True and r[0].shape[2] - 1 == int(gi["stop_index"])
    assert maxabs(r[0], gi["stop_mel"]) < TOL and maxabs(r[1], gi["stop_mel_postnet"]) < TOL


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_split_steps_are_deterministic():
    """Two switch-on training-mode passes (dropout and SMA noise on) from the same seed: identical outputs and gradients."""
    from tacotron2_subword_amd.loss_function import Tacotron2Loss
    B, Tin, Tsub, T = 33, 9, 6, 4
    batch = recipe.make_batch(hp_for(SMA), B, Tin, Tsub, T)
    runs = []
    with mode("bf16x3", True):
        for _ in range(2):
            m = build_model(SMA, train=True)
            x, y = m.parse_batch(batch)
            out = m(x)
            Tacotron2Loss()(out, y, x)[0].backward()
            torch.cuda.synchronize()
            runs.append(([o.detach().clone() for o in out], {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    for k, a, b in zip(NAMES, runs[0][0], runs[1][0]):
        assert torch.equal(a, b), k
    assert runs[0][1].keys() == runs[1][1].keys()
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
