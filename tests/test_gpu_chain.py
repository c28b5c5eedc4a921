"""Persistent chain kernels (csrc/chain.hip) against the launch-per-step kernels they replace.

Both paths run the bf16-operand mode on the same inputs with the same RNG keys, so they differ only in summation
order, the hardware-exp tanh / sigmoid of the energies and (for memory rows resident in LDS) a bf16 copy of the
encoder memory in the context sum.  The launch-per-step path itself is pinned against the oracle / golden vectors by
test_gpu_decoder.py and test_gpu_model.py.  Reference semantics: model.py:322-428 (Decoder.decode / forward)."""
import os

import pytest
import torch

from helpers import LSA, SMA, hp_for, maxabs, to_dev
from oracle import recipe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from tacotron2_subword_amd import _lib as L, ops
    L.lib()
    yield L, ops
    L.set_precision("f32")
    L.set_chain(True)


def _inputs(B, Tin, Tsub, T, seed=5, ragged=True):
    g = torch.Generator().manual_seed(seed)
    mem = torch.randn(B, Tin, 512, generator=g) * 0.5
    mems = torch.randn(B, Tsub, 512, generator=g) * 0.5
    mels = torch.randn(B, 80, T, generator=g)
    if ragged:
        tl = torch.randint(max(1, Tin // 2), Tin + 1, (B,), generator=g); tl[0] = Tin
        bl = torch.randint(max(1, Tsub // 2), Tsub + 1, (B,), generator=g); bl[0] = Tsub
    else:
        tl, bl = torch.full((B,), Tin), torch.full((B,), Tsub)
    return [x.cuda() for x in (mem, mems, tl, bl, mels)]


def _plan(L, att, backward, B, Tin, Tsub, NS=2):
    """What the library's plan says for the attention chain of a pass on this device (t2_chain_plan: launches nothing)."""
    return L.chain_plan("sma" if att is SMA else "lsa", backward, NS=NS, B=B, Tin=(Tin, Tsub),
                        cus=torch.cuda.get_device_properties(0).multi_processor_count, claimed=bool(L.lib().t2_chain_claimed()))


def _run(env, att, B, Tin, Tsub, T, chain, training, seed=11, ragged=True):
    """-> outputs, status words, the pass's objects; _run.fwd_steps: per-step forward LSTM launches of the pass (exact, bf16, split)"""
    L, ops = env
    hp = hp_for(att)
    P = to_dev(recipe.make_weights(hp))
    dims = L.dims_from_hparams(hp)
    W = L.decoder_weights(P, dims.attention_kind)
    mem, mems, tl, bl, mels = _inputs(B, Tin, Tsub, T, ragged=ragged)
    L.set_precision("bf16")
    L.set_chain(chain)
    L.step_counts(reset=True)
    dp = ops.decoder_forward(W, dims, mem, mems, tl, bl, mels, training=training, prenet_dropout=training, seed=seed)
    torch.cuda.synchronize()
    _run.fwd_steps = L.step_counts()[:3]
    st = dp.chain_status()
    saved = {k: dp.view(k, n).clone() for k, n in (("ga", B * T * 4096), ("ca", B * T * 1024), ("din", B * T * 3072),
                                                    ("dout", B * T * 2048), ("qs", B * T * 128), ("gd", B * T * 4096), ("cd", B * T * 1024))}
    out = dict(mel=dp.mel.clone(), gate=dp.gate.clone(), align=dp.align.clone(), align_sub=dp.align_sub.clone(), **saved)
    return out, st, (W, P, dims, dp, mem, mems)


@pytest.mark.parametrize("att", [SMA, LSA])
@pytest.mark.parametrize("B,Tin,Tsub,T", [(3, 13, 9, 12), (33, 20, 11, 10), (64, 100, 60, 8), (128, 37, 22, 6)])
@pytest.mark.parametrize("training", [False, True])
def test_chain_matches_per_step_launches(env, att, B, Tin, Tsub, T, training):
    """Every tiling (B <= 32: one row tile, 8 units per item, context in 4 parts; B <= 64: 16 units, 2 parts; B <= 128: two
    row tiles, whole context rows), ragged memory lengths, with and without LSTM-state dropout + SMA noise.  The plan names the
    tiling, and the per-step launch counters show which path each run took."""
    plan = _plan(env[0], att, False, B, Tin, Tsub)
    assert plan["covered"], plan
    assert (plan["UT"], plan["RT"], plan["CS"]) == {3: (1, 1, 4), 33: (2, 1, 2), 64: (2, 1, 2), 128: (2, 2, 1)}[B], plan
    ref, st0, _ = _run(env, att, B, Tin, Tsub, T, chain=False, training=training)
    assert sum(_run.fwd_steps) > 0, _run.fwd_steps                     # one launch per step
    got, st1, _ = _run(env, att, B, Tin, Tsub, T, chain=True, training=training)
    assert _run.fwd_steps == (0, 0, 0), _run.fwd_steps                 # the persistent kernels took every step
    assert not any(st0) and not any(st1), (st0, st1)
    errs = {k: maxabs(got[k], ref[k]) for k in ref}
    print("chain vs launches, max-abs:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k in ("align", "align_sub"):
        assert errs[k] < 2e-3, errs
    for k in ("mel", "gate", "ga", "ca", "din", "dout", "qs", "gd", "cd"):
        assert errs[k] < 3e-2, errs
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


@pytest.mark.parametrize("att", [SMA, LSA])
def test_tiling_without_a_kernel_takes_the_per_step_launches(env, att):
    """One stream at 97-128 rows asks for the tiling UT = 1, RT = 2, which has no kernel instance: the plan refuses it with a
    reason of its own and the pass runs one launch per step, chains on or off, with the same bits.  (Before the plan existed the
    tiling was accepted and the pass failed on the host, ahead of any launch: "tiling UT=1 RT=2 not instantiated".)"""
    L, ops = env
    B, Tin, T = 97, 20, 4
    plan = _plan(L, att, False, B, Tin, 0, NS=1)
    assert not plan["covered"] and plan["reason_text"] == "the tiling of this shape has no kernel instance", plan
    hp = hp_for(att)
    P = to_dev(recipe.make_weights(hp, single=True))
    dims = L.dims_from_hparams(hp, n_streams=1)
    W = L.decoder_weights(P, dims.attention_kind, single=True)
    mem, _, tl, _, mels = _inputs(B, Tin, 4, T)
    L.set_precision("bf16")
    outs = {}
    for chain in (True, False):
        L.set_chain(chain)
        L.step_counts(reset=True)
        dp = ops.decoder_forward(W, dims, mem, None, tl, None, mels, training=False, prenet_dropout=False, seed=11)
        torch.cuda.synchronize()
        assert sum(L.step_counts()[:3]) > 0 and not any(dp.chain_status())
        outs[chain] = dict(mel=dp.mel.clone(), gate=dp.gate.clone(), align=dp.align.clone(), dout=dp.view("dout", B * T * 1536).clone())
    L.set_chain(True)
    for k, v in outs[False].items():
        assert bool(torch.isfinite(v).all()) and torch.equal(v, outs[True][k]), k


def test_chain_without_lds_residency_is_tight(env):
    """With nothing resident in LDS the context sum reads the fp32 memory like the launch path: what remains is summation
    order and the hardware exp, a much tighter bound over a short sequence."""
    os.environ["T2_CHAIN_NO_RESIDENT"] = "1"
    try:
        got, st1, _ = _run(env, SMA, 5, 17, 9, 6, chain=True, training=False)
    finally:
        del os.environ["T2_CHAIN_NO_RESIDENT"]
    ref, _, _ = _run(env, SMA, 5, 17, 9, 6, chain=False, training=False)
    assert not any(st1)
    errs = {k: maxabs(got[k], ref[k]) for k in ref}
    print("chain (no residency) vs launches, max-abs:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["align"] < 2e-4 and errs["align_sub"] < 2e-4 and errs["mel"] < 5e-3, errs


def test_chain_long_sequence_stays_close_to_fp32(env):
    """BASELINE-shaped pass (B=64, 100 phones, 60 sub-word tokens, 400 frames): the persistent path against the fp32
    parity path, within the documented bf16-mode bound (mel 0.03, gate 0.014, alignments 0.002 on
    the golden case; random inputs and weights here, so a looser cap)."""
    L, ops = env
    got, st, _ = _run(env, SMA, 64, 100, 60, 400, chain=True, training=False, ragged=True)
    assert not any(st)
    hp = hp_for(SMA)
    P = to_dev(recipe.make_weights(hp))
    dims = L.dims_from_hparams(hp)
    W = L.decoder_weights(P, dims.attention_kind)
    mem, mems, tl, bl, mels = _inputs(64, 100, 60, 400)
    L.set_precision("f32")
    dp = ops.decoder_forward(W, dims, mem, mems, tl, bl, mels, training=False, prenet_dropout=False, seed=11)
    torch.cuda.synchronize()
    errs = dict(mel=maxabs(got["mel"], dp.mel), gate=maxabs(got["gate"], dp.gate), align=maxabs(got["align"], dp.align),
                align_sub=maxabs(got["align_sub"], dp.align_sub))
    print("chain bf16 vs fp32 launches at B=64, T=400:", errs)
    assert errs["mel"] < 0.012 and errs["gate"] < 0.005 and errs["align"] < 0.004 and errs["align_sub"] < 0.004, errs    # observed 0.0045 / 0.0017 / 0.0012 / 0.0016
    # ... and against the ORACLE itself (the reference's arithmetic restated on the CPU), two items at full length: the
    # decoder has no cross-item arithmetic, so an item of the batch equals that item run alone
    from oracle import tacotron2_oracle as O
    Pc = recipe.make_weights(hp)
    idx = [5, 40]
    with torch.no_grad():
        mel, gate, al, alb = O.decoder_forward(mem[idx].cpu(), mems[idx].cpu(), mels[idx].cpu(), tl[idx].cpu(), bl[idx].cpu(), Pc, hp)
    eo = dict(mel=maxabs(got["mel"][idx].cpu().transpose(1, 2), mel), gate=maxabs(got["gate"][idx].cpu(), gate),
              align=maxabs(got["align"][idx][:, :, :al.shape[2]].cpu(), al), align_sub=maxabs(got["align_sub"][idx][:, :, :alb.shape[2]].cpu(), alb))
    print("chain bf16 vs the CPU oracle, items 5 and 40, T=400:", eo)
    assert eo["mel"] < 0.012 and eo["gate"] < 0.005 and eo["align"] < 0.004 and eo["align_sub"] < 0.004, eo


@pytest.mark.parametrize("att", [SMA, LSA])
def test_backward_chain_matches_per_step_backward(env, att):
    """Same forward (persistent chains), backward as persistent launches vs one launch per step and kernel: the two differ
    in summation order only (same bf16 operands, same RNG keys; LSA: the dloc product takes bf16 operands in the chain).
    LSA memories are long enough for two position splits with 15-row halos (the persistent LSA backward's geometry);
    the profile counters show that the persistent kernel really ran."""
    L, ops = env
    res = {}
    cases = ((8, 10, 40, 36), (64, 40 if att is SMA else 24, 100, 60))
    for B, T, Tin, Tsub in cases:
        assert _plan(L, att, True, B, Tin, Tsub)["covered"] and _plan(L, att, False, B, Tin, Tsub)["covered"]
        for bwd in (False, True):
            L.set_chain_bwd(bwd)
            try:
                out, st, (W, P, dims, dp, mem, mems) = _run(env, att, B, Tin, Tsub, T, chain=True, training=True)
                g = torch.Generator(device="cuda").manual_seed(3)
                dmel = torch.randn(B, T, 80, device="cuda", generator=g)
                dgate = torch.randn(B, T, device="cuda", generator=g)
                # external gradients on the alignments too (the alignment-guide losses of loss_function.py produce them)
                dal = 0.1 * torch.randn(B, T, Tin, device="cuda", generator=g)
                dals = 0.1 * torch.randn(B, T, Tsub, device="cuda", generator=g)
                assert _run.fwd_steps == (0, 0, 0), _run.fwd_steps
                L.prof_enable(8 * T + 64)
                L.step_counts(reset=True)
                G, dm, dms = ops.decoder_backward(W, P, dims, dp, mem, mems, dmel, dgate, training=True, prenet_dropout=True, seed=11,
                                                  d_align=dal, d_align_sub=dals)
                torch.cuda.synchronize()
                prof, grad_steps = L.prof_collect(), L.step_counts()[3:]
                assert not any(dp.chain_status()), dp.chain_status()
                assert prof["chain_a_bwd"][1] == (1 if bwd else 0), prof
                assert grad_steps == (0, 0, 0) if bwd else sum(grad_steps) > 0, grad_steps
            finally:
                L.set_chain_bwd(True)
            res[bwd] = dict(G, d_memory=dm, d_memory_sub=dms)
        worst = {}
        for k, v in res[False].items():
            if v is not None:
                worst[k] = float((res[True][k] - v).norm()) / (float(v.norm()) + 1e-12)
        print(f"{att} B={B} T={T}: relative gradient deviation, persistent vs per-step backward:", dict(sorted(worst.items(), key=lambda kv: -kv[1])[:4]))
        # (LSA: d(Wc) takes [w; cum] as bf16 operands in the chain, and cum grows with t: one operand rounding, 2^-8)
        assert max(worst.values()) < (5e-3 if att is SMA else 8e-3), worst


@pytest.mark.parametrize("att", [SMA, LSA])
def test_backward_consumes_chain_activations(env, att):
    """The hand-written BPTT reads what the persistent forward saved (gates, cells, DIN / DOUT rows, queries, selection
    probabilities / cumulative weights, alignments): gradients from a chain forward (+ for SMA the persistent backward)
    match gradients from the per-step path."""
    L, ops = env
    res = {}
    # (the 12-position memory is below the backward chain's 16, LSA's splits below the conv halo: forward on the chain, backward one
    #  launch per step)
    assert _plan(L, att, False, 8, 21, 12)["covered"] and not _plan(L, att, True, 8, 21, 12)["covered"]
    for chain in (False, True):
        out, st, (W, P, dims, dp, mem, mems) = _run(env, att, 8, 21, 12, 10, chain=chain, training=True)
        assert not any(st) and (_run.fwd_steps == (0, 0, 0) if chain else sum(_run.fwd_steps) > 0), _run.fwd_steps
        g = torch.Generator(device="cuda").manual_seed(3)
        dmel = torch.randn(8, 10, 80, device="cuda", generator=g)
        dgate = torch.randn(8, 10, device="cuda", generator=g)
        L.step_counts(reset=True)
        G, dm, dms = ops.decoder_backward(W, P, dims, dp, mem, mems, dmel, dgate, training=True, prenet_dropout=True, seed=11)
        torch.cuda.synchronize()
        assert sum(L.step_counts()[3:]) > 0
        res[chain] = dict(G, d_memory=dm, d_memory_sub=dms)
    worst = {}
    for k, v in res[False].items():
        if v is None:
            continue
        n = float(v.norm()) + 1e-12
        worst[k] = float((res[True][k] - v).norm()) / n
    print("relative gradient deviation chain vs launches:", dict(sorted(worst.items(), key=lambda kv: -kv[1])[:6]))
    assert max(worst.values()) < 0.008, worst                          # observed 0.0038


@pytest.mark.parametrize("att", [SMA, LSA])
def test_chains_are_bit_reproducible(env, att):
    """The hand-offs of the teacher-forced chains carry no counters: a consumer accepts a unit when its step tag fits.  A stale or
    torn unit that slipped through would change some output bit.  Same inputs, same seeds, forward + backward five times over
    (dropout and noise on; 64 x 100 / 60 positions, 40 steps — the tags of a parity buffer repeat every four steps): every output
    and every gradient bit-identical, and no status word set."""
    L, ops = env
    B, T, Tin, Tsub = 64, 40, 100, 60
    g = torch.Generator(device="cuda").manual_seed(3)
    dmel = torch.randn(B, T, 80, device="cuda", generator=g)
    dgate = torch.randn(B, T, device="cuda", generator=g)
    ref = None
    assert _plan(L, att, False, B, Tin, Tsub)["covered"] and _plan(L, att, True, B, Tin, Tsub)["covered"]
    for rep in range(5):
        out, st, (W, P, dims, dp, mem, mems) = _run(env, att, B, Tin, Tsub, T, chain=True, training=True)
        assert not any(st), st
        L.step_counts(reset=True)
        G, dm, dms = ops.decoder_backward(W, P, dims, dp, mem, mems, dmel, dgate, training=True, prenet_dropout=True, seed=11)
        torch.cuda.synchronize()
        assert _run.fwd_steps == (0, 0, 0) and L.step_counts()[3:] == (0, 0, 0), (_run.fwd_steps, L.step_counts())
        assert not any(dp.chain_status()), dp.chain_status()
        cur = dict(out, **{"grad_" + k: v for k, v in G.items()}, d_memory=dm, d_memory_sub=dms)
        if ref is None:
            ref = {k: v.clone() for k, v in cur.items() if v is not None}
        else:
            for k, v in ref.items():
                assert torch.equal(v, cur[k]), (rep, k, float((v - cur[k]).abs().max()))


def test_lsa_backward_after_a_launch_path_forward(env):
    """The LSA backward chain reads the tanh tile and the location features the forward CHAIN saved (layout.usave / locsave).  A
    forward that ran one launch per step leaves them unwritten: its backward must take the launch path even with the chains on
    (the library keeps, per workspace, whether the tile was saved) — same gradients as with the chains off, bit for bit, and no
    persistent attention backward in the profile.  A chain forward right after, into a fresh workspace, gets the chain backward."""
    L, ops = env
    B, T, Tin, Tsub = 64, 12, 100, 60
    g = torch.Generator(device="cuda").manual_seed(3)
    dmel = torch.randn(B, T, 80, device="cuda", generator=g)
    dgate = torch.randn(B, T, device="cuda", generator=g)
    res, launches = {}, {}
    for name, fwd_chain, bwd_chain in (("launch/launch", False, False), ("launch/chain-enabled", False, True), ("chain/chain", True, True)):
        out, st, (W, P, dims, dp, mem, mems) = _run(env, LSA, B, Tin, Tsub, T, chain=fwd_chain, training=True)
        L.set_chain(bwd_chain)
        try:
            L.prof_enable(8 * T + 64)
            G, dm, dms = ops.decoder_backward(W, P, dims, dp, mem, mems, dmel, dgate, training=True, prenet_dropout=True, seed=11)
            torch.cuda.synchronize()
            launches[name] = L.prof_collect()["chain_a_bwd"][1]
        finally:
            L.set_chain(True)
        res[name] = dict(G, d_memory=dm, d_memory_sub=dms)
    assert launches == {"launch/launch": 0, "launch/chain-enabled": 0, "chain/chain": 1}, launches
    for k, v in res["launch/launch"].items():
        if v is not None:
            assert torch.equal(v, res["launch/chain-enabled"][k]), k


def test_reported_abort_raises_at_every_entry_point(env):
    """The sticky status word (page-locked host memory the device writes directly): an abort report is seen by the next
    entry point without any copy or synchronisation of its own, and the raise clears it."""
    L, ops = env
    ops.check_chain_status(block=True)                               # (whatever earlier tests left behind)
    out, st, (W, P, dims, dp, mem, mems) = _run(env, SMA, 8, 21, 12, 6, chain=True, training=True)
    assert not any(st) and ops.chain_status_words() == (0, 0, 0, 0)
    ops.check_chain_status()                                         # clean: a no-op
    ops.debug_report_abort(7)                                        # as a timed-out hand-off reports
    torch.cuda.synchronize()
    assert ops.chain_status_words()[0] == 7
    with pytest.raises(RuntimeError, match="persistent chain"):
        ops.decoder_forward(W, dims, mem, mems, None, None, torch.zeros(8, 80, 6, device="cuda"), training=False, prenet_dropout=False, seed=1)
    assert ops.chain_status_words() == (0, 0, 0, 0)                  # the raise cleared it: the caller may carry on
    ops.check_chain_status(block=True)


def _tiny_training_objects():
    from tacotron2_subword_amd import train as T
    from tacotron2_subword_amd.hparams import create_hparams
    hp = create_hparams()
    hp.distributed_run = False
    model, opt, crit = T.make_training_objects(hp)
    model.train()
    x, y = model.parse_batch(T.synthetic_batch(hp, 8, 24, 16, 40, seed=3))
    return T, hp, model, opt, crit, x, y


def test_reported_abort_skips_the_optimizer_step(env):
    """an aborted chain's gradients must never reach the parameters.  The optimizer kernels read the
    sticky word on the device, so the step that follows the abort changes nothing even though the host has not looked
    yet; the host raises at its next look; after that training carries on."""
    L, ops = env
    L.set_precision("bf16"); L.set_chain(True)
    ops.check_chain_status(block=True)
    T, hp, model, opt, crit, x, y = _tiny_training_objects()
    for it in range(2):                                               # Adam state exists, the fast path is warm
        T.train_step(model, crit, opt, x, y, hp, it)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in model.state_dict().items() if v.is_floating_point() and "running" not in k}
    m_before = [opt.state[p]["exp_avg"].clone() for p in model.parameters() if p in opt.state]
    model.zero_grad()
    loss = crit(model(x), y, x, 2)[0]
    loss.backward()
    torch.cuda._sleep(400_000_000)                                    # (the device is busy for a moment: what follows is enqueued, not yet run)
    ops.debug_report_abort(12)                                        # "the backward attention chain timed out" — enqueued, the host does not know
    opt.step(max_norm=hp.grad_clip_thresh)                            # no raise here: the report has not run when the host looks
    torch.cuda.synchronize()
    after = model.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items()), "a parameter moved on invalid gradients"
    assert all(torch.equal(a, b) for a, b in zip(m_before, [opt.state[p]["exp_avg"] for p in model.parameters() if p in opt.state]))
    with pytest.raises(RuntimeError, match="persistent chain"):
        T.train_step(model, crit, opt, x, y, hp, 3)                   # the next look (first entry point of the next step)
    T.train_step(model, crit, opt, x, y, hp, 3)                       # status cleared by the raise: training carries on
    torch.cuda.synchronize()
    assert any(not torch.equal(model.state_dict()[k], v) for k, v in before.items())
    ops.check_chain_status(block=True)


@pytest.mark.parametrize("mode", ["no_grad_forward", "inference"])
def test_chain_starved_of_cus_aborts_loudly(env, mode):
    """The real failure: a foreign kernel holds CUs, so the persistent grid is never whole; its hand-offs time out after
    1 s (bounded spins), the grid drains, and (1) the outputs of the pass are NaN, (2) the sticky status is set, (3) the
    host raises at its next look — under no_grad (GTA, validation) and in Decoder.inference just as in training."""
    L, ops = env
    from tacotron2_subword_amd.hparams import create_hparams
    from tacotron2_subword_amd.model import BERT_Tacotron2
    from tacotron2_subword_amd import train as T
    if not L.lib().t2_chain_claimed():
        pytest.skip("another process holds this GPU's persistent-kernel claim")
    L.set_precision("bf16"); L.set_chain(True)
    ops.check_chain_status(block=True)
    hp = create_hparams()
    model = BERT_Tacotron2(hp).cuda().eval()
    b = T.synthetic_batch(hp, 8, 24, 16, 12, seed=4)
    # the foreign kernel comes from ANOTHER PROCESS (its own hardware queues: two streams of one process may share a queue
    # and then simply run one after the other): 96 CUs gone for 3 s
    import subprocess, sys, time
    child = subprocess.Popen([sys.executable, "-c",
                              "import ctypes, sys\n"
                              f"lib = ctypes.CDLL({L.LIB_PATH!r})\n"
                              "lib.t2_debug_occupy.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]\n"
                              "rc = lib.t2_debug_occupy(96, 3000, None)\n"
                              "print('started', rc, flush=True)\n"
                              "ctypes.CDLL('libamdhip64.so').hipDeviceSynchronize()\n"], stdout=subprocess.PIPE, text=True)
    assert child.stdout.readline().split() == ["started", "0"]
    time.sleep(0.2)                                                            # the blocker is resident before the pass is enqueued
    with torch.no_grad():
        if mode == "no_grad_forward":
            x, _ = model.parse_batch(b)
            out = model(x)
            torch.cuda.synchronize()
            assert bool(torch.isnan(out[0][0]).all()) and bool(torch.isnan(out[2][0]).all())      # (item 0 has no padding frames; padding is filled after)
            with pytest.raises(RuntimeError, match="persistent chain"):
                ops.check_chain_status()
        else:
            model.decoder.max_decoder_steps, model.decoder.gate_threshold = 16, 2.0
            with pytest.raises(RuntimeError, match="persistent chain"):
                model.inference(b[0].cuda(), b[6].cuda(), b[7].cuda(), b[8].cuda())
    torch.cuda.synchronize()
    assert child.wait(timeout=30) == 0
    ops.check_chain_status(block=True)                                         # cleared; nothing else pending
    with torch.no_grad():                                                      # and the device is fine afterwards
        x, _ = model.parse_batch(b)
        out = model(x)
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out[0]).all())
    ops.check_chain_status(block=True)
