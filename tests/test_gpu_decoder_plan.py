"""The decoder drivers do what their plan says (csrc/decoder_plan.hip -> csrc/decoder.hip).

For each case the plan is read first (t2_decoder_pass_plan with this device's facts and the switches the case sets: nothing is
launched), then the pass runs once under the in-situ profile, and what ran is compared with what the plan implies: launches per
kind (a persistent chain: one per step range; per-step kernels: one per step, or none), the per-step LSTM launch counters by
family, the deferred-tail counter and the number of products.  A second run gives the same bits.  The smallest shapes that reach
each branch; default dims wherever a chain is meant to run (the chains take no other)."""
import pytest
import torch

from helpers import LSA, SMA, hp_for, tiny_hp, to_dev
from oracle import recipe

pytestmark = pytest.mark.gpu
FAMILY = {(False, False): 0, (True, False): 1, (False, True): 2}            # (use16, split) -> exact, bf16, split


@pytest.fixture(scope="module")
def env():
    from tacotron2_subword_amd import _lib as L, ops
    L.lib()
    yield L, ops
    L.set_precision("f32"); L.set_chain(True); L.set_chain_bwd(True); L.lib().t2_set_overlap(1)


def _setup(L, hp, NS, B, Tin, Tsub, T, seed=5):
    single = NS == 1
    P = to_dev(recipe.make_weights(hp, single=single)) if single else to_dev(recipe.make_weights(hp))
    dims = L.dims_from_hparams(hp, n_streams=NS)
    W = L.decoder_weights(P, dims.attention_kind, single=True) if single else L.decoder_weights(P, dims.attention_kind)
    g = torch.Generator().manual_seed(seed)
    E, M = hp["encoder_embedding_dim"], dims.n_mel
    mem = (torch.randn(B, Tin, E, generator=g) * 0.5).cuda()
    mems = None if single else (torch.randn(B, Tsub, E, generator=g) * 0.5).cuda()
    tl = torch.full((B,), Tin).cuda()
    bl = None if single else torch.full((B,), Tsub).cuda()
    mels = torch.randn(B, M, T, generator=g).cuda()
    return P, dims, W, mem, mems, tl, bl, mels


def _plan(L, dims, kind, B, T, Tin, Tsub, precision, chain, chain_bwd=True, overlap=True, **kw):
    return L.decoder_pass_plan(dims, kind, B, T, Tin, Tsub, precision=precision, split_steps=L.get_split_steps(), chain=chain, chain_bwd=chain_bwd, overlap=overlap,
                               cus=torch.cuda.get_device_properties(0).multi_processor_count, claimed=bool(L.lib().t2_chain_claimed()), **kw)


def _measured(L, fn, T):
    L.step_counts(reset=True); L.gemm_counts(reset=True); L.defer_counts(reset=True)
    L.prof_enable(8 * T + 64)
    out = fn()
    torch.cuda.synchronize()
    prof = {k: v[1] for k, v in L.prof_collect().items()}
    return out, prof, L.step_counts(reset=True), L.gemm_counts(reset=True), L.defer_counts(reset=True)


def _content(dims, L):
    return dims.attention_kind in (L.ATTN_SMA, L.ATTN_LSA)


def _check_forward(L, dims, p, T, NS, prof, steps, gemms, precision):
    ranges = len(p["bounds"]) - 1
    a, b = p["chain_a"]["on"], p["chain_b"]["on"]
    want = dict(chain_a_fwd=ranges if a else 0, att_lstm_fwd=0 if a else T, attention_fwd=0 if a else T,
                chain_b_fwd=ranges if b else 0, dec_lstm_fwd=0 if b else T)
    assert {k: prof[k] for k in want} == want, (prof, p)
    fam = [0, 0, 0]
    fam[FAMILY[(p["use16"], p["split"])]] = (0 if a else T) + (0 if b else T)
    assert list(steps[:3]) == fam and not any(steps[3:]), (steps, p)
    products = 2 * NS + NS + (NS if _content(dims, L) else 0) + ranges + 2      # prenets, hoisted att input, processed memory, dec input per range, projections
    assert sum(gemms) == products and (precision != "f32" or gemms[1:] == (0, 0, 0)) and (precision == "bf16x3" or gemms[3] == 0), (gemms, products)


def _check_backward(L, dims, p, T, NS, prof, steps, gemms, defers, precision):
    ranges = len(p["bounds"]) - 1
    a, b = p["chain_a"]["on"], p["chain_b"]["on"]
    want = dict(chain_b_bwd=ranges if b else 0, dec_lstm_bwd_pointwise=0 if b else T, dec_lstm_bwd_gemm=0 if b else T - 1,
                chain_a_bwd=ranges if a else 0, attention_bwd=0 if a else T, att_lstm_bwd_pointwise=0 if a else T, att_lstm_bwd_gemm=0 if a else T - 1)
    assert {k: prof[k] for k in want} == want, (prof, p)
    fam = [0, 0, 0]
    fam[FAMILY[(p["use16"], p["split"])]] = (0 if a else T - 1) + (0 if b else T - 1)
    assert list(steps[3:]) == fam and not any(steps[:3]), (steps, p)
    assert defers == ((1, 0) if p["defer"] else (0, 1)) and p["tail_on_side"] == p["defer"], (defers, p)
    content = 1 if _content(dims, L) else 0
    # projections (gate term folded into the mel product) 1 + 2, dDIN per range, dec-LSTM dW_ih + dW_hh, per stream: d(memory) and the tail
    products = 3 + ranges + (2 if T > 1 else 1) + NS * (content + 1) + NS * ((3 if T > 1 else 2) + 1 + 3 + 1 + content)
    assert sum(gemms) == products and (precision != "f32" or gemms[1:] == (0, 0, 0)) and (precision == "bf16x3" or gemms[3] == 0), (gemms, products)


def _train_case(env, hp, NS, B, T, Tin, Tsub, precision, chain, defer=False, fwd_chain=None, expect=None, chain_bwd=True, overlap=True):
    """One forward + backward, twice; expect: plan fields the case is there for, {'forward': {...}, 'backward': {...}}"""
    L, ops = env
    L.set_precision(precision); L.set_chain_bwd(chain_bwd); L.lib().t2_set_overlap(int(overlap)); L.set_gemm_fold(True)
    P, dims, W, mem, mems, tl, bl, mels = _setup(L, hp, NS, B, Tin, Tsub, T)
    fwd_chain = chain if fwd_chain is None else fwd_chain
    Tsub = Tsub if NS == 2 else 1                                           # one stream: no second memory, the pass is sized for one position
    runs = []
    for _ in range(2):
        L.set_chain(fwd_chain)
        pf = _plan(L, dims, "forward", B, T, Tin, Tsub, precision, fwd_chain, chain_bwd, overlap)
        dp, prof, steps, gemms, _ = _measured(L, lambda: ops.decoder_forward(W, dims, mem, mems, tl, bl, mels, training=True, prenet_dropout=True, seed=7), T)
        _check_forward(L, dims, pf, T, NS, prof, steps, gemms, precision)
        assert not any(dp.chain_status())
        L.set_chain(chain)
        pb = _plan(L, dims, "backward", B, T, Tin, Tsub, precision, chain, chain_bwd, overlap, defer_weight_grads=defer, saved_tiles=pf["saves_tiles"])
        d_mel, d_gate = torch.ones_like(dp.mel) * 0.01, torch.ones_like(dp.gate) * 0.01
        keep = [] if defer else None

        def bwd():
            out = ops.decoder_backward(W, P, dims, dp, mem, mems, d_mel, d_gate, training=True, prenet_dropout=True, seed=7, defer=keep)
            if defer:
                ops.side_join()
            return out
        (G, dm, dms), prof, steps, gemms, defers = _measured(L, bwd, T)
        _check_backward(L, dims, pb, T, NS, prof, steps, gemms, defers, precision)
        assert not any(dp.chain_status())
        for kind, plan in (("forward", pf), ("backward", pb)):
            for k, v in (expect or {}).get(kind, {}).items():
                got = plan[k]["on"] if k.startswith("chain_") and isinstance(v, bool) else plan[k]
                assert got == v, (kind, k, got, v)
        out = dict(mel=dp.mel.clone(), gate=dp.gate.clone(), align=dp.align.clone(), d_mem=dm.clone(), **{k: v.clone() for k, v in G.items()})
        if dms is not None:
            out.update(align_sub=dp.align_sub.clone(), d_mem_sub=dms.clone())
        runs.append(out)
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert bool(torch.isfinite(runs[0][k]).all()) and torch.equal(runs[0][k], runs[1][k]), k
    L.set_chain_bwd(True); L.lib().t2_set_overlap(1)
    return pf, pb


def test_tiny_dims_fp32(env):
    pf, pb = _train_case(env, tiny_hp(SMA), 2, 2, 3, 11, 7, "f32", True,
                         expect=dict(forward=dict(use16=False, chain_a=False, overlap=False, pre16=False), backward=dict(use16=False, share=False, chain_a=False)))
    assert not pf["chain_a"]["asked"] and pb["scratch"]["dg16"][1] == 0


@pytest.mark.parametrize("att", [SMA, LSA])
def test_chains_at_the_smallest_shape(env, att):
    """B 3, T 12, memories of 13 and 9 positions: both forward chains; the backward attention chain refuses memories shorter than
    16 positions and takes the decoder-LSTM chain with it"""
    pf, pb = _train_case(env, hp_for(att), 2, 3, 12, 13, 9, "bf16", True,
                         expect=dict(forward=dict(use16=True, pre16=True, chain_a=True, chain_b=True, clear="teacher", bounds=[0, 12], saves_tiles=att is LSA),
                                     backward=dict(chain_a=False, chain_b=False, overlap=False)))
    # (SMA: the launch path takes one position split below 16 positions, and the chain is asked for only where it takes two)
    assert pb["chain_a"]["reason_text"] == ("not asked for" if att is SMA else "a memory is shorter than 16 positions") and not pb["chain_b"]["asked"]
    assert pb["nsplit"] == 1


@pytest.mark.parametrize("att", [SMA, LSA])
def test_backward_chains(env, att):
    """memories of 35 and 31 positions: the shortest whose two position splits both hold the LSA conv's halo"""
    _train_case(env, hp_for(att), 2, 3, 12, 35, 31, "bf16", True,
                expect=dict(backward=dict(chain_a=True, chain_b=True, dec_wgrads="chain_b", lsa_chain=att is LSA, dq_parts=2)))


@pytest.mark.parametrize("att", [SMA, LSA])
@pytest.mark.parametrize("defer", [False, True])
def test_chains_off_two_overlapped_ranges(env, defer, att):
    _train_case(env, hp_for(att), 2, 3, 34, 13, 9, "bf16", False, defer=defer,
                expect=dict(forward=dict(chain_a=False, overlap=True, bounds=[0, 16, 34], clear="status", poison_words=0),
                            backward=dict(overlap=True, bounds=[0, 16, 34], defer=defer, dec_wgrads="chain_b", nsplit=1)))


@pytest.mark.parametrize("chain", [False, True])
def test_overlap_switch_off(env, chain):
    """t2_set_overlap(0) at T 34: one range on the caller's stream with the chains off too, and no deferred tail though one is asked for"""
    _train_case(env, hp_for(SMA), 2, 3, 34, 35, 31, "bf16", chain, defer=True, overlap=False,
                expect=dict(forward=dict(overlap=False, bounds=[0, 34], chain_a=chain), backward=dict(overlap=False, bounds=[0, 34], defer=False, tail_on_side=False,
                                                                                                    chain_a=chain, dec_wgrads="chain_b")))


@pytest.mark.parametrize("att", [SMA, LSA])
def test_chain_bwd_switch_off(env, att):
    """t2_set_chain_bwd(0): the forward chains run, the backward pass takes the per-step launches, overlapped from T 32 on"""
    pf, pb = _train_case(env, hp_for(att), 2, 3, 34, 35, 31, "bf16", True, chain_bwd=False,
                         expect=dict(forward=dict(chain_a=True, chain_b=True, saves_tiles=att is LSA), backward=dict(chain_a=False, chain_b=False, overlap=True, bounds=[0, 16, 34])))
    assert not pb["chain_a"]["asked"]


@pytest.mark.parametrize("T,share,chunk_cast", [(32, True, True), (34, False, False)])
@pytest.mark.parametrize("chain", [False, True])
def test_shared_dg_copy_on_and_off(env, T, share, chunk_cast, chain):
    """B 8: T 32 gives B*T a multiple of 64 (the shared bf16 copy of dG, cast range by range: 16 steps x 8 rows), T 34 does not.
    With the chains on and a deferred tail the decoder-LSTM weight gradients move to the tail's stream."""
    _train_case(env, hp_for(SMA), 2, 8, T, 35, 31, "bf16", chain, defer=chain,
                expect=dict(backward=dict(share=share, tail_share=share, chunk_cast=chunk_cast, dec_wgrads_staged=chunk_cast, chain_a=chain,
                                          dec_wgrads="tail" if chain else "chain_b")))


def test_one_stream_without_a_kernel_instance(env):
    """One stream at B 97: the attention chain's tiling has no kernel instance, and the decoder LSTM leaves its chain too"""
    pf, pb = _train_case(env, hp_for(SMA), 1, 97, 4, 20, 4, "bf16", True,
                         expect=dict(forward=dict(chain_a=False, chain_b=False, chained=False), backward=dict(chain_a=False, nsplit=2)))
    assert pf["chain_a"]["reason_text"] == "the tiling of this shape has no kernel instance" and not pf["chain_b"]["asked"]


def test_lsa_backward_after_a_launch_path_forward(env):
    pf, pb = _train_case(env, hp_for(LSA), 2, 3, 12, 35, 31, "bf16", True, fwd_chain=False,
                         expect=dict(forward=dict(chain_a=False, saves_tiles=False), backward=dict(chain_a=False, chain_b=False, lsa_chain=False, dq_parts=1)))
    assert pb["chain_a"]["asked"] and pb["chain_a"]["reason_text"] == "the forward pass saved no tanh tile and location features"


@pytest.mark.parametrize("chain", [True, False])
def test_decode_loop(env, chain):
    L, ops = env
    B, T, Tin, Tsub = 2, 40, 13, 9
    L.set_precision("bf16"); L.set_chain(chain)
    P, dims, W, mem, mems, tl, bl, _ = _setup(L, hp_for(SMA), 2, B, Tin, Tsub, T)
    p = _plan(L, dims, "infer", B, T, Tin, Tsub, "bf16", chain)
    assert p["chain_a"]["on"] == chain and p["poll"] == (32 if chain else 16) and p["clear"] == ("decode" if chain else "status") and p["use16"]
    runs = []
    for _ in range(2):
        (dp, steps_run, stop), prof, steps, gemms, _ = _measured(
            L, lambda: ops.decoder_infer(W, dims, mem, mems, max_steps=T, gate_threshold=2.0, prenet_dropout=True, seed=3, mem_lengths=tl, sub_lengths=bl), T)
        assert steps_run == T and not any(dp.chain_status())                  # a sigmoid never reaches 2: every step runs
        launches = -(-T // p["poll"])
        want = dict(chain_dec=launches if chain else 0, att_lstm_fwd=0 if chain else T, attention_fwd=0 if chain else T, dec_lstm_fwd=0 if chain else T)
        assert {k: prof[k] for k in want} == want, prof
        assert steps == ((0, 0, 0, 0, 0, 0) if chain else (0, 2 * T, 0, 0, 0, 0)) and sum(gemms) == 2, (steps, gemms)
        runs.append(dict(mel=dp.mel.clone(), gate=dp.gate.clone(), align=dp.align.clone(), align_sub=dp.align_sub.clone()))
    for k in runs[0]:
        assert bool(torch.isfinite(runs[0][k]).all()) and torch.equal(runs[0][k], runs[1][k]), k
