"""The weight-gradient tail of the decoder backward on the library's side stream (Decoder.defer_weight_grads,
t2_decoder_bwd_args.defer_weight_grads), underneath the encoders' backward and joined at the end of backward.

The schedule changes no arithmetic, so every check here is bit for bit against the one-stream schedule: in the persistent
path (bf16 mode, both backward chains persistent; the library forks its side stream after the chains and also moves the
decoder-LSTM weight gradients there), below the T >= 32 threshold, with a gradient already in place (the Python layer must
not defer then), through optimizer steps with no host synchronisation, and in the per-step-launch path (fp32 mode).
t2_defer_counts says what the library did with each pass; the profile says which chains ran.  Default hparams throughout:
the persistent chains take no other dims."""
import pytest
import torch

from helpers import LSA, SMA, hp_for
from oracle import recipe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from tacotron2_subword_amd import _lib as L
    L.lib()
    yield L
    L.set_precision("f32")
    L.set_chain(True)


def _model(att):
    from tacotron2_subword_amd.hparams import create_hparams
    from tacotron2_subword_amd.model import BERT_Tacotron2
    hps = create_hparams()
    hps.attention = att
    m = BERT_Tacotron2(hps)
    m.load_state_dict(recipe.make_weights(hp_for(att)))
    m = m.cuda()
    m.train(True)
    return m


def _passes(L, m, x, y, defer, iters=2, zero=True):
    """`iters` forward + backward passes from the same RNG state.  Returns the gradients after each pass, what
    t2_defer_counts counted and how often each backward chain was launched."""
    from tacotron2_subword_amd.loss_function import Tacotron2Loss
    m.decoder.defer_weight_grads = defer
    m._t2_calls, m.decoder._t2_calls = 0, 0
    m.zero_grad()
    T = x[3].shape[2]
    L.defer_counts(reset=True)
    L.prof_enable(iters * (8 * T + 64))
    out = []
    for it in range(iters):
        if zero or it == 0:
            m.zero_grad()
        Tacotron2Loss()(m(x), y, x)[0].backward()
        out.append({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    torch.cuda.synchronize()
    prof = L.prof_collect()
    return out, L.defer_counts(reset=True), {k: prof[k][1] for k in ("chain_a_bwd", "chain_b_bwd")}


def _same(a, b):
    assert len(a) == len(b)
    for it, (ga, gb) in enumerate(zip(a, b)):
        assert ga.keys() == gb.keys() and len(ga) > 40
        for k in ga:
            assert torch.equal(ga[k], gb[k]), (it, k, float((ga[k] - gb[k]).abs().max()))


def _setup(att, shape):
    """Model and batch, after one pass that is not compared: at B >= 32 the first pass of a fresh model differs from every
    later one under either schedule (flag off twice in a row: every gradient, up to 1e-4 absolute in the embeddings);
    the later ones repeat bit for bit, and those are what the two schedules are compared on."""
    from tacotron2_subword_amd.loss_function import Tacotron2Loss
    m = _model(att)
    x, y = m.parse_batch(recipe.make_batch(hp_for(att), *shape))
    Tacotron2Loss()(m(x), y, x)[0].backward()
    torch.cuda.synchronize()
    return m, x, y


@pytest.mark.parametrize("att", [SMA, LSA])
@pytest.mark.parametrize("shape", [(4, 35, 31, 33), (33, 35, 31, 32), (8, 35, 31, 32)])
def test_persistent_path_defers_and_keeps_every_gradient(env, att, shape):
    """(B, Tin, Tsub, T) = (4, 35, 31, 33): one row tile, one step over the threshold, odd T, LSA's shortest memories;
    (33, 35, 31, 32): the first batch size with two row tiles (the second partly filled), T at the threshold;
    (8, 35, 31, 32): B * T a multiple of 64 and B of 8, the smallest case in which the weight-gradient products read the
    shared bf16 copy of dG at the head of the GEMM scratch, as they do at the benchmark's shape: whatever overwrites the
    copy before its last reader shows here."""
    L = env
    L.set_precision("bf16"); L.set_chain(True)
    m, x, y = _setup(att, shape)
    on, counts_on, chains_on = _passes(L, m, x, y, True)
    off, counts_off, chains_off = _passes(L, m, x, y, False)
    assert chains_on == {"chain_a_bwd": 2, "chain_b_bwd": 2} and chains_off == chains_on, (chains_on, chains_off)
    assert counts_on == (2, 0) and counts_off == (0, 2), (counts_on, counts_off)
    _same(on, off)


def test_below_the_threshold_nothing_is_deferred(env):
    L = env
    L.set_precision("bf16"); L.set_chain(True)
    m, x, y = _setup(SMA, (4, 35, 31, 31))
    on, counts_on, _ = _passes(L, m, x, y, True)
    off, counts_off, _ = _passes(L, m, x, y, False)
    assert counts_on == (0, 2) and counts_off == (0, 2), (counts_on, counts_off)
    _same(on, off)


def test_existing_gradients_are_accumulated_on_one_stream(env):
    """No zero_grad before the second backward: AccumulateGrad reads the new gradient during backward, so that pass must
    not leave it on the side stream."""
    L = env
    L.set_precision("bf16"); L.set_chain(True)
    m, x, y = _setup(SMA, (4, 35, 31, 33))
    on, counts_on, chains = _passes(L, m, x, y, True, zero=False)
    off, counts_off, _ = _passes(L, m, x, y, False, zero=False)
    assert chains == {"chain_a_bwd": 2, "chain_b_bwd": 2}, chains
    assert counts_on == (1, 1) and counts_off == (0, 2), (counts_on, counts_off)
    _same(on, off)


def test_optimizer_steps_wait_for_the_side_stream(env):
    """Three training iterations back to back, nothing synchronises the host in between: the optimizer reads every
    gradient and the next iteration reuses the released workspaces, both only after the join."""
    from tacotron2_subword_amd import train as T
    from tacotron2_subword_amd.hparams import create_hparams
    L = env
    L.set_precision("bf16"); L.set_chain(True)
    res, counts = {}, {}
    for defer in (True, False):
        hps = create_hparams()
        hps.distributed_run = False
        model, opt, crit = T.make_training_objects(hps)
        model.train()
        model.decoder.defer_weight_grads = defer
        x, y = model.parse_batch(T.synthetic_batch(hps, 4, 35, 31, 33, seed=3))
        L.defer_counts(reset=True)
        for it in range(3):
            T.train_step(model, crit, opt, x, y, hps, it)
        torch.cuda.synchronize()
        counts[defer] = L.defer_counts(reset=True)
        state = {"param." + k: p.detach().clone() for k, p in model.named_parameters()}
        for k, p in model.named_parameters():
            if p in opt.state:
                state["m." + k], state["v." + k] = opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()
        res[defer] = state
    assert counts == {True: (3, 0), False: (0, 3)}, counts
    assert res[True].keys() == res[False].keys() and any(k.startswith("v.decoder.") for k in res[True])
    for k in res[True]:
        assert torch.equal(res[True][k], res[False][k]), k


def test_launch_path_still_defers(env):
    """fp32 mode runs one launch per step and kernel: the side stream exists from the first chunk on, as before."""
    L = env
    L.set_precision("f32"); L.set_chain(True)
    m, x, y = _setup(SMA, (4, 21, 13, 40))
    on, counts_on, chains = _passes(L, m, x, y, True)
    off, counts_off, _ = _passes(L, m, x, y, False)
    assert chains == {"chain_a_bwd": 0, "chain_b_bwd": 0}, chains
    assert counts_on == (2, 0) and counts_off == (0, 2), (counts_on, counts_off)
    _same(on, off)
