"""GPU checks of per-item frame counts in the postnet and in batched inference (blocks.conv_bn_stack / Postnet.forward_btc
`lengths=`, Decoder.last_mel_lengths, BERT_Tacotron2.inference `per_item=`), in precision mode "f32" and eval mode.

With lengths every item must come out as its own frames alone do: the restatement below runs the five Conv1d + BatchNorm1d
layers in fp64 torch on x[b, :len_b] by itself, and the bound is the 2e-4 max-abs of test_conv_bn_stack_vs_oracle.  What the
input holds behind a length is NaN here, so anything that reads it shows."""
import pytest
import torch
import torch.nn.functional as F

from oracle import recipe

from helpers import SMA, hp_for, load_golden, maxabs
from test_gpu_model import TOL, build_model

pytestmark = pytest.mark.gpu

B, T, LENGTHS = 3, 24, [24, 11, 3]


@pytest.fixture(autouse=True)
def f32_mode():
    from tacotron2_subword_amd import _lib as L
    before = L.get_precision()
    L.set_precision("f32")
    yield
    L.set_precision(before)


def _postnet():
    from tacotron2_subword_amd.hparams import create_hparams
    from tacotron2_subword_amd.model import Postnet
    g = torch.Generator().manual_seed(21)
    net = Postnet(create_hparams())
    for blk in net.convolutions:
        bn = blk[1]
        bn.weight.data.uniform_(0.5, 1.5, generator=g); bn.bias.data.uniform_(-0.2, 0.2, generator=g)
        bn.running_mean.uniform_(-0.1, 0.1, generator=g); bn.running_var.uniform_(0.5, 1.5, generator=g)
    return net.cuda().eval()


def _restated(net, x_tc):
    """x + the five layers on one item [T, n_mel] in fp64 on the CPU (eval-mode BatchNorm, tanh on all but the last)."""
    h = x_tc.double().t()[None]
    n = len(net.convolutions)
    for i, blk in enumerate(net.convolutions):
        conv, bn = blk[0].conv, blk[1]
        h = F.conv1d(h, conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu(), padding=conv.padding[0])
        h = F.batch_norm(h, bn.running_mean.double().cpu(), bn.running_var.double().cpu(), bn.weight.detach().double().cpu(),
                         bn.bias.detach().double().cpu(), False, 0.0, bn.eps)
        if i < n - 1:
            h = torch.tanh(h)
    return h[0].t() + x_tc.double()


def test_postnet_with_lengths_vs_item_alone():
    net = _postnet()
    x = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(22))
    xd = x.clone()
    for b, n in enumerate(LENGTHS):
        xd[b, n:] = float("nan")
    xd = xd.cuda()
    keep = xd.clone()
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device="cuda")
    y = net.forward_btc(xd, 5, lengths=lengths)
    torch.cuda.synchronize()
    assert y.shape == (B, T, 80) and torch.isfinite(y).all() and not y.requires_grad
    assert torch.equal(torch.nan_to_num(xd, nan=7.0), torch.nan_to_num(keep, nan=7.0))       # the caller's tensor is not masked
    for b, n in enumerate(LENGTHS):
        ref = _restated(net, x[b, :n])
        err = float((y[b, :n].cpu().double() - ref).abs().max())
        print("item", b, "frames", n, "max err vs the item alone in fp64", err, "max |ref|", float(ref.abs().max()))
        assert float(ref.abs().max()) > 0.1 and err < 2e-4
        assert float(y[b, n:].abs().sum()) == 0.0
    # the padded call is not that: the item's last frames see what follows them
    clean = x.cuda()
    padded = net.forward_btc(clean, 5).detach()
    assert float((padded[1, :LENGTHS[1]] - y[1, :LENGTHS[1]]).abs().max()) > 1e-2
    # without lengths: the call as it was
    assert torch.equal(net.forward_btc(clean, 5, lengths=None).detach(), padded)
    full = net.forward_btc(clean, 5, lengths=torch.tensor([T] * B, dtype=torch.int32, device="cuda"))
    assert torch.equal(full, padded)


def test_lengths_raise_in_training_mode_and_on_a_bad_tensor():
    net = _postnet()
    x = torch.zeros(B, T, 80, device="cuda")
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device="cuda")
    net.train()
    with pytest.raises(RuntimeError, match="eval mode only"):
        net.forward_btc(x, 5, lengths=lengths)
    net.eval()
    with pytest.raises(RuntimeError, match="int64"):
        net.forward_btc(x, 5, lengths=lengths.long())
    with pytest.raises(RuntimeError, match="cpu"):
        net.forward_btc(x, 5, lengths=lengths.cpu())


def _stop_batch():
    """Three single items, the first being the golden stop-threshold case: under the CPU oracle they stop on frames 6, 0 and 0
    with the gate at least 1e-3 away from the threshold on every frame before."""
    g = load_golden("sma_infer")
    _, Tin, Tsub, steps = (int(v) for v in g["meta"])
    items = [recipe.make_batch(hp_for(SMA), 1, Tin, Tsub, 8, seed=s, ragged=False) for s in (4321, 4322, 4326)]
    return g, steps, [torch.cat([it[i] for it in items]).cuda() for i in (0, 6, 7, 8)]


def test_last_mel_lengths_and_per_item_inference():
    g, steps, (ids, sub, pcls, bcls) = _stop_batch()
    m, _ = build_model(SMA)
    # never stopped: every item holds all the frames decoded
    m.decoder.gate_threshold, m.decoder.max_decoder_steps = 2.0, steps
    r = m.inference(ids, sub, pcls, bcls)
    ml = m.decoder.last_mel_lengths
    assert r[5] is False and ml.dtype == torch.int32 and ml.is_cuda and ml.tolist() == [steps] * 3
    assert m.decoder.last_stop_index.tolist() == [-1] * 3
    # every item stops
    m.decoder.gate_threshold, m.decoder.max_decoder_steps = float(g["stop_threshold"]), 1000
    d = m.inference(ids, sub, pcls, bcls)
    stop = m.decoder.last_stop_index
    assert d[5] is True and bool((stop >= 0).all()) and int(stop[0]) == int(g["stop_index"])
    ml = m.decoder.last_mel_lengths
    assert ml.dtype == torch.int32 and ml.is_cuda and ml.tolist() == (stop + 1).tolist()
    assert len(set(ml.tolist())) > 1                                        # a ragged result, or the rest shows nothing
    r = m.inference(ids, sub, pcls, bcls, per_item=True)
    assert r[5] is True and torch.equal(m.last_mel_lengths, ml) and r[0].shape == d[0].shape
    for b, n in enumerate(ml.tolist()):
        assert torch.equal(r[0][b, :, :n], d[0][b, :, :n])                  # mel inside the length: the default call's
        assert float(r[0][b, :, n:].abs().sum()) == 0.0 and float(r[1][b, :, n:].abs().sum()) == 0.0
        assert torch.isfinite(r[1][b]).all()
        print("item", b, "frames", n, "mel_postnet: per-item differs from the default call by", maxabs(r[1][b, :, :n], d[1][b, :, :n]))
    # item 0 is the golden case: its mel_postnet is what its B = 1 run gives
    n0 = int(ml[0])
    assert maxabs(r[0][:1, :, :n0], g["stop_mel"]) < TOL and maxabs(r[1][:1, :, :n0], g["stop_mel_postnet"]) < TOL
    # the default call stays as it was: nothing zeroed, the same bits from call to call
    d2 = m.inference(ids, sub, pcls, bcls)
    assert torch.equal(d2[0], d[0]) and torch.equal(d2[1], d[1])
