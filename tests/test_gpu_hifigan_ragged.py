"""GPU checks of the HiFi-GAN generator on padded batches with per-item frame counts (csrc/vocoder.hip, `lengths=`).

The contract is bit equality: item b of a ragged batch is what `gen(mel[b:b+1, :, :len_b])` gives through the unchanged
equal-length path, which tests/test_gpu_hifigan.py pins to the reference; behind its length the output is exact zeros and
what the mel holds there (NaN here) is never read.  Lengths [1, 4, 8, 16, 17, 20] at rates (8, 2) and (8, 4) put the row
lengths below, at and one past the 128-sample tile edge at both stages, and one item is shorter than every pad.  Against
fp64 the bound is the vocoder's end-to-end contract, 1e-4 max-abs (tests/test_gpu_hifigan.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hifigan_ref as R
import test_gpu_hifigan as TG

pytestmark = pytest.mark.gpu

TILE = TG.TILE
LENGTHS = [1, 4, 8, 16, 17, 20]
NAN = float("nan")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(TG.GOLDEN, "hifigan.npz"))


def _gen(gold, tag, folded=True):
    gen = TG._generator(TG._config(gold, tag), TG._sd(gold, tag, "normed"))
    if folded:
        gen.remove_weight_norm()
    return gen


def _batch():
    return R.make_mel(6, 20, 9).cuda()


def _poisoned(mel, lengths):
    out = mel.clone()
    for b, n in enumerate(lengths):
        out[b, :, n:] = NAN
    return out


def _alone(gen, mel, b, n):
    with torch.no_grad():
        return gen(mel[b:b + 1, :, :n].contiguous(), return_pre_tanh=True)


@pytest.mark.parametrize("folded", [False, True], ids=["weight_normed", "folded"])
@pytest.mark.parametrize("tag", ["rb1", "rb2"])
def test_same_bits_as_alone(gold, tag, folded):
    gen = _gen(gold, tag, folded)
    up = gen.upsample_factor
    mel = _batch()
    with torch.no_grad():
        audio, pre, sl = gen(mel, return_pre_tanh=True, lengths=LENGTHS)
    torch.cuda.synchronize()
    assert audio.shape == pre.shape == (6, 1, 20 * up)
    assert sl.dtype == torch.int32 and sl.is_cuda and sl.tolist() == [n * up for n in LENGTHS]
    for b, n in enumerate(LENGTHS):
        a1, p1 = _alone(gen, mel, b, n)
        assert torch.equal(audio[b:b + 1, :, :n * up], a1), (tag, b)
        assert torch.equal(pre[b:b + 1, :, :n * up], p1), (tag, b)
        assert float(audio[b, :, n * up:].abs().sum()) == 0.0 and float(pre[b, :, n * up:].abs().sum()) == 0.0, (tag, b)
        assert float(a1.abs().max()) > 1e-3                                  # the comparison pins something


@pytest.mark.parametrize("tag", ["rb1", "rb2"])
def test_padding_does_not_matter(gold, tag):
    gen = _gen(gold, tag)
    up = gen.upsample_factor
    mel = _batch()
    with torch.no_grad():
        clean, pre_c, _ = gen(mel, return_pre_tanh=True, lengths=LENGTHS)
        dirty, pre_d, _ = gen(_poisoned(mel, LENGTHS), return_pre_tanh=True, lengths=LENGTHS)
        padded = gen(mel)
    torch.cuda.synchronize()
    assert torch.isfinite(dirty).all() and torch.isfinite(pre_d).all()
    assert torch.equal(clean, dirty) and torch.equal(pre_c, pre_d)
    # without lengths the frames behind an item's end leak into it: the equality above is not a tautology
    for b in (3, 4):
        n = LENGTHS[b] * up
        leak = float((padded[b, :, :n] - clean[b, :, :n]).abs().max())
        print(tag, "item of", LENGTHS[b], "frames: padded run differs from the item alone by", leak)
        assert leak > 1e-2


def test_list_and_device_tensor_agree_and_bad_values(gold):
    gen = _gen(gold, "rb1")
    up = gen.upsample_factor
    mel = _batch()
    dev = mel.device
    with torch.no_grad():
        a_list, s_list = gen(mel, lengths=LENGTHS)
        a_dev, s_dev = gen(mel, lengths=torch.tensor(LENGTHS, dtype=torch.int32, device=dev))
        # on the device 25 (T = 20) behaves as 20, -3 as 0; nothing is read back, the kernels clamp
        wild = [25, -3, 0, 16, 17, 20]
        a_wild, s_wild = gen(_poisoned(mel, [20, 0, 0, 16, 17, 20]), lengths=torch.tensor(wild, dtype=torch.int32, device=dev))
        a_ok, s_ok = gen(mel, lengths=[20, 0, 0, 16, 17, 20])
    torch.cuda.synchronize()
    assert torch.equal(a_list, a_dev) and torch.equal(s_list, s_dev)
    assert torch.equal(a_wild, a_ok) and torch.equal(s_wild, s_ok) and s_ok.tolist() == [20 * up, 0, 0, 16 * up, 17 * up, 20 * up]
    assert torch.isfinite(a_wild).all()
    assert float(a_ok[1].abs().sum()) == 0.0 and float(a_ok[2].abs().sum()) == 0.0      # length 0: an all-zero row of length 0
    with pytest.raises(RuntimeError, match=r"lengths\[0\]=25"):
        gen(mel, lengths=wild)
    with pytest.raises(RuntimeError, match=r"lengths\[1\]=-3"):
        gen(mel, lengths=[20, -3, 0, 16, 17, 20])


def test_full_width_vs_fp64():
    h, sd, _, _ = TG._full(1)
    lengths = [12, 5, 1]
    mel = R.make_mel(3, 12, 77)
    folded = R.fold({k: t.double() for k, t in sd.items()})
    gen = TG._generator(h, sd)
    gen.remove_weight_norm()
    with torch.no_grad():
        audio, sl = gen(_poisoned(mel, lengths).cuda(), lengths=lengths)
    torch.cuda.synchronize()
    up = gen.upsample_factor
    assert sl.tolist() == [n * up for n in lengths]
    for b, n in enumerate(lengths):
        ref, _ = R.generator_forward(folded, h, mel[b:b + 1, :, :n].contiguous())
        err = float((audio[b:b + 1, :, :n * up].cpu().double() - ref).abs().max())
        print("config_v1 item", b, "frames", n, "audio err vs fp64", err, "max |ref|", float(ref.abs().max()))
        assert ref.shape == (1, 1, n * up) and err < 1e-4
        assert float(audio[b, :, n * up:].abs().sum()) == 0.0
        assert b or float(ref.abs().max()) > 0.3                            # the comparison pins something


# ---------------------------------------------------------------------------------------------------------------------
# single layers through t2_vocoder_conv_ragged
# ---------------------------------------------------------------------------------------------------------------------
def _ragged_layer(x, w, bias, k, d, u, slope, lengths, res=None, dst=None, scale=1.0, fill=7.0):
    """y of the ragged unit entry point; where dst is None y starts as `fill` everywhere."""
    L = TG._L()
    B, Cin, Lt = x.shape
    Cout = w.shape[1] if u else w.shape[0]
    xd, wd = x.cuda().contiguous(), w.cuda().contiguous()
    bd = None if bias is None else bias.cuda().contiguous()
    rd = None if res is None else res.cuda().contiguous()
    y = dst.cuda().contiguous().clone() if dst is not None else torch.full((B, Cout, Lt * max(u, 1)), fill, device="cuda")
    ln = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    packed = torch.empty(L.lib().t2_vocoder_packed_floats(Cin, Cout, k, u), device="cuda")
    conv = L.VocoderConvArgs(B, Cin, Cout, Lt, k, d, u, L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(rd), L.ptr(y), L.ptr(packed),
                             slope, int(dst is not None), scale)
    L.check(L.lib().t2_vocoder_conv_ragged(C.byref(L.VocoderConvRaggedArgs(conv, L.ptr(ln))), L.stream()))
    torch.cuda.synchronize()
    return y.cpu()


def _behind(t, lengths, mult=1, value=NAN):
    t = t.clone()
    for b, n in enumerate(lengths):
        t[b, :, n * mult:] = value
    return t


CONV_CASE = TG.CONV_CASES[-1]        # (32, 32, 2 * TILE + 2, 11, 1, B = 3, bias, 0.1, residual, accumulate-and-scale)
CONVT_CASE = TG.CONVT_CASES[2]       # (16, 8, TILE + 1, 16, 8), run here at B = 3


@pytest.mark.parametrize("which", [0, 1], ids=["L-TILE-1", "L-1-0"])
def test_ragged_conv1d_layer(which):
    Cin, Cout, Lt, k, d, B, has_bias, slope, has_res, acc = CONV_CASE
    assert B == 3 and has_bias and has_res and acc
    lengths = [[Lt, TILE, 1], [Lt, 1, 0]][which]
    g = torch.Generator().manual_seed(31)
    x = TG._ramp(B, Cin, Lt)
    w, bias = torch.randn(Cout, Cin, k, generator=g), torch.randn(Cout, generator=g)
    res, dst = torch.randn(B, Cout, Lt, generator=g), torch.randn(B, Cout, Lt, generator=g)
    scale = float(np.float32(1.0 / 3.0))
    got = _ragged_layer(_behind(x, lengths), w, bias, k, d, 0, slope, lengths, _behind(res, lengths), _behind(dst, lengths), scale)
    for b, n in enumerate(lengths):
        if n:
            alone = TG._layer(False, x[b:b + 1, :, :n], w, bias, k, d, 0, slope, res[b:b + 1, :, :n], dst[b:b + 1, :, :n], scale)
            assert torch.equal(got[b:b + 1, :, :n], alone), (b, n)
        assert torch.isnan(got[b, :, n:]).all()                            # behind the length y is left untouched: still the NaN it held
    # without residual and accumulate: y behind the length keeps the value it had
    plain = _ragged_layer(_behind(x, lengths), w, None, k, d, 0, slope, lengths)
    for b, n in enumerate(lengths):
        if n:
            assert torch.equal(plain[b:b + 1, :, :n], TG._layer(False, x[b:b + 1, :, :n], w, None, k, d, 0, slope))
        assert bool((plain[b, :, n:] == 7.0).all())


@pytest.mark.parametrize("which", [0, 1], ids=["L-TILE-1", "L-1-0"])
def test_ragged_transposed_layer(which):
    Cin, Cout, Lt, k, u, _ = CONVT_CASE
    B = 3
    lengths = [[Lt, TILE, 1], [Lt, 1, 0]][which]
    g = torch.Generator().manual_seed(32)
    x = TG._ramp(B, Cin, Lt)
    w, bias = torch.randn(Cin, Cout, k, generator=g), torch.randn(Cout, generator=g)
    got = _ragged_layer(_behind(x, lengths), w, bias, k, 1, u, 0.1, lengths)
    assert got.shape == (B, Cout, Lt * u)
    for b, n in enumerate(lengths):
        if n:
            alone = TG._layer(True, x[b:b + 1, :, :n], w, bias, k, 1, u, 0.1)
            assert torch.equal(got[b:b + 1, :, :n * u], alone), (b, n)
        assert bool((got[b, :, n * u:] == 7.0).all())                      # untouched


def test_surface(gold):
    gen = _gen(gold, "rb1")
    mel = R.make_mel(2, 5, 1).cuda()
    with torch.no_grad():
        out = gen(mel)
        pair = gen(mel, return_pre_tanh=True)
        ragged = gen(mel, lengths=[5, 3])
        ragged3 = gen(mel, return_pre_tanh=True, lengths=[5, 3])
    assert isinstance(out, torch.Tensor) and out.shape == (2, 1, 80)          # without lengths: what it was
    assert isinstance(pair, tuple) and len(pair) == 2
    assert isinstance(ragged, tuple) and len(ragged) == 2 and ragged[1].dtype == torch.int32
    assert len(ragged3) == 3 and torch.equal(ragged3[0], ragged[0])
    with pytest.raises(RuntimeError, match="int64"):
        gen(mel, lengths=torch.tensor([5, 3], device="cuda"))
    with pytest.raises(RuntimeError, match=r"\(3,\)"):
        gen(mel, lengths=torch.tensor([5, 3, 1], dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="cpu"):
        gen(mel, lengths=torch.tensor([5, 3], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="3 lengths for a batch of 2"):
        gen(mel, lengths=[5, 3, 1])
    with pytest.raises(RuntimeError, match=r"lengths\[1\]=6"):
        gen(mel, lengths=[5, 6])
