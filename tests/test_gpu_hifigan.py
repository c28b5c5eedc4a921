"""GPU checks of the HiFi-GAN vocoder (csrc/vocoder.hip): single layers through the unit entry points against fp64 torch on
the CPU, the whole generator against the vectors recorded from the reference and against the fp64 restatement.

Single layers are held to 1e-6 * sum|w||x| + 1e-7 per output element, the sum being the same convolution of absolute
values in fp64: an fp32 MFMA chain is a k-ordered fmaf chain with 0.75 - 3.5e-7 * sum|a b| of error, 1e-6 is that with a
margin of about 3.  Inputs are a ramp in time times a per-channel sign (and a per-item gain), so that a shifted tap, a
swapped row and column or a neighbouring item cannot pass.  End to end the contract is 1e-4 max-abs, about 25 times the
reference's own fp32 error on these vectors."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hifigan_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 128


def _L():
    from tacotron2_subword_amd import _lib as L
    assert L.VOCODER_TIME_TILE == TILE
    return L


def _ramp(B, Cch, Lt, integer=False):
    t = torch.arange(Lt, dtype=torch.float64)
    sign = torch.tensor([1.0 if (c * 5 + 1) % 3 else -1.0 for c in range(Cch)], dtype=torch.float64)
    if integer:
        base = (t % 7 + 1).view(1, 1, Lt) + (torch.arange(Cch, dtype=torch.float64) % 3).view(1, Cch, 1)
        return (base * sign.view(1, Cch, 1) + torch.arange(B, dtype=torch.float64).view(B, 1, 1)).float()
    x = (1.0 + t / Lt).view(1, 1, Lt) * sign.view(1, Cch, 1) * (1.0 + 0.25 * torch.arange(B, dtype=torch.float64)).view(B, 1, 1)
    return x.float()


def _layer(transposed, x, w, bias, k, d, u, slope, res=None, dst=None, scale=1.0):
    L = _L()
    B, Cin, Lt = x.shape
    Cout = w.shape[1] if transposed else w.shape[0]
    dev = "cuda"
    xd, wd = x.to(dev).contiguous(), w.to(dev).contiguous()
    bd = None if bias is None else bias.to(dev).contiguous()
    rd = None if res is None else res.to(dev).contiguous()
    y = dst.to(dev).contiguous().clone() if dst is not None else torch.full((B, Cout, Lt * max(u, 1)), float("nan"), device=dev)
    packed = torch.empty(L.lib().t2_vocoder_packed_floats(Cin, Cout, k, u), device=dev)
    a = L.VocoderConvArgs(B, Cin, Cout, Lt, k, d, u, L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(rd), L.ptr(y), L.ptr(packed),
                          slope, int(dst is not None), scale)
    fn = L.lib().t2_vocoder_conv_transpose1d if transposed else L.lib().t2_vocoder_conv1d
    L.check(fn(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    return y.cpu()


def _check(tag, got, ref, mag):
    bound = 1e-6 * mag + 1e-7
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print(tag, "max err", float(err.max()), "worst err/bound", worst, "min bound", float(bound.min()))
    assert torch.isfinite(got).all()
    assert worst <= 1.0, tag


# (Cin, Cout, L, k, d, B, bias, slope, residual, accumulate-and-scale)
CONV_CASES = [
    (8, 8, 1, 11, 5, 1, True, 0.1, False, False),            # the whole signal is shorter than the pad of 25
    (8, 8, 8, 11, 5, 1, False, 0.01, False, False),
    (16, 16, 40, 7, 12, 1, True, 0.1, True, False),          # pad 36
    (8, 8, 140, 11, 12, 1, True, 0.1, False, False),         # pad 60: the widest halo
    (8, 16, TILE - 1, 3, 1, 1, True, 0.1, False, False),
    (8, 16, TILE, 5, 2, 1, False, 0.1, True, True),
    (16, 8, TILE + 1, 3, 3, 2, True, 0.01, True, False),
    (80, 32, 40, 7, 1, 2, True, 1.0, False, False),          # conv_pre: no activation (slope 1)
    (8, 8, 40, 3, 1, 1, True, 0.1, True, True),
    (16, 16, 40, 5, 6, 1, True, 0.1, False, True),
    (32, 32, 40, 7, 5, 1, False, 0.1, True, False),
    (24, 40, 70, 3, 2, 1, True, 0.1, True, True),            # channel counts that fill neither a chunk nor a tile
    (512, 512, 40, 3, 1, 1, True, 0.1, True, True),          # 32 chunks of K, 4 x 4 row tiles
    (32, 32, 2 * TILE + 2, 11, 1, 3, True, 0.1, True, True), # B = 3, three time tiles
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "-".join(str(int(v) if not isinstance(v, float) else v) for v in c))
def test_dilated_conv_vs_fp64(case):
    Cin, Cout, Lt, k, d, B, has_bias, slope, has_res, acc = case
    g = torch.Generator().manual_seed(Cin * 1000 + Lt * 10 + k)
    x = _ramp(B, Cin, Lt)
    w = torch.randn(Cout, Cin, k, generator=g)
    bias = torch.randn(Cout, generator=g) if has_bias else None
    res = torch.randn(B, Cout, Lt, generator=g) if has_res else None
    dst = torch.randn(B, Cout, Lt, generator=g) if acc else None
    scale = float(np.float32(1.0 / 3.0)) if acc else 1.0
    got = _layer(False, x, w, bias, k, d, 0, slope, res, dst, scale)
    xa = F.leaky_relu(x.double(), slope)
    pad = (k * d - d) // 2
    ref = F.conv1d(xa, w.double(), None if bias is None else bias.double(), padding=pad, dilation=d)
    if has_res:
        ref = ref + res.double()
    if acc:
        ref = (dst.double() + ref) * scale
    mag = F.conv1d(xa.abs(), w.double().abs(), padding=pad, dilation=d)
    _check(f"conv {case}", got, ref, mag)


def test_dilated_conv_exact_integers_bit_for_bit():
    # small integers and slope 0.5: every product and sum is exact in fp32, so any order must give the fp64 result exactly
    g = torch.Generator().manual_seed(5)
    B, Cin, Cout, Lt, k, d = 2, 24, 40, TILE + 3, 5, 3
    x = _ramp(B, Cin, Lt, integer=True)
    w = torch.randint(-3, 4, (Cout, Cin, k), generator=g).float()
    bias = torch.randint(-5, 6, (Cout,), generator=g).float()
    res = torch.randint(-9, 10, (B, Cout, Lt), generator=g).float()
    got = _layer(False, x, w, bias, k, d, 0, 0.5, res)
    ref = F.conv1d(F.leaky_relu(x.double(), 0.5), w.double(), bias.double(), padding=(k * d - d) // 2, dilation=d) + res.double()
    assert float(ref.abs().max()) < 2 ** 23
    assert torch.equal(got, ref.float())


# (Cin, Cout, L, k, u, B)
CONVT_CASES = [
    (16, 8, 1, 16, 8, 2), (32, 16, 2, 16, 8, 2), (16, 8, TILE + 1, 16, 8, 2), (512, 256, TILE, 16, 8, 2),
    (16, 8, 1, 4, 2, 2), (32, 16, 2, 4, 2, 2), (16, 8, TILE - 1, 4, 2, 2), (512, 256, 5, 4, 2, 2),
    (16, 8, 1, 8, 4, 2), (32, 16, 2, 8, 4, 2), (32, 16, TILE + 1, 8, 4, 2), (16, 8, TILE, 8, 4, 2),
]


@pytest.mark.parametrize("case", CONVT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_transposed_conv_vs_fp64(case):
    Cin, Cout, Lt, k, u, B = case
    g = torch.Generator().manual_seed(Cin * 1000 + Lt * 10 + k)
    x = _ramp(B, Cin, Lt)
    w = torch.randn(Cin, Cout, k, generator=g)
    bias = torch.randn(Cout, generator=g)
    got = _layer(True, x, w, bias, k, 1, u, 0.1)
    xa = F.leaky_relu(x.double(), 0.1)
    ref = F.conv_transpose1d(xa, w.double(), bias.double(), stride=u, padding=(k - u) // 2)
    mag = F.conv_transpose1d(xa.abs(), w.double().abs(), stride=u, padding=(k - u) // 2)
    assert got.shape == ref.shape == (B, Cout, Lt * u)
    _check(f"convT {case}", got, ref, mag)


def test_transposed_conv_exact_integers_bit_for_bit():
    g = torch.Generator().manual_seed(6)
    B, Cin, Cout, Lt, k, u = 2, 16, 24, TILE + 2, 8, 4
    x = _ramp(B, Cin, Lt, integer=True)
    w = torch.randint(-3, 4, (Cin, Cout, k), generator=g).float()
    bias = torch.randint(-5, 6, (Cout,), generator=g).float()
    got = _layer(True, x, w, bias, k, 1, u, 0.5)
    ref = F.conv_transpose1d(F.leaky_relu(x.double(), 0.5), w.double(), bias.double(), stride=u, padding=(k - u) // 2)
    assert torch.equal(got, ref.float())


def test_unit_entry_points_refuse_what_is_not_implemented():
    L = _L()
    x = torch.zeros(1, 16, 4, device="cuda")
    y = torch.zeros(1, 16, 64, device="cuda")
    w = torch.zeros(16 * 16 * 16, device="cuda")
    packed = torch.zeros(1 << 16, device="cuda")
    for k, u, needle in ((15, 8, b"odd"), (24, 8, b"not implemented"), (16, 4, b"not implemented")):
        a = L.VocoderConvArgs(1, 16, 16, 4, k, 1, u, L.ptr(x), L.ptr(w), None, None, L.ptr(y), L.ptr(packed), 0.1, 0, 1.0)
        assert L.lib().t2_vocoder_conv_transpose1d(C.byref(a), L.stream()) != 0
        assert needle in L.lib().t2_last_error()
    a = L.VocoderConvArgs(1, 16, 16, 4, 9, 1, 0, L.ptr(x), L.ptr(w), None, None, L.ptr(y), L.ptr(packed), 0.1, 0, 1.0)
    assert L.lib().t2_vocoder_conv1d(C.byref(a), L.stream()) != 0 and b"9" in L.lib().t2_last_error()
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "hifigan.npz"))


def _config(gold, tag):
    return R.H(json.loads(str(gold["configs"]))[tag])


def _sd(gold, tag, state):
    return {k: torch.from_numpy(gold[f"{tag}_{state}/{k}"]) for k in json.loads(str(gold[f"{tag}_{state}_keys"]))}


def _generator(h, normed):
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import Generator
    gen = Generator(h)
    gen.load_state_dict(normed)
    return gen.cuda().eval()


@pytest.mark.parametrize("tag", ["rb1", "rb2"])
def test_end_to_end_vs_reference_recording(gold, tag):
    gen = _generator(_config(gold, tag), _sd(gold, tag, "normed"))
    mels = [torch.from_numpy(gold[f"{tag}_mel{n}"]).cuda() for n in range(len(gold["cases"]))]
    with torch.no_grad():
        before = [gen(m, return_pre_tanh=True) for m in mels]           # still weight-normed
    gen.remove_weight_norm()
    assert "conv_pre.weight" in gen.state_dict()
    for n, m in enumerate(mels):
        with torch.no_grad():
            audio, pre = gen(m, return_pre_tanh=True)
        torch.cuda.synchronize()
        ea = float((audio.cpu() - torch.from_numpy(gold[f"{tag}_audio{n}"])).abs().max())
        ep = float((pre.cpu() - torch.from_numpy(gold[f"{tag}_pre{n}"])).abs().max())
        print(tag, tuple(m.shape), "audio err", ea, "pre-tanh err", ep)
        assert audio.shape == pre.shape == gold[f"{tag}_audio{n}"].shape
        assert ea < 1e-4 and ep < 1e-4
        assert torch.equal(audio, before[n][0]) and torch.equal(pre, before[n][1])


_FULL = {}


def _full(v):
    """(h, calibrated weight-normed state dict, mel, fp64 audio) of a full-width configuration, computed once."""
    if v not in _FULL:
        h = R.load_config(os.path.join(GOLDEN, f"hifigan_config_v{v}.json"))
        mel = R.make_mel(1, 12, 40 + v)
        sd = R.calibrate(R.make_state_dict(h, 10 + v), h, mel)
        audio, _ = R.generator_forward(R.fold({k: t.double() for k, t in sd.items()}), h, mel)
        _FULL[v] = (h, sd, mel, audio)
    return _FULL[v]


@pytest.mark.parametrize("v", [1, 2, 3])
def test_full_width_configuration_vs_fp64_restatement(v):
    h, sd, mel, ref = _full(v)
    assert float(ref.abs().max()) > 0.3 and float((ref.abs() > 0.99).double().mean()) < 0.01      # the comparison pins something
    gen = _generator(h, sd)
    gen.remove_weight_norm()
    with torch.no_grad():
        audio = gen(mel.cuda())
    torch.cuda.synchronize()
    err = float((audio.cpu().double() - ref).abs().max())
    print(f"config_v{v}", tuple(audio.shape), "audio err vs fp64", err)
    assert audio.shape == ref.shape and err < 1e-4


def test_long_signal_vs_fp64_restatement(gold):
    h, normed = _config(gold, "rb1"), _sd(gold, "rb1", "normed")
    mel = R.make_mel(1, 700, 3)
    ref, _ = R.generator_forward(R.fold({k: t.double() for k, t in normed.items()}), h, mel)
    gen = _generator(h, normed)
    gen.remove_weight_norm()
    with torch.no_grad():
        audio = gen(mel.cuda())
    torch.cuda.synchronize()
    err = float((audio.cpu().double() - ref).abs().max())
    print("T=700", tuple(audio.shape), "audio err vs fp64", err)
    assert audio.shape == (1, 1, 700 * 16) and err < 1e-4


@pytest.mark.parametrize("tag", ["rb1", "rb2"])
def test_batch_item_alone_and_rerun_give_the_same_bits(gold, tag):
    gen = _generator(_config(gold, tag), _sd(gold, tag, "normed"))
    gen.remove_weight_norm()
    mel = R.make_mel(3, 20, 9).cuda()                                    # 160 samples after the first stage: two time tiles
    with torch.no_grad():
        a = gen(mel)
        b = gen(mel)
        alone = gen(mel[1:2].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(a[1:2], alone)
    assert not torch.equal(a[0:1], alone)


def test_surface(gold):
    gen = _generator(_config(gold, "rb1"), _sd(gold, "rb1", "normed"))
    mel = R.make_mel(2, 5, 1).cuda()
    out = gen(mel.clone().requires_grad_(True).detach())
    assert out.shape == (2, 1, 80) and out.dtype == torch.float32 and out.is_cuda and not out.requires_grad
    with pytest.raises(RuntimeError, match="inference only"):
        gen(mel.clone().requires_grad_(True))
    with torch.no_grad():
        gen(mel.clone().requires_grad_(True))                            # grad mode off: fine
    with pytest.raises(RuntimeError, match="79 channels"):
        gen(mel[:, :79].contiguous())
    with pytest.raises(RuntimeError, match="GPU"):
        gen(mel.cpu())
    # an in-place edit of a parameter is picked up (autograd's version counter), an edit through .data after repack()
    with torch.no_grad():
        before = gen(mel)
        saved = gen.conv_post.bias.detach().clone()
        gen.conv_post.bias.add_(0.25)
        moved = gen(mel)
        gen.conv_post.bias.data.copy_(saved)
        gen.repack()
        back = gen(mel)
    assert not torch.equal(before, moved) and torch.equal(before, back)
