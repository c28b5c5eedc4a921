"""GPU checks of the kernels of HiFi-GAN generator training (csrc/vocoder_bwd.hip), each through its unit entry point against
torch's autograd in fp64 on the CPU: the Conv1d and ConvTranspose1d data gradients, the weight and bias gradient of both forms
and conv_post's backward.

The bound is the vocoder's own (test_gpu_hifigan.py): 1e-6 * mag + 1e-7 per element for a product whose reduction has at most
1536 terms, mag being the same reduction over absolute values in fp64 (times the leaky-ReLU derivative where the kernel
multiplies by it).  Every case stays within 1536 terms.  Outputs are pre-filled with NaN; the gradients fed in are a ramp in
time times a per-channel sign and a per-item gain, so that a swapped row, a flipped or shifted tap or a neighbouring item
cannot pass; the saved inputs are random with exact zeros and negative zeros planted."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TILE = 128


def _L():
    from tacotron2_subword_amd import _lib as L
    assert L.VOCODER_TIME_TILE == TILE
    return L


def _ramp(B, Cch, Lt):
    t = torch.arange(Lt, dtype=torch.float64)
    sign = torch.tensor([1.0 if (c * 5 + 1) % 3 else -1.0 for c in range(Cch)], dtype=torch.float64)
    x = (1.0 + t / Lt).view(1, 1, Lt) * sign.view(1, Cch, 1) * (1.0 + 0.25 * torch.arange(B, dtype=torch.float64)).view(B, 1, 1)
    return x.float()


def _saved(B, Cch, Lt, g):
    """A pre-activation input: both signs, and exact zeros and negative zeros (torch's leaky ReLU takes the slope side there)."""
    x = torch.randn(B, Cch, Lt, generator=g)
    flat = x.view(-1)
    flat[::5] = 0.0
    flat[2::7] = -0.0
    return x


def _check(tag, got, ref, mag):
    bound = 1e-6 * mag + 1e-7
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print(tag, "max err", float(err.max()), "worst err/bound", worst, "min bound", float(bound.min()))
    assert torch.isfinite(got).all(), tag
    assert worst <= 1.0, tag


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _dgrad(dy, w, x, k, d, u, slope, res=None, dst=None, scale=1.0):
    L = _L()
    B, Cin, Lt = (x.shape if x is not None else (dy.shape[0], w.shape[0] if u else w.shape[1], dy.shape[2] // max(u, 1)))
    Cout = dy.shape[1]
    dev = "cuda"
    dyd, wd = dy.to(dev).contiguous(), w.to(dev).contiguous()
    xd = None if x is None else x.to(dev).contiguous()
    rd = None if res is None else res.to(dev).contiguous()
    dx = dst.to(dev).contiguous().clone() if dst is not None else _nan(B, Cin, Lt)
    packed = _nan(L.lib().t2_vocoder_dgrad_packed_floats(Cin, Cout, k, u))
    a = L.VocoderDgradArgs(B, Cin, Cout, Lt, k, d, u, L.ptr(dyd), L.ptr(wd), L.ptr(xd), L.ptr(rd), L.ptr(dx), L.ptr(packed), slope, int(dst is not None), scale)
    fn = L.lib().t2_vocoder_conv_transpose1d_dgrad if u else L.lib().t2_vocoder_conv1d_dgrad
    L.check(fn(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    return dx.cpu()


def _mask(x, slope):
    one, sl = torch.tensor(1.0, dtype=torch.float64), torch.tensor(slope, dtype=torch.float64)
    return torch.where(x.double() > 0, one, sl)


# ---------------------------------------------------------------------------------------------------------------------
# Conv1d data gradient.  (Cin, Cout, L, k, d, B, residual, accumulate-and-scale)
# ---------------------------------------------------------------------------------------------------------------------
DGRAD_CASES = [
    (8, 8, 1, 3, 1, 1, False, False),
    (8, 8, 1, 11, 12, 1, True, False),                 # the whole signal is shorter than the pad of 60
    (8, 8, TILE - 1, 3, 1, 1, False, False),
    (8, 8, TILE, 3, 1, 1, True, True),
    (8, 8, TILE + 1, 3, 1, 1, True, False),
    (24, 8, 40, 3, 1, 1, False, True),                 # rows: a partial 32-row tile
    (8, 24, 40, 3, 1, 1, True, True),                  # K: a partial 16-channel chunk
    (8, 8, TILE + 2, 11, 12, 1, True, True),           # the widest halo (60): both clipped edges and a tile crossing
    (8, 8, TILE + 5, 3, 1, 3, True, True),             # B = 3
    (40, 16, 2 * TILE + 2, 7, 5, 3, False, False),     # two row tiles, three time tiles
]


def _dgrad_ref(dy, w, x, k, d, slope, res, dst, scale):
    pad = (k * d - d) // 2
    core = F.conv_transpose1d(dy.double(), w.double(), padding=pad, dilation=d)
    mag = F.conv_transpose1d(dy.double().abs(), w.double().abs(), padding=pad, dilation=d)
    m = _mask(x, slope) if x is not None else torch.ones_like(core)
    # the same through autograd, so that the formula above is not the only witness
    if x is not None:
        x64 = x.double().requires_grad_(True)
        F.conv1d(F.leaky_relu(x64, slope), w.double(), padding=pad, dilation=d).backward(dy.double())
        assert torch.allclose(x64.grad, m * core, rtol=1e-12, atol=1e-12)
    ref = m * core
    if res is not None:
        ref = ref + res.double()
    ref = ref * scale
    if dst is not None:
        ref = dst.double() + ref
    return ref, mag * m * scale


@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_conv1d_data_gradient_vs_fp64(case):
    Cin, Cout, Lt, k, d, B, has_res, acc = case
    assert Cout * k <= 1536
    g = torch.Generator().manual_seed(Cin * 1000 + Lt * 10 + k)
    dy = _ramp(B, Cout, Lt)
    w = torch.randn(Cout, Cin, k, generator=g)
    x = _saved(B, Cin, Lt, g)
    res = torch.randn(B, Cin, Lt, generator=g) if has_res else None
    dst = torch.randn(B, Cin, Lt, generator=g) if acc else None
    scale = float(torch.tensor(1.0 / 3.0, dtype=torch.float32)) if acc else 1.0
    got = _dgrad(dy, w, x, k, d, 0, 0.1, res, dst, scale)
    ref, mag = _dgrad_ref(dy, w, x, k, d, 0.1, res, dst, scale)
    _check(f"conv1d dgrad {case}", got, ref, mag)


def test_conv1d_data_gradient_without_activation():
    """conv_pre: no saved input, no mask (the mel's gradient)."""
    g = torch.Generator().manual_seed(11)
    B, Cin, Cout, Lt, k = 2, 80, 16, 33, 7
    dy, w = _ramp(B, Cout, Lt), torch.randn(Cout, Cin, k, generator=g)
    got = _dgrad(dy, w, None, k, 1, 0, 1.0)
    ref, mag = _dgrad_ref(dy, w, None, k, 1, 1.0, None, None, 1.0)
    _check("conv_pre dgrad", got, ref, mag)


def test_zero_and_negative_zero_take_the_slope_side():
    g = torch.Generator().manual_seed(12)
    B, C_, Lt, k = 1, 8, 16, 3
    dy, w = _ramp(B, C_, Lt), torch.randn(C_, C_, k, generator=g)
    x = torch.zeros(B, C_, Lt)
    x[:, ::2] = -0.0
    got = _dgrad(dy, w, x, k, 1, 0, 0.25)
    ones = _dgrad(dy, w, torch.ones(B, C_, Lt), k, 1, 0, 0.25)
    assert torch.equal(got, ones * 0.25)               # a multiplication by a power of two: exact


# ---------------------------------------------------------------------------------------------------------------------
# ConvTranspose1d data gradient.  (Cin, Cout, L_in, u, B)
# ---------------------------------------------------------------------------------------------------------------------
DGRAD_T_CASES = [(16, 8, 1, 2, 2), (16, 8, 2, 2, 2), (16, 16, 64, 2, 2), (24, 8, 65, 2, 2), (16, 8, TILE + 1, 2, 2),
                 (16, 8, 1, 8, 2), (16, 16, 2, 8, 2), (16, 8, 64, 8, 2), (24, 16, 65, 8, 2), (40, 8, TILE + 1, 8, 2),
                 (16, 8, 33, 4, 2)]


@pytest.mark.parametrize("case", DGRAD_T_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conv_transpose1d_data_gradient_vs_fp64(case):
    Cin, Cout, Lt, u, B = case
    k, pad = 2 * u, u // 2
    assert Cout * k <= 1536
    g = torch.Generator().manual_seed(Cin * 1000 + Lt * 10 + k)
    dy = _ramp(B, Cout, Lt * u)
    w = torch.randn(Cin, Cout, k, generator=g)
    x = _saved(B, Cin, Lt, g)
    got = _dgrad(dy, w, x, k, 1, u, 0.1)
    x64 = x.double().requires_grad_(True)
    F.conv_transpose1d(F.leaky_relu(x64, 0.1), w.double(), stride=u, padding=pad).backward(dy.double())
    mag = F.conv1d(dy.double().abs(), w.double().abs(), stride=u, padding=pad) * _mask(x, 0.1)
    assert mag.shape == got.shape == (B, Cin, Lt)
    _check(f"convT dgrad {case}", got, x64.grad, mag)


# ---------------------------------------------------------------------------------------------------------------------
# weight and bias gradient.  (Cin, Cout, L_in, k, d, u, B)
# ---------------------------------------------------------------------------------------------------------------------
WGRAD_CASES = [
    (8, 8, 1, 3, 1, 0, 3), (8, 8, 31, 3, 1, 0, 3), (8, 8, 32, 3, 1, 0, 3), (8, 8, 33, 3, 1, 0, 3), (8, 8, 257, 3, 1, 0, 3),
    (40, 24, 33, 3, 1, 0, 3),                          # rows and columns no multiple of 32; one partial tile each way
    (24, 136, 33, 11, 1, 0, 3),                        # two row tiles, 265 columns: a tap that straddles a column tile
    (8, 40, 33, 3, 1, 0, 3), (40, 8, 33, 4, 0, 2, 3),  # 33..64 rows: the waves' two-tile share (Conv1d; transposed with its row of ones)
    (8, 8, 100, 11, 12, 0, 3),                         # every tap shift clips both edges
    (80, 16, 33, 7, 1, 0, 2),                          # conv_pre
    (16, 8, 1, 4, 0, 2, 3), (16, 8, 33, 4, 0, 2, 3), (136, 8, 33, 4, 0, 2, 3),
    (16, 8, 1, 16, 0, 8, 3), (16, 8, 33, 16, 0, 8, 3), (24, 16, 63, 16, 0, 8, 3),
]


def _wgrad(x, dy, Cin, Cout, k, d, u, slope, with_bias=True):
    L = _L()
    B, _, Lt = x.shape
    dev = "cuda"
    xd, dyd = x.to(dev).contiguous(), dy.to(dev).contiguous()
    dw = _nan(*((Cin, Cout, k) if u else (Cout, Cin, k)))
    db = _nan(Cout) if with_bias else None
    part = _nan(L.lib().t2_vocoder_wgrad_part_floats(B, Cin, Cout, Lt, k, d, u))
    a = L.VocoderWgradArgs(B, Cin, Cout, Lt, k, d, u, L.ptr(xd), L.ptr(dyd), L.ptr(dw), L.ptr(db), L.ptr(part), slope)
    L.check(L.lib().t2_vocoder_wgrad(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    return dw.cpu(), (None if db is None else db.cpu())


def _wgrad_ref(xa, dy, shape, Cout, k, d, u):
    w = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose1d(xa, w, b, stride=u, padding=(k - u) // 2) if u else F.conv1d(xa, w, b, padding=(k * d - d) // 2, dilation=d)
    y.backward(dy)
    return w.grad, b.grad


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_weight_and_bias_gradient_vs_fp64(case):
    Cin, Cout, Lt, k, d, u, B = case
    assert B * Lt * max(u, 1) <= 1536
    g = torch.Generator().manual_seed(Cin * 1000 + Lt * 10 + k)
    slope = 1.0 if Cin == 80 else 0.1
    x = _saved(B, Cin, Lt, g) * (1.0 + torch.arange(Cin).view(1, Cin, 1) / Cin)
    dy = _ramp(B, Cout, Lt * max(u, 1))
    dw, db = _wgrad(x, dy, Cin, Cout, k, d, u, slope)
    xa = F.leaky_relu(x.double(), slope)
    shape = (Cin, Cout, k) if u else (Cout, Cin, k)
    rw, rb = _wgrad_ref(xa, dy.double(), shape, Cout, k, d, u)
    mw, mb = _wgrad_ref(xa.abs(), dy.double().abs(), shape, Cout, k, d, u)
    _check(f"dw {case}", dw, rw, mw)
    _check(f"db {case}", db, rb, mb)
    assert float(rw.abs().max()) > 0.0 and float(rb.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# conv_post and the tanh, backwards
# ---------------------------------------------------------------------------------------------------------------------
def _post(x, w, audio, d_audio, scale):
    L = _L()
    B, C_, Lt = x.shape
    dev = "cuda"
    xd, wd, ad, dd = (t.to(dev).contiguous() for t in (x, w, audio, d_audio))
    dx, dw, db = _nan(B, C_, Lt), _nan(C_, 7), _nan(1)
    part = torch.full((L.lib().t2_vocoder_post_part_doubles(B, C_, Lt),), float("nan"), device=dev, dtype=torch.float64)
    a = L.VocoderPostBwdArgs(B, C_, Lt, L.ptr(xd), L.ptr(wd), L.ptr(ad), L.ptr(dd), L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(part), scale)
    L.check(L.lib().t2_vocoder_post_backward(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    return dx.cpu(), dw.cpu(), db.cpu()


@pytest.mark.parametrize("C_", [8, 32])
@pytest.mark.parametrize("Lt", [1, 255, 256, 257])
def test_conv_post_backward_vs_fp64(C_, Lt):
    B = 2
    assert B * Lt <= 1536 and C_ * 7 <= 1536
    g = torch.Generator().manual_seed(C_ * 1000 + Lt)
    x = _saved(B, C_, Lt, g)
    w = torch.randn(1, C_, 7, generator=g) * 0.2
    bias = torch.randn(1, generator=g) * 0.1
    audio = torch.tanh(F.conv1d(F.leaky_relu(x.double(), 0.01), w.double(), bias.double(), padding=3)).float()
    d_audio = _ramp(B, 1, Lt)
    scale = float(torch.tensor(1.0 / 3.0, dtype=torch.float32))
    dx, dw, db = _post(x, w.view(C_, 7), audio.view(B, Lt), d_audio.view(B, Lt), scale)
    d_pre = d_audio.double() * (1.0 - audio.double() ** 2)                     # from the fp32 audio the kernel is given
    x64 = x.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    F.conv1d(F.leaky_relu(x64, 0.01), w64, b64, padding=3).backward(d_pre)
    mx = F.conv_transpose1d(d_pre.abs(), w.double().abs(), padding=3) * _mask(x, 0.01) * scale
    wa = torch.zeros(1, C_, 7, dtype=torch.float64, requires_grad=True)
    F.conv1d(F.leaky_relu(x.double(), 0.01).abs(), wa, padding=3).backward(d_pre.abs())
    _check(f"post dx {C_} {Lt}", dx, x64.grad * scale, mx)
    _check(f"post dw {C_} {Lt}", dw, w64.grad.view(C_, 7), wa.grad.view(C_, 7))
    _check(f"post db {C_} {Lt}", db, b64.grad, d_pre.abs().sum().view(1))


# ---------------------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_an_item_alone_its_bits_in_the_batch():
    g = torch.Generator().manual_seed(21)
    B, Cin, Cout, Lt = 3, 24, 16, TILE + 7
    for k, d, u in ((7, 3, 0), (16, 1, 8)):
        dy = _ramp(B, Cout, Lt * max(u, 1)) * torch.randn(B, Cout, Lt * max(u, 1), generator=g)
        w = torch.randn((Cin, Cout, k) if u else (Cout, Cin, k), generator=g)
        x = _saved(B, Cin, Lt, g)
        res = None if u else torch.randn(B, Cin, Lt, generator=g)
        full = _dgrad(dy, w, x, k, d, u, 0.1, res)
        assert torch.equal(full, _dgrad(dy, w, x, k, d, u, 0.1, res))
        for b in range(B):
            alone = _dgrad(dy[b:b + 1], w, x[b:b + 1], k, d, u, 0.1, None if res is None else res[b:b + 1])
            assert torch.equal(alone[0], full[b]), (u, b)
        dw, db = _wgrad(x, dy, Cin, Cout, k, d, u, 0.1)
        dw2, db2 = _wgrad(x, dy, Cin, Cout, k, d, u, 0.1)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)
    x, w = _saved(2, 8, 300, g), torch.randn(8, 7, generator=g)
    audio, d_audio = torch.tanh(torch.randn(2, 300, generator=g)), torch.randn(2, 300, generator=g)
    first, second = _post(x, w, audio, d_audio, 1.0), _post(x, w, audio, d_audio, 1.0)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_unit_entry_points_refuse_by_name():
    """Every refusal comes before anything is written, the weight pack included: the buffers hold random values, not zeros."""
    L = _L()
    z = torch.randn(1 << 16, generator=torch.Generator().manual_seed(31)).cuda()
    before = z.clone()
    a = L.VocoderDgradArgs(1, 16, 16, 4, 9, 1, 0, L.ptr(z), L.ptr(z), None, None, L.ptr(z[4096:]), L.ptr(z[8192:]), 0.1, 0, 1.0)
    assert L.lib().t2_vocoder_conv1d_dgrad(C.byref(a), L.stream()) != 0 and b"kernel size 9" in L.lib().t2_last_error()
    # dy is 1 x 16 x 4 = 64 floats: a destination equal to it, one that starts inside it, and one that overlaps the residual
    for dx, res in ((z, None), (z[32:], None), (z[4096:], z[4096 + 63:])):
        a = L.VocoderDgradArgs(1, 16, 16, 4, 3, 1, 0, L.ptr(z), L.ptr(z[2048:]), None, L.ptr(res), L.ptr(dx), L.ptr(z[8192:]), 0.1, 0, 1.0)
        assert L.lib().t2_vocoder_conv1d_dgrad(C.byref(a), L.stream()) != 0 and b"must not overlap" in L.lib().t2_last_error()
    torch.cuda.synchronize()
    assert torch.equal(z, before)
    a = L.VocoderDgradArgs(1, 16, 8, 4, 4, 1, 2, L.ptr(z), L.ptr(z[2048:]), None, None, L.ptr(z[64:]), L.ptr(z[8192:]), 0.1, 0, 1.0)
    assert L.lib().t2_vocoder_conv_transpose1d_dgrad(C.byref(a), L.stream()) == 0       # dy is 1 x 8 x 8 = 64 floats: the next float is free
    torch.cuda.synchronize()
    assert torch.equal(z[:64], before[:64]) and torch.equal(z[128:8192], before[128:8192]) and not torch.equal(z[64:128], before[64:128])
    z.copy_(before)
    a = L.VocoderWgradArgs(1, 16, 16, 4, 24, 1, 8, L.ptr(z), L.ptr(z), L.ptr(z), None, L.ptr(z), 0.1)
    assert L.lib().t2_vocoder_wgrad(C.byref(a), L.stream()) != 0 and b"not implemented" in L.lib().t2_last_error()
    torch.cuda.synchronize()
    assert torch.equal(z, before)
