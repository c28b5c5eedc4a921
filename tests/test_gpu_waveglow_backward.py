"""GPU checks of WaveGlow's training direction (csrc/waveglow.hip: the forward that keeps what the backward reads, and the
backward): every kernel the driver launches on its own through the unit entry points against fp64, then ``WaveGlow.trainable()``
end to end -- ``.grad`` of every parameter against the gradients recorded from the reference's own forward and torch's autograd
(tests/golden/waveglow_grad.npz) and against the fp64 restatement (tests/waveglow_grad_ref.py), weight-normed and folded, at full
width, for general upstream gradients, over three SGD steps, determinism and the surface.

Bounds.  A product whose reduction has at most 1536 terms is held to 1e-6 * mag + 1e-7 per element, mag the same sum over absolute
values in fp64 (tests/test_gpu_waveglow.py).  A sum the kernels accumulate in fp64 from exact products is held to 2^-23 * sum
|terms| plus what the fp32 factors of the terms themselves carry, stated where it is used.  End to end a gradient tensor is held
to 25 * max(the fp32 CPU autograd's own max deviation from fp64 on that tensor, 2^-23 * max |g64|), and max |g64| > 0 is asserted
for every tensor.  No test calls torch's convolution library on the GPU: every reference is computed on the CPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import waveglow_fwd_ref as FR
import waveglow_grad_ref as GR
import waveglow_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
ULP = 2.0 ** -23
SIGMA = 0.7


def _L():
    from tacotron2_subword_amd import _lib as L
    return L


def _glow():
    from tacotron2_subword_amd.waveglow import glow
    return glow


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _check(tag, got, ref, bound):
    got = got.cpu()
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print(tag, "max err", float(err.max()), "worst err/bound", worst, "min bound", float(bound.min()))
    assert torch.isfinite(got).all(), tag
    assert worst <= 1.0, tag
    return worst


def _ramp(B, Cch, Lt):
    """A ramp in time times a per-channel sign and a per-item gain: a swapped row or a neighbouring item cannot pass."""
    t = torch.arange(Lt, dtype=torch.float64)
    sign = torch.tensor([1.0 if (c * 5 + 1) % 3 else -1.0 for c in range(Cch)], dtype=torch.float64)
    return ((1.0 + t / Lt).view(1, 1, Lt) * sign.view(1, Cch, 1) * (1.0 + 0.25 * torch.arange(B, dtype=torch.float64)).view(B, 1, 1)).float()


def _rough(B, Cch, Lt, g, scale=1.0):
    """The ramp with every element's gain drawn from [1, 1.5): rows with equal signs differ too."""
    return _ramp(B, Cch, Lt) * (1.0 + 0.5 * torch.rand(B, Cch, Lt, generator=g)) * scale


def _shifted(x, sh):
    """y[..., l] = x[..., l + sh], zero outside the row."""
    Lt, y = x.shape[-1], torch.zeros_like(x)
    if 0 <= sh < Lt:
        y[..., :Lt - sh] = x[..., sh:]
    elif -Lt < sh < 0:
        y[..., -sh:] = x[..., :Lt + sh]
    return y


# ------------------------------------------------------------------------------------------------------------------ 1. weight gradient
# (nc, n_cond, L, d, B): L = 1; a partial row tile, both edges clipped, a time chunk of 32 crossed; side taps that see nothing;
# the published width; three items with a row longer than 256; then rows of whole quads, which take the 16-byte loads: with
# shifts of whole quads that clip both edges across a chunk, and with shifts that are none (the taps then load element by element)
WGRAD_CASES = [(8, 8, 1, 1, 1), (40, 64, 129, 4, 3), (16, 8, 100, 128, 2), (256, 640, 127, 2, 1), (24, 8, 257, 1, 3), (40, 64, 132, 4, 2),
               (24, 8, 68, 2, 3)]


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("rows", ["2nc", "nc"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_weight_grad_vs_fp64(case, rows, padded):
    """M = 2nc: the in-layer's launch (x at three shifts, spect, the bias column); M = nc: res_skip's (one tap, no spect).
    B * L <= 1536 in every case, so every element is held to 1e-6 * mag + 1e-7.  padded: both operands are the first rows of
    buffers with more rows per item (as dW_start reads n_half of audio_in's c rows; the extra rows hold other values), and the
    bias column goes to a second destination too (as cond_layer.bias's slice)."""
    L = _L()
    nc, n_cond, Lt, d, B = case
    assert B * Lt <= 1536
    wide = rows == "2nc"
    M, taps, n_cond, d = (2 * nc, 3, n_cond, d) if wide else (nc, 1, 0, 0)
    g = torch.Generator().manual_seed(nc * 1000 + Lt * 10 + d)
    a, x = _rough(B, M, Lt, g), _rough(B, nc, Lt, g, 0.5)
    spect = _rough(B, n_cond, Lt, g, 0.25) if wide else None
    dw_x, dw_s, db = _nan(M, nc, taps), (_nan(M, n_cond) if wide else None), _nan(M)
    ws = _nan(L.lib().t2_waveglow_weight_grad_ws_floats(M, nc, n_cond, taps, B, Lt))
    a_rows, x_rows = (M + 3, nc + 2) if padded else (0, 0)
    wider = lambda v, extra: torch.cat([v, 7.0 - _rough(B, extra, Lt, g)], 1) if padded else v
    db2 = _nan(M) if padded else None
    t = [_d(wider(a, 3)), _d(wider(x, 2)), _d(spect)]        # kept alive until the kernel has run
    args = L.WaveglowWeightGradArgs(B, M, nc, n_cond, Lt, taps, d, a_rows, x_rows, *[L.ptr(v) for v in t], L.ptr(dw_x), L.ptr(dw_s), L.ptr(db), L.ptr(ws),
                                    L.ptr(db2))
    L.check(L.lib().t2_waveglow_weight_grad(C.byref(args), L.stream()))
    torch.cuda.synchronize()
    assert db2 is None or torch.equal(db, db2)
    a64, x64 = a.double(), x.double()
    xs = [_shifted(x64, (j - taps // 2) * d) for j in range(taps)]
    ref = torch.stack([torch.einsum("bml,bcl->mc", a64, s) for s in xs], 2)
    mag = torch.stack([torch.einsum("bml,bcl->mc", a64.abs(), s.abs()) for s in xs], 2)
    if wide and d >= Lt:
        assert float(ref[:, :, 0].abs().max()) == 0.0 == float(ref[:, :, 2].abs().max())       # the side taps see nothing
    _check(f"dW_x {case} {rows}", dw_x, ref, 1e-6 * mag + 1e-7)
    if wide:
        _check(f"dW_spect {case}", dw_s, torch.einsum("bml,bcl->mc", a64, spect.double()), 1e-6 * torch.einsum("bml,bcl->mc", a64.abs(), spect.double().abs()) + 1e-7)
    _check(f"db {case} {rows}", db, a64.sum((0, 2)), 1e-6 * a64.abs().sum((0, 2)) + 1e-7)


# ------------------------------------------------------------------------------------------------------------------ 2. gate and conv backward
# (nc, n_cond, L, d, B, last, first): the edges of tests/test_gpu_waveglow.py's GATED_CASES, each with a first / last variant
BWD_CASES = [(8, 64, 1, 1, 1, 0, 0), (8, 64, 32, 64, 1, 1, 1), (16, 64, 127, 2, 3, 0, 1), (24, 64, 128, 128, 1, 1, 0), (16, 640, 129, 128, 1, 0, 0),
             (8, 64, 258, 128, 3, 1, 1), (24, 64, 258, 64, 1, 0, 0), (256, 640, 129, 2, 1, 0, 0), (256, 64, 32, 128, 1, 1, 1), (24, 640, 1, 128, 3, 0, 1)]


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gate_backward_vs_fp64(case):
    """d_acts = W_rs^T [dx; d_out] is a chain over at most 2nc <= 512 terms: e = 1e-6 * mag + 1e-7.  du_a = d_acts g (1 - t^2):
    e times |g (1 - t^2)|, plus 4 ulp of |d_acts g| (t^2 and 1 - t^2, of size at most 1, round once each, the two products once
    each); du_b = d_acts t g (1 - g): e times |t g (1 - g)| plus 5 ulp of |d_acts t g|.  acts = t g is one fp32 product: bit exact."""
    L = _L()
    nc, _, Lt, _, B, last, _ = case
    g = torch.Generator().manual_seed(nc * 1000 + Lt * 10 + last)
    rows = nc if last else 2 * nc
    w = torch.randn(rows, nc, generator=g) * rows ** -0.5
    dx, d_out = (None if last else _rough(B, nc, Lt, g)), _rough(B, nc, Lt, g, 0.5)
    t, s = torch.tanh(torch.randn(B, nc, Lt, generator=g)), torch.sigmoid(torch.randn(B, nc, Lt, generator=g))
    du, acts = _nan(B, 2 * nc, Lt), _nan(B, nc, Lt)
    pw = _nan(2 * L.lib().t2_waveglow_packed_floats(L.WAVEGLOW_RES_SKIP, nc, nc, 0))
    held = [_d(dx), _d(d_out), _d(w), _d(t), _d(s)]
    a = L.WaveglowGateBackwardArgs(B, nc, Lt, last, *[L.ptr(v) for v in held], L.ptr(pw), L.ptr(du), L.ptr(acts))
    L.check(L.lib().t2_waveglow_gate_backward(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    d_rs = d_out.double() if last else torch.cat([dx, d_out], 1).double()
    da = torch.einsum("rc,brl->bcl", w.double(), d_rs)
    e = 1e-6 * torch.einsum("rc,brl->bcl", w.double().abs(), d_rs.abs()) + 1e-7
    t64, s64 = t.double(), s.double()
    fa, fb = s64 * (1 - t64 * t64), t64 * s64 * (1 - s64)
    ref = torch.cat([da * fa, da * fb], 1)
    bound = torch.cat([e * fa.abs() + 4 * ULP * (da * s64).abs(), e * fb.abs() + 5 * ULP * (da * t64 * s64).abs()], 1) + 1e-30
    assert float(ref.std()) > 0.01
    _check(f"du {case}", du, ref, bound)
    assert torch.equal(acts.cpu(), t * s)


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conv_backward_vs_fp64(case):
    """dx (+)= conv^T(du) has K = 3 * 2nc <= 1536 terms, d_spect (+)= W_cond^T du has 2nc: 1e-6 * mag + 1e-7 each, and an
    accumulating epilogue starts from a non-zero dx / d_spect, whose sum rounds once more: + ulp * (|start| + |result|)."""
    L = _L()
    nc, n_cond, Lt, d, B, first_dx, first_spect = case
    g = torch.Generator().manual_seed(nc * 1000 + Lt * 10 + d)
    w_in, w_cond = torch.randn(2 * nc, nc, 3, generator=g) * (6 * nc) ** -0.5, torch.randn(2 * nc, n_cond, generator=g) * (2 * nc) ** -0.5
    du = _rough(B, 2 * nc, Lt, g)
    dx0, ds0 = _rough(B, nc, Lt, g, 0.5), _rough(B, n_cond, Lt, g, 0.25)
    dx, dsp = (_nan(B, nc, Lt) if first_dx else _d(dx0).clone()), (_nan(B, n_cond, Lt) if first_spect else _d(ds0).clone())
    pw = _nan(L.lib().t2_waveglow_conv_backward_packed_floats(nc, n_cond))
    held = [_d(du), _d(w_in), _d(w_cond)]
    a = L.WaveglowConvBackwardArgs(B, nc, n_cond, Lt, d, first_dx, first_spect, *[L.ptr(v) for v in held], L.ptr(pw), L.ptr(dx), L.ptr(dsp))
    L.check(L.lib().t2_waveglow_conv_backward(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    du64 = du.double()
    ref = F.conv_transpose1d(du64, w_in.double(), dilation=d, padding=d)
    mag = F.conv_transpose1d(du64.abs(), w_in.double().abs(), dilation=d, padding=d)
    assert ref.shape == (B, nc, Lt)
    if not first_dx:
        ref, mag = ref + dx0.double(), mag + (ULP / 1e-6) * (dx0.double().abs() + (ref + dx0.double()).abs())
    _check(f"dx {case}", dx, ref, 1e-6 * mag + 1e-7)
    ref = torch.einsum("rm,brl->bml", w_cond.double(), du64)
    mag = torch.einsum("rm,brl->bml", w_cond.double().abs(), du64.abs())
    if not first_spect:
        ref, mag = ref + ds0.double(), mag + (ULP / 1e-6) * (ds0.double().abs() + (ref + ds0.double()).abs())
    _check(f"d_spect {case}", dsp, ref, 1e-6 * mag + 1e-7)


# ------------------------------------------------------------------------------------------------------------------ 3. tail backward
# the grid of test_tail_vs_fp64 with both upstream gradients given; each of them omitted once on an inner and once on the last flow
TAIL_CASES = [(4, 0, 8, 1, 1, "both"), (4, 2, 256, 257, 2, "both"), (3, 0, 24, 300, 1, "both"), (3, 2, 16, 255, 3, "both"), (2, None, 256, 40, 1, "both"),
              (1, None, 8, 513, 2, "both"), (4, 2, 256, 257, 2, "no_dz"), (4, 2, 256, 257, 2, "no_dlog_s"), (2, None, 256, 40, 1, "no_dz"),
              (2, None, 256, 40, 1, "no_dlog_s")]


@pytest.mark.parametrize("n_half, n_peel, nc, Lt, B, upstream", TAIL_CASES)
def test_tail_backward_vs_fp64(n_half, n_peel, nc, Lt, B, upstream):
    """The grid of test_tail_vs_fp64 (n_peel None: the last flow).  (b, s) = end(out) are chains over nc, e_s = 1e-6 * mag + 1e-7.
    dV is dz (exact) or a chain over at most 8 terms through W_next (e_V = 1e-6 * mag + 1e-7).  da1 = db exp(s) carries
    e_a = e_V exp(s) + |db| exp(s) (e_s + 3 ulp) (the error of s to first order, expf, one product); ds = da1 a1 + dlog_s carries
    e_ds = e_a |a1| + ulp |ds| (one fma).  d_out = W_end^T [db; ds] is a chain over at most 8 terms of those.  The sums dW_end,
    db_end and dW_next are formed in fp64 from exact products of the kernel's fp32 factors and rounded once: 2^-23 * sum |terms|
    of the fp64 sums, plus the factors' own errors e_V, e_ds, e_v summed against the other factor."""
    L = _L()
    g = torch.Generator().manual_seed(n_half * 1000 + nc + Lt)
    c, G = 2 * n_half, 8
    last = n_peel is None
    n_peel = c if last else n_peel
    cn, zoff = c - n_peel, G - c if last else 2
    out = _ramp(B, nc, Lt) * 0.5
    w_end, b_end = torch.randn(c, nc, generator=g) * 0.5 * nc ** -0.5, torch.randn(c, generator=g) * 0.1
    audio = torch.randn(B, c, Lt, generator=g)
    W = None if last else (torch.linalg.qr(torch.randn(cn, cn, generator=g))[0] * (0.5 + 1.5 * torch.rand(cn, generator=g))).contiguous()
    d_next = None if last else _rough(B, cn, Lt, g)
    dz = None if upstream == "no_dz" else _rough(B, G, Lt, g, 0.7)
    dls = None if upstream == "no_dlog_s" else _rough(B, n_half, Lt, g, 0.3)
    nblk = (Lt + 255) // 256
    d_out, d_in = _nan(B, nc, Lt), _nan(B, c, Lt)
    part = _nan(B * nblk * 4 * (c * nc + c + cn * cn), dtype=torch.float64)
    dw_end, db_end, dw_next = _nan(c, nc), _nan(c), (None if last else _nan(cn, cn))
    t = [_d(out), _d(w_end), _d(b_end), _d(audio), _d(W), _d(d_next), _d(dz), _d(dls)]
    a = L.WaveglowTailBackwardArgs(B, nc, n_half, Lt, n_peel, G, zoff, *[L.ptr(v) for v in t], L.ptr(d_out), L.ptr(d_in), L.ptr(part), L.ptr(dw_end),
                                   L.ptr(db_end), L.ptr(dw_next))
    L.check(L.lib().t2_waveglow_tail_backward(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    out64 = out.double()
    o = F.conv1d(out64, w_end.double()[:, :, None], b_end.double())
    e_o = 1e-6 * F.conv1d(out64.abs(), w_end.double().abs()[:, :, None], b_end.double().abs()) + 1e-7
    b, s, e_b, e_s = o[:, :n_half], o[:, n_half:], e_o[:, :n_half], e_o[:, n_half:]
    a0, a1 = audio[:, :n_half].double(), audio[:, n_half:].double()
    es = torch.exp(s)
    v = torch.cat([a0, es * a1 + b], 1)
    e_v = torch.cat([torch.zeros_like(e_b), e_b + es * a1.abs() * (e_s + 2 * ULP) + ULP * v[:, n_half:].abs()], 1)
    dV, e_V = torch.zeros(B, c, Lt, dtype=torch.float64), torch.zeros(B, c, Lt, dtype=torch.float64)
    if dz is not None:
        dV[:, :n_peel] = dz[:, zoff:zoff + n_peel].double()
    if not last:
        dV[:, n_peel:] = torch.einsum("qr,bql->brl", W.double(), d_next.double())
        e_V[:, n_peel:] = 1e-6 * torch.einsum("qr,bql->brl", W.double().abs(), d_next.double().abs()) + 1e-7
    db, e_db = dV[:, n_half:], e_V[:, n_half:]
    da1, e_a = db * es, e_V[:, n_half:] * es + db.abs() * es * (e_s + 3 * ULP)
    ds = da1 * a1 + (0.0 if dls is None else dls.double())
    e_ds = e_a * a1.abs() + ULP * ds.abs()
    _check("d_in", d_in, torch.cat([dV[:, :n_half], da1], 1), torch.cat([e_V[:, :n_half], e_a], 1) + 1e-30)
    e, e_e = torch.cat([db, ds], 1), torch.cat([e_db, e_ds], 1)
    ref = torch.einsum("rc,brl->bcl", w_end.double(), e)
    _check("d_out", d_out, ref, torch.einsum("rc,brl->bcl", w_end.double().abs(), e_e + 1e-6 * e.abs()) + 1e-7)
    _check("dW_end", dw_end, torch.einsum("brl,bcl->rc", e, out64),
           ULP * torch.einsum("brl,bcl->rc", e.abs(), out64.abs()) + torch.einsum("brl,bcl->rc", e_e, out64.abs()) + 1e-300)
    _check("db_end", db_end, e.sum((0, 2)), ULP * e.abs().sum((0, 2)) + e_e.sum((0, 2)) + 1e-300)
    if not last:
        dn, vn, e_vn = d_next.double(), v[:, n_peel:], e_v[:, n_peel:]
        _check("dW_next", dw_next, torch.einsum("bql,brl->qr", dn, vn),
               ULP * torch.einsum("bql,brl->qr", dn.abs(), vn.abs()) + torch.einsum("bql,brl->qr", dn.abs(), e_vn) + 1e-300)


@pytest.mark.parametrize("nc, c, n_half, Lt, B", [(8, 2, 1, 1, 1), (256, 8, 4, 257, 2), (24, 6, 3, 300, 1), (16, 8, 2, 255, 3)])
def test_start_backward_vs_fp64(nc, c, n_half, Lt, B):
    """d_in[:, :n_half] += W_start^T dx is a chain over nc <= 512 terms added to what the tail left there: 1e-6 * mag + 1e-7 plus
    ulp * (|start| + |result|); the rows from n_half on stay bit for bit.  dW_start and db_start are the weight-gradient kernel on
    the first n_half of audio_in's c rows, B * L <= 1536 terms: 1e-6 * mag + 1e-7."""
    L = _L()
    assert B * Lt <= 1536
    g = torch.Generator().manual_seed(nc * 100 + c * 10 + Lt)
    dx, ain, d0 = _rough(B, nc, Lt, g), _rough(B, c, Lt, g, 0.5), _rough(B, c, Lt, g, 0.3)
    w = torch.randn(nc, n_half, generator=g) * nc ** -0.5
    d_in, dw, db = _d(d0).clone(), _nan(nc, n_half), _nan(nc)
    ws = _nan(L.lib().t2_waveglow_weight_grad_ws_floats(nc, n_half, 0, 1, B, Lt))
    held = [_d(dx), _d(w), _d(ain)]
    a = L.WaveglowStartBackwardArgs(B, nc, c, n_half, Lt, *[L.ptr(v) for v in held], L.ptr(d_in), L.ptr(dw), L.ptr(db), L.ptr(ws))
    L.check(L.lib().t2_waveglow_start_backward(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    dx64, a0 = dx.double(), ain[:, :n_half].double()
    ref = d0[:, :n_half].double() + torch.einsum("ch,bcl->bhl", w.double(), dx64)
    bound = 1e-6 * torch.einsum("ch,bcl->bhl", w.double().abs(), dx64.abs()) + 1e-7 + ULP * (d0[:, :n_half].double().abs() + ref.abs())
    _check(f"d_in {(nc, c, n_half, Lt, B)}", d_in[:, :n_half], ref, bound)
    assert torch.equal(d_in[:, n_half:].cpu(), d0[:, n_half:])
    _check("dW_start", dw, torch.einsum("bcl,bhl->ch", dx64, a0), 1e-6 * torch.einsum("bcl,bhl->ch", dx64.abs(), a0.abs()) + 1e-7)
    _check("db_start", db, dx64.sum((0, 2)), 1e-6 * dx64.abs().sum((0, 2)) + 1e-7)


@pytest.mark.parametrize("G", [2, 8])
@pytest.mark.parametrize("N", ["G", 8 * 256 + 5])
def test_head_backward_vs_fp64(G, N):
    """dW_0 = sum d(audio_in_0) * regrouped audio^T, an fp64 sum of exact products rounded once: 2^-23 * sum |terms|.  The grid of
    test_head_regroup_and_mix: L = 1, and nine column blocks with a dropped tail of N mod G samples."""
    L = _L()
    N, B = G if N == "G" else N, 3
    Lt = N // G
    g = torch.Generator().manual_seed(G * 10 + Lt)
    d_in, audio = _rough(B, G, Lt, g), torch.randn(B, N, generator=g)
    part, dw = _nan(B * ((Lt + 255) // 256) * 4 * G * G, dtype=torch.float64), _nan(G, G)
    held = [_d(d_in), _d(audio)]
    a = L.WaveglowHeadBackwardArgs(B, G, N, *[L.ptr(v) for v in held], L.ptr(part), L.ptr(dw))
    L.check(L.lib().t2_waveglow_head_backward(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    x = audio[:, :Lt * G].double().reshape(B, Lt, G).permute(0, 2, 1)
    _check(f"dW_0 {(G, N)}", dw, torch.einsum("brl,bgl->rg", d_in.double(), x), ULP * torch.einsum("brl,bgl->rg", d_in.double().abs(), x.abs()) + 1e-300)


# ------------------------------------------------------------------------------------------------------------------ 4. upsample backward
@pytest.mark.parametrize("n_mel, T, G, B, extra", [(8, 1, 8, 1, 0), (8, 5, 8, 3, 0), (80, 2, 8, 1, 0), (8, 5, 2, 1, 0), (8, 3, 8, 2, 768)])
def test_upsample_backward_vs_fp64(n_mel, T, G, B, extra):
    """extra = 768: n_samples = (T - 1) * 256 + 1024, the three frames past T included.  Each element is an fp64 sum of exact
    products rounded once: 2^-23 * sum |terms|."""
    L = _L()
    n = T * 256 + extra
    g = torch.Generator().manual_seed(n_mel * 100 + T * 10 + G)
    mel = R.make_mel(B, T, 77, n_mel=n_mel)
    d_spect = _rough(B, n_mel * G, n // G, g)
    dw, db = _nan(n_mel, n_mel, 1024), _nan(n_mel)
    held = [_d(mel), _d(d_spect)]
    a = L.WaveglowUpsampleBackwardArgs(B, n_mel, T, G, n, *[L.ptr(v) for v in held], L.ptr(dw), L.ptr(db))
    L.check(L.lib().t2_waveglow_upsample_backward(C.byref(a), L.stream()))
    torch.cuda.synchronize()

    def grad(m, ds):
        p = {"upsample.weight": torch.zeros(n_mel, n_mel, 1024, dtype=torch.float64, requires_grad=True),
             "upsample.bias": torch.zeros(n_mel, dtype=torch.float64, requires_grad=True)}
        (FR.upsample(p, dict(n_group=G), m.double(), n) * ds.double()).sum().backward()
        return p["upsample.weight"].grad, p["upsample.bias"].grad
    (rw, rb), (mw, mb) = grad(mel, d_spect), grad(mel.abs(), d_spect.abs())
    assert float(rw.abs().max()) > 0
    _check(f"dW_up {(n_mel, T, G, B, extra)}", dw, rw, ULP * mw + 1e-300)
    _check("db_up", db, rb, ULP * mb + 1e-300)


# ------------------------------------------------------------------------------------------------------------------ 5. end to end
@pytest.fixture(scope="module")
def gold():
    z, fwd, base = (np.load(os.path.join(GOLDEN, f)) for f in ("waveglow_grad.npz", "waveglow_forward.npz", "waveglow.npz"))
    out = {k: z[k] for k in z.files}
    out["fwd"], out["base"], out["configs"] = {k: fwd[k] for k in fwd.files}, {k: base[k] for k in base.files}, json.loads(str(base["configs"]))
    assert float(out["sigma"]) == SIGMA
    return out


def _sd(gold, tag):
    base = gold["base"]
    sd = {k: torch.from_numpy(base[k if k.startswith("upsample.") else f"{tag}/{k}"]) for k in json.loads(str(base[f"{tag}_keys"]))}
    return {k: torch.from_numpy(gold["fwd"][f"{tag}/{k}"]) if k.startswith("convinv.") else v for k, v in sd.items()}


def _inputs(gold, n):
    fc = int(gold["forward_case"][n])
    return torch.from_numpy(gold["fwd"][f"mel{fc}"]), torch.from_numpy(gold["fwd"][f"audio{fc}"])


def _model(cfg, sd, removed=False):
    glow = _glow()
    m = glow.WaveGlow(**cfg)
    m.load_state_dict(sd)
    if removed:
        glow.WaveGlow.remove_weightnorm(m)
    return m.cuda().trainable()


def _step(model, mel, audio, value=None):
    """One forward + backward of WaveGlowLoss(SIGMA) (or of value(outputs)): (loss, {name: grad on the CPU}, outputs)."""
    model.zero_grad(set_to_none=True)
    outputs = model((_d(mel), _d(audio)))
    assert outputs[0].grad_fn is not None and all(s.grad_fn is not None for s in outputs[1])
    loss = _glow().WaveGlowLoss(SIGMA)(outputs) if value is None else value(outputs)
    loss.backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    return float(loss.detach()), grads, outputs


def _compare(tag, grads, g64, dev):
    """Every tensor against fp64 within 25 * max(dev[key], 2^-23 * max |g64|); returns the worst err / bound."""
    assert sorted(grads) == sorted(g64)
    worst = 0.0
    for k, ref in g64.items():
        mag = float(ref.abs().max())
        assert mag > 0, k                                     # nothing passes by being zero
        assert grads[k].shape == ref.shape and torch.isfinite(grads[k]).all(), k
        bound = 25 * max(dev[k], ULP * mag)
        ratio = float((grads[k].double() - ref).abs().max()) / bound
        worst = max(worst, ratio)
        assert ratio <= 1.0, (tag, k, ratio)
    print(tag, len(g64), "tensors, worst err/bound", worst)
    return worst


def _cpu_dev(sd, cfg, mel, audio, g64, **kw):
    g32 = GR.grads(sd, cfg, mel, audio, torch.float32, **kw)[0]
    return {k: float((g32[k].double() - g64[k]).abs().max()) for k in g64}


@pytest.mark.parametrize("tag", ["a", "deep"])
def test_gradients_vs_reference_recording_and_fp64(gold, tag):
    """Every tensor of both models on both cases against fp64, within the recorded fp32 deviation of the reference's own gradients
    on that run.  A deviation from the issue, which asks for the reference's gradients of both models on both cases: a committed
    file may not exceed 1 MiB and the four sets are 2.3 MB, so the recording stores the gradients themselves for "a" on the
    first case and for "deep" on the second, with ``upsample.weight`` at every 5th element; the comparison with the recording
    covers what is stored, the comparison with fp64 every element of all four runs."""
    cfg, sd = gold["configs"][tag], _sd(gold, tag)
    keys = json.loads(str(gold[f"{tag}_keys"]))
    stored, stride = json.loads(str(gold["stored"]))[tag], int(gold["up_stride"])
    normed, removed = _model(cfg, sd), _model(cfg, sd, removed=True)
    for n in range(len(gold["cases"])):
        mel, audio = _inputs(gold, n)
        fc = int(gold["forward_case"][n])
        g64, loss64, _ = GR.grads(sd, cfg, mel, audio, torch.float64, sigma=SIGMA)
        dev = dict(zip(keys, (float(v) for v in gold[f"{tag}_dev{n}"])))
        loss, grads, (z, log_s, logdet) = _step(normed, mel, audio)
        _compare(f"{tag} case {n} weight-normed vs fp64", grads, g64, dev)
        assert abs(loss - loss64) <= 25 * max(abs(float(gold[f"{tag}_loss{n}"][0]) - loss64), ULP * abs(loss64))
        # the values of the trainable forward, within the forward tests' bound
        zref, sref = float(gold["fwd"][f"{tag}_z_err{fc}"]), [float(v) for v in gold["fwd"][f"{tag}_log_s_err{fc}"]]
        assert float((z.detach().cpu().double() - torch.from_numpy(gold["fwd"][f"{tag}_z{fc}"]).double()).abs().max()) <= 25 * zref
        for k, s in enumerate(log_s):
            assert float((s.detach().cpu().double() - torch.from_numpy(gold["fwd"][f"{tag}_log_s{fc}_{k}"]).double()).abs().max()) <= 25 * sref[k]
        if n == stored:                                       # the reference's own fp32 gradients
            worst = 0.0
            for k in keys:
                rec, got = torch.from_numpy(gold[f"{tag}_g{n}/{k}"]), grads[k]
                got = got.flatten()[::stride] if k == "upsample.weight" else got
                ratio = float((got.double() - rec.double()).abs().max()) / (25 * max(dev[k], ULP * float(g64[k].abs().max())))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (tag, n, k, ratio)
            print(tag, "case", n, "vs the recording, worst err/bound", worst)
        folded = R.fold(sd)
        f64 = GR.grads(folded, cfg, mel, audio, torch.float64, sigma=SIGMA)[0]
        loss_r, grads_r, _ = _step(removed, mel, audio)
        _compare(f"{tag} case {n} folded vs fp64", grads_r, f64, _cpu_dev(folded, cfg, mel, audio, f64, sigma=SIGMA))


def test_full_width_vs_fp64_restatement():
    cfg = dict(n_mel_channels=80, n_flows=2, n_group=8, n_early_every=1, n_early_size=2, WN_config=dict(n_layers=8, n_channels=256, kernel_size=3))
    sd = FR.skew_mixes(R.make_state_dict(cfg, 287), cfg, 61)
    mel = R.make_mel(1, 2, 41)
    audio = torch.randn(1, 512, generator=torch.Generator().manual_seed(42)) * 0.3
    g64 = GR.grads(sd, cfg, mel, audio, torch.float64, sigma=SIGMA)[0]
    assert len(g64) == 116
    _, grads, _ = _step(_model(cfg, sd), mel, audio)
    _compare("full width", grads, g64, _cpu_dev(sd, cfg, mel, audio, g64, sigma=SIGMA))


def test_general_upstream_gradients_vs_fp64(gold):
    """A seeded random linear functional of z and of each log_s[k], one log_s left out of it entirely; log det W is not part of it,
    so the mixes' gradients come through the flow alone."""
    cfg, sd = gold["configs"]["a"], _sd(gold, "a")
    mel, audio = _inputs(gold, 1)
    B, N = audio.shape
    Lt, g = N // cfg["n_group"], torch.Generator().manual_seed(9)
    cz = torch.randn(B, cfg["n_group"], Lt, generator=g)
    cs = [torch.randn(B, c // 2, Lt, generator=g) for c in R.flow_channels(cfg)]
    cs[1] = None
    g64 = GR.grads(sd, cfg, mel, audio, torch.float64, cz=cz, cs=cs)[0]

    def value(outputs):
        z, log_s, _ = outputs
        total = (_d(cz) * z).sum()
        for s, c in zip(log_s, cs):
            if c is not None:
                total = total + (_d(c) * s).sum()
        return total
    _, grads, _ = _step(_model(cfg, sd), mel, audio, value)
    _compare("general upstream", grads, g64, _cpu_dev(sd, cfg, mel, audio, g64, cz=cz, cs=cs))


SGD_LR = 0.02


def test_three_sgd_steps_follow_the_fp64_run(gold):
    """p -= lr * grad three times.  The loss before every step and after the last, and every parameter at the end, stay within 25 times
    the fp32 CPU run's deviation from the fp64 run of the same steps, floored at 2^-23 * max |p64| (parameters) and 2^-23 * the
    size of the terms the loss adds (waveglow_fwd_ref.loss_magnitude at the start); the loss moves by more than 1 % and decreases."""
    cfg, sd = gold["configs"]["a"], _sd(gold, "a")
    mel, audio = _inputs(gold, 0)
    l64, p64 = GR.sgd_steps(sd, cfg, mel, audio, torch.float64, SIGMA, SGD_LR, 3)
    l32, p32 = GR.sgd_steps(sd, cfg, mel, audio, torch.float32, SIGMA, SGD_LR, 3)
    assert l64[3] < l64[2] < l64[1] < l64[0] and l64[0] - l64[3] > 0.01 * abs(l64[0])
    z, log_s, logdet = FR.forward(R.fold(sd), cfg, mel, audio)
    floor = ULP * FR.loss_magnitude(z, log_s, logdet, SIGMA)
    model, got = _model(cfg, sd), []
    for _ in range(3):
        loss, _, _ = _step(model, mel, audio)
        got.append(loss)
        with torch.no_grad():
            for p in model.parameters():
                p -= SGD_LR * p.grad
    with torch.no_grad():
        got.append(float(_glow().WaveGlowLoss(SIGMA)(model((_d(mel), _d(audio))))))
    print("loss fp64", l64, "fp32 CPU", l32, "GPU", got)
    assert got[3] < got[2] < got[1] < got[0]
    for a, b, c in zip(got, l64, l32):
        assert abs(a - b) <= 25 * max(abs(c - b), floor)
    worst = 0.0
    for k, p in model.state_dict().items():
        bound = 25 * max(float((p32[k].double() - p64[k]).abs().max()), ULP * float(p64[k].abs().max()))
        worst = max(worst, float((p.cpu().double() - p64[k]).abs().max()) / bound)
    print("parameters after three steps, worst err/bound", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("tag, n", [("a", 0), ("deep", 1)])
def test_train_forward_keeps_the_bits_of_forward(gold, tag, n):
    """t2_waveglow_train_forward against t2_waveglow_forward on the same packed buffer: z, every log_s, the fp64 sums and the loss
    bit for bit (the saving epilogues change no arithmetic)."""
    L = _L()
    cfg_d, model = gold["configs"][tag], _model(gold["configs"][tag], _sd(gold, tag))
    mel, audio = (_d(t) for t in _inputs(gold, n))
    cfg = model._config()
    (B, n_mel, T), N = mel.shape, audio.shape[1]
    plan, bplan = L.waveglow_forward_plan(cfg, B, T, N), L.waveglow_backward_plan(cfg, B, T, N)
    with torch.no_grad():
        ts = model._tensors(forward=True)
    packed, logdet_w = _nan(plan.packed_bytes // 4), _nan(cfg.n_flows)
    tp = (C.c_void_p * len(ts))(*[L.ptr(t) for t in ts])
    L.check(L.lib().t2_waveglow_pack(C.byref(cfg), tp, len(ts), L.ptr(packed), L.stream()))
    L.check(L.lib().t2_waveglow_logdet(C.byref(cfg), L.ptr(packed), L.ptr(logdet_w), L.stream()))
    runs = []
    for keep in (False, True):
        ws, z = _nan(plan.workspace_bytes // 4), _nan(B, cfg.n_group, plan.L)
        log_s = [_nan(B, c // 2, plan.L) for c in R.flow_channels(cfg_d)]
        table = (C.c_void_p * len(log_s))(*[L.ptr(t) for t in log_s])
        sums, item, loss = _nan(B, cfg.n_flows + 1, dtype=torch.float64), _nan(B), _nan(1)
        a = L.WaveglowForwardArgs(B, T, n_mel, N, L.ptr(packed), L.ptr(logdet_w), L.ptr(mel), L.ptr(audio), L.ptr(ws), L.ptr(z), table, None, SIGMA,
                                  L.ptr(sums), L.ptr(item), L.ptr(loss), None)
        if keep:
            saved = _nan(bplan.saved_bytes // 4)
            L.check(L.lib().t2_waveglow_train_forward(C.byref(cfg), C.byref(L.WaveglowTrainForwardArgs(a, L.ptr(saved))), L.stream()))
        else:
            L.check(L.lib().t2_waveglow_forward(C.byref(cfg), C.byref(a), L.stream()))
        torch.cuda.synchronize()
        runs.append([z, *log_s, sums, item, loss])
    assert torch.isfinite(saved).all()                          # every float of `saved` is written
    assert all(torch.isfinite(t).all() for t in runs[0]) and all(torch.equal(p, q) for p, q in zip(*runs))


def test_no_grad_takes_the_plain_forward_and_keeps_nothing(gold, monkeypatch):
    """Under torch.no_grad(), and with grad mode on when no parameter requires grad, the trainable model calls t2_waveglow_forward
    and never the saving entry point; with grad mode on and parameters requiring grad it is the other way round.  An output the
    loss does not use reaches t2_waveglow_backward as a null pointer."""
    L = _L()
    lib, calls = L.lib(), []
    plain, keeping, backward = lib.t2_waveglow_forward, lib.t2_waveglow_train_forward, lib.t2_waveglow_backward

    def seen(*args):
        a = args[1]._obj
        calls.append(("backward", bool(a.dz), [bool(a.dlog_s_host[k]) for k in range(args[0]._obj.n_flows)]))
        return backward(*args)
    monkeypatch.setattr(lib, "t2_waveglow_forward", lambda *a: (calls.append("forward"), plain(*a))[1])
    monkeypatch.setattr(lib, "t2_waveglow_train_forward", lambda *a: (calls.append("train_forward"), keeping(*a))[1])
    monkeypatch.setattr(lib, "t2_waveglow_backward", seen)
    cfg, sd = gold["configs"]["a"], _sd(gold, "a")
    model = _model(cfg, sd)
    mel, audio = (_d(t) for t in _inputs(gold, 0))
    assert all(p.requires_grad for p in model.parameters())
    with torch.no_grad():
        z0 = model((mel, audio))[0]
    assert calls == ["forward"] and z0.grad_fn is None
    z, log_s, _ = model((mel, audio))
    assert calls == ["forward", "train_forward"] and torch.equal(z, z0)
    (log_s[0].sum() + 2 * log_s[2].sum()).backward()
    assert calls[2] == ("backward", False, [True, False, True, False])
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for k, p in model.named_parameters() if not k.startswith("convinv.3"))
    for p in model.parameters():
        p.requires_grad_(False)
    del calls[:]
    assert model((mel, audio))[0].grad_fn is None and calls == ["forward"]


def test_two_runs_are_bit_identical(gold):
    cfg, sd = gold["configs"]["deep"], _sd(gold, "deep")
    mel, audio = _inputs(gold, 1)
    model, runs = _model(cfg, sd), []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        times = {}
        outputs = model._train_forward((_d(mel), _d(audio)), kernel_times=times)
        _glow().WaveGlowLoss(SIGMA)(outputs).backward()
        assert set(times["backward"]) == set(_L().WAVEGLOW_BACKWARD_KERNELS) and all(v >= 0 for v in times["backward"].values())
        runs.append((times["arena"].clone(), [p.grad.clone() for p in model.parameters()], outputs[0].detach().clone()))
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_surface(gold):
    glow = _glow()
    cfg, sd = gold["configs"]["a"], _sd(gold, "a")
    mel, audio = (_d(t) for t in _inputs(gold, 0))
    plain = glow.WaveGlow(**cfg)
    plain.load_state_dict(sd)
    plain.cuda()
    with pytest.raises(RuntimeError, match="inference only"):
        plain((mel, audio))
    model = _model(cfg, sd)
    assert model.trainable() is model
    with torch.no_grad():
        z, log_s, logdet = model((mel, audio))
    assert z.grad_fn is None and all(t.grad_fn is None for t in log_s + logdet) and not z.requires_grad
    z2, log_s2, logdet2 = model((mel, audio))
    assert z2.grad_fn is not None and torch.equal(z, z2) and all(torch.equal(a, b) for a, b in zip(log_s, log_s2))
    assert len(log_s) == len(logdet) == cfg["n_flows"] and all(t.dim() == 0 and t.dtype == torch.float32 for t in logdet)
    with torch.no_grad():
        za, sa, lda = model.analyze((mel, audio))
    assert z.shape == za.shape and [t.shape for t in log_s] == [t.shape for t in sa]
    assert all(abs(float(a) - float(b)) <= 1e-5 * abs(float(b)) + 1e-5 for a, b in zip(logdet, lda))
    with pytest.raises(RuntimeError, match="the mel requires grad"):
        model((mel.clone().requires_grad_(True), audio))
    with pytest.raises(RuntimeError, match="the audio requires grad"):
        model((mel, audio.clone().requires_grad_(True)))
    with pytest.raises(RuntimeError, match="backward is not built"):
        model.analyze((mel, audio))
    with pytest.raises(RuntimeError, match="backward is not built"):
        model.nll(mel, audio)
    with pytest.raises(RuntimeError, match="float32"):
        model((mel.half(), audio))
    assert model.trainable(False) is model
    with pytest.raises(RuntimeError, match="inference only"):
        model((mel, audio))
    model.trainable()
    # infer after a training step: the caches notice the version bump
    spect = _d(R.make_mel(1, 3, 5, n_mel=cfg["n_mel_channels"]))
    with torch.no_grad():
        noise = [torch.randn(s, generator=torch.Generator().manual_seed(3)).to(DEV) for s in R.noise_shapes(cfg, 1, 3)]
        before = model.infer(spect, sigma=0.8, noise=noise)
    glow.WaveGlowLoss(SIGMA)(model((mel, audio))).backward()
    with torch.no_grad():
        for p in model.parameters():
            p -= 0.05 * p.grad
        after = model.infer(spect, sigma=0.8, noise=noise)
        fresh = glow.WaveGlow(**cfg)
        fresh.load_state_dict(model.state_dict())
        assert not torch.equal(before, after) and torch.equal(after, fresh.cuda().infer(spect, sigma=0.8, noise=noise))
