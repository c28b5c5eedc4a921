"""GPU tests of the SSIM kernels (csrc/ssim.hip) and of the ssim module, against the fp64 restatement tests/ssim_ref.py.

Bound per quantity and case: 2 * max(dev_ref, 2^-23 * max|truth|).  dev_ref is the deviation of the reference's own
fp32 statement from the same statement in fp64 on that case (recorded in tests/golden/ssim.npz for the fixture cases,
computed here on the CPU with the module's _ssim otherwise); the floor is one fp32 rounding of the output; the factor 2
covers a summation order that differs from conv2d's.  On the three silence cases the kernel must also stay within a
tenth of dev_ref (value and dx): that is what the fp64 moments are for.  Every check prints err / bound."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssim_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_ssim import AMPS, NAMES, load_case  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim.npz")
DEV = "cuda"
WORST = {}


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


def M():
    from tacotron2_subword_amd import ssim
    return ssim


def LIB():
    from tacotron2_subword_amd import _lib
    return _lib


def check(group, what, got, truth, dev, factor=2.0, extra=0.0):
    truth = torch.as_tensor(truth, dtype=torch.float64)
    err = float((got.detach().double().cpu() - truth).abs().max())
    bound = factor * max(float(dev), 2.0 ** -23 * float(truth.abs().max())) + extra
    share = err / bound
    WORST[group] = max(WORST.get(group, 0.0), share)
    print(f"[{group}] {what}: err {err:.3e} bound {bound:.3e} err/bound {share:.3f} (worst of group {WORST[group]:.3f})")
    assert err <= bound, (group, what, err, bound)
    return err


def reference(x, y, ws=11, size_average=True, grad=1.0):
    """Truth (ssim_ref, fp64) and dev_ref (the module's torch-op statement on the CPU, fp32 against fp64) of out, map, dx, dy
    for the upstream gradient `grad` (a number, or [B] weights with size_average=False)."""
    Cn = x.shape[1]
    g = torch.as_tensor(grad, dtype=torch.float64)
    dx, dy = R.ssim_grad(x, y, ws, g, size_average)
    truth = dict(out=R.ssim_value(x, y, ws, size_average), map=R.ssim_map(x, y, ws), dx=dx, dy=dy)
    res = {}
    for dt in (torch.float32, torch.float64):
        a, b = x.clone().to(dt).requires_grad_(True), y.clone().to(dt).requires_grad_(True)
        out = M()._ssim(a, b, M().create_window(ws, Cn).to(dt), ws, Cn, size_average)
        (out * g.to(dt)).sum().backward()
        res[dt] = dict(out=out.detach(), map=R.reference_form(x, y, ws, True, dt)[1], dx=a.grad, dy=b.grad)
    dev = {k: float((res[torch.float32][k].double() - res[torch.float64][k]).abs().max()) for k in truth}
    return truth, dev


def run(x, y, ws=11, size_average=True, grad=1.0, need=(True, True)):
    """The public path on device tensors x, y (taken as they are): out, dx, dy (None where not asked)."""
    a = x.detach().requires_grad_(need[0])
    b = y.detach().requires_grad_(need[1])
    out = M().ssim(a, b, ws, size_average)
    if any(need):
        (out * torch.as_tensor(grad, dtype=torch.float32, device=out.device)).sum().backward()
    return out, a.grad, b.grad


def full_check(group, tag, xc, yc, xd, yd, ws=11, size_average=True, grad=1.0):
    truth, dev = reference(xc, yc, ws, size_average, grad)
    out, dx, dy = run(xd, yd, ws, size_average, grad)
    smap = M().ssim_map(xd, yd, ws)
    assert out.dtype == torch.float32 and dx.shape == xd.shape and dy.shape == yd.shape and smap.shape == xd.shape
    for k, got in (("out", out), ("map", smap), ("dx", dx), ("dy", dy)):
        check(group, f"{tag} {k}", got, truth[k], dev[k])
    return out, dx, dy


def randn(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


# ------------------------------------------------------------------------------------------------------------------ fixture
@pytest.mark.parametrize("name", NAMES)
def test_fixture_cases(name):
    z = golden()
    x, y = load_case(z, name)
    xd, yd = x.to(DEV), y.to(DEV)
    dx64, dy64 = R.ssim_grad(x, y, 11)
    dev = {k: float(z[f"{name}_dev_{k}"]) for k in ("value", "items", "map", "dx", "dy")}
    out, dx, dy = run(xd, yd)
    items = M().ssim(xd, yd, 11, False)
    assert out.shape == () and items.shape == (x.shape[0],)
    errs = dict(value=check("fixture", f"{name} value", out, R.ssim_value(x, y, 11), dev["value"]),
                dx=check("fixture", f"{name} dx", dx, dx64, dev["dx"]))
    check("fixture", f"{name} items", items, R.ssim_value(x, y, 11, False), dev["items"])
    check("fixture", f"{name} map", M().ssim_map(xd, yd), R.ssim_map(x, y, 11), dev["map"])
    check("fixture", f"{name} dy", dy, dy64, dev["dy"])
    if name in AMPS:
        # the feature's own condition: fp64 moments keep the kernel within a tenth of the fp32 statement's deviation
        for k in ("value", "dx"):
            ratio = errs[k] / dev[k]
            print(f"[silence] {name} {k}: kernel deviation {errs[k]:.3e} = {ratio:.2e} x dev_ref {dev[k]:.3e}")
            assert errs[k] <= 0.1 * dev[k], (name, k, errs[k], dev[k])


# ------------------------------------------------------------------------------------------------------------------ edges
def _tile():
    p = LIB().ssim_plan(1, 1, 1, 11, 0)
    return p.tile_h, p.tile_w


def _edge_sizes(tile, r=5):
    return sorted({1, 4, 5, 6, 11, tile - 1, tile, tile + 1, tile + r, 2 * tile + 1})


@pytest.mark.parametrize("hi", range(10))
def test_edges_ws11(hi):
    """Every H x W of the two edge lists, B and C cycling through {1, 3} x {1, 3}; x is a view one element off 16-byte
    alignment (a slice [..., 1:] of a wider buffer), y is contiguous."""
    th, tw = _tile()
    hs, wsz = _edge_sizes(th), _edge_sizes(tw)
    assert len(hs) == 10 and len(wsz) == 10 and any(w % 4 for w in wsz)
    H = hs[hi]
    for wi, W in enumerate(wsz):
        B, Cn = ((1, 1), (3, 1), (1, 3), (3, 3))[(hi + wi) % 4]
        wide = randn((B, Cn, H, W + 1), 1000 + 10 * hi + wi)
        y = randn((B, Cn, H, W), 2000 + 10 * hi + wi)
        xd = wide.to(DEV)[..., 1:]
        assert xd.data_ptr() % 16 == 4
        full_check("edges", f"B{B} C{Cn} {H}x{W}", wide[..., 1:], y, xd, y.to(DEV))


@pytest.mark.parametrize("ws", [1, 3, 31])
def test_edges_other_windows(ws):
    th, tw = _tile()
    H, W = th + ws // 2 + 1, tw + ws // 2 + 2
    x, y = randn((2, 3, H, W), 3000 + ws), randn((2, 3, H, W), 3100 + ws)
    full_check("edges", f"ws{ws} {H}x{W}", x, y, x.to(DEV), y.to(DEV), ws)
    x, y = randn((1, 1, 3, 5), 3200 + ws), randn((1, 1, 3, 5), 3300 + ws)         # smaller than the window
    full_check("edges", f"ws{ws} 3x5", x, y, x.to(DEV), y.to(DEV), ws)


# ------------------------------------------------------------------------------------------------------------------ layouts
def test_layouts_run_without_a_copy(monkeypatch):
    """[2,1,80,23] contiguous, and the same data as the transposed view of a [2,23,80] buffer: same results to the bound,
    and the kernels are handed the caller's own pointers and strides."""
    L = LIB()
    x, y = randn((2, 1, 80, 23), 41, 2.0, -5.0), randn((2, 1, 80, 23), 42, 2.0, -5.0)
    seen = []
    real_fwd, real_bwd = L.ssim_forward, L.ssim_backward
    monkeypatch.setattr(L, "ssim_forward", lambda a: (seen.append(("fwd", a.x.p, a.x.row_stride, a.x.col_stride, a.y.p, a.y.row_stride, a.y.col_stride)), real_fwd(a))[1])
    monkeypatch.setattr(L, "ssim_backward", lambda a: (seen.append(("bwd", a.x.p, a.x.row_stride, a.x.col_stride, a.y.p, a.y.row_stride, a.y.col_stride)), real_bwd(a))[1])
    xd, yd = x.to(DEV), y.to(DEV)
    a = full_check("layouts", "contiguous", x, y, xd, yd)
    xt = x[:, 0].transpose(1, 2).contiguous().to(DEV)              # the [2,23,80] buffers
    yt = y[:, 0].transpose(1, 2).contiguous().to(DEV)
    xv, yv = xt.transpose(1, 2).unsqueeze(1), yt.transpose(1, 2).unsqueeze(1)
    assert xv.shape == (2, 1, 80, 23) and xv.stride()[2:] == (1, 80)
    seen.clear()
    b = full_check("layouts", "transposed", x, y, xv, yv)
    assert ("fwd", xt.data_ptr(), 1, 80, yt.data_ptr(), 1, 80) in seen and ("bwd", xt.data_ptr(), 1, 80, yt.data_ptr(), 1, 80) in seen
    assert all(s[1:] == (xt.data_ptr(), 1, 80, yt.data_ptr(), 1, 80) for s in seen)
    seen.clear()
    full_check("layouts", "mixed", x, y, xv, yd)                    # transposed x against contiguous y
    assert all(s[1:] == (xt.data_ptr(), 1, 80, yd.data_ptr(), 23, 1) for s in seen) and seen
    for p, q in zip(a, b):                  # the two orientations take the row and column passes in opposite order: close, not equal
        assert float((p.detach() - q.detach()).abs().max()) <= 2.0 ** -22 * float(p.detach().abs().max())


# ------------------------------------------------------------------------------------------------------------------ upstream gradients
def test_upstream_gradients():
    x, y = randn((3, 2, 21, 70), 51), randn((3, 2, 21, 70), 52)
    xd, yd = x.to(DEV), y.to(DEV)
    full_check("upstream", "scalar -0.5", x, y, xd, yd, grad=-0.5)
    w = [0.25, -2.0, 1.5]
    full_check("upstream", "per-item weights", x, y, xd, yd, size_average=False, grad=w)
    truth, dev = reference(x, y, 11, True, -0.5)
    both = run(xd, yd, grad=-0.5)
    out, dx, dy = run(xd, yd, grad=-0.5, need=(False, True))
    assert dx is None and torch.equal(dy, both[2]) and torch.equal(out, both[0])
    check("upstream", "dy only", dy, truth["dy"], dev["dy"])
    out, dx, dy = run(xd, yd, grad=-0.5, need=(True, False))
    assert dy is None and torch.equal(dx, both[1])
    out, dx, dy = run(xd, yd, need=(False, False))
    assert not out.requires_grad and dx is None and dy is None and torch.equal(out, both[0])


def test_determinism():
    x, y = randn((2, 3, 40, 130), 61).to(DEV), randn((2, 3, 40, 130), 62).to(DEV)
    first, second = run(x, y, grad=0.7), run(x, y, grad=0.7)
    for p, q in zip(first, second):
        assert torch.equal(p, q)
    assert torch.equal(M().ssim_map(x, y), M().ssim_map(x, y))
    assert torch.equal(M().ssim(x, y, 11, False), M().ssim(x, y, 11, False))


# ------------------------------------------------------------------------------------------------------------------ loss
def _loss_inputs(B=2, T=23, seed=5):
    g = torch.Generator().manual_seed(seed)
    mel_t = torch.randn(B, 80, T, generator=g) * 2 - 5
    gate_t = (torch.rand(B, T, generator=g) > 0.8).float()
    mel = mel_t + 0.3 * torch.randn(B, 80, T, generator=g)
    post = mel_t + 0.2 * torch.randn(B, 80, T, generator=g)
    gate = torch.randn(B, T, generator=g)
    return [mel, post, gate], [mel_t, gate_t]


def _three_terms(mel, post, gate, mel_t, gate_t):
    return F.mse_loss(mel, mel_t) + F.mse_loss(post, mel_t) + F.binary_cross_entropy_with_logits(gate.reshape(-1, 1), gate_t.reshape(-1, 1))


def test_loss_with_the_term(monkeypatch):
    from tacotron2_subword_amd.loss_function import Tacotron2Loss
    outs, tgts = _loss_inputs()
    # the three-term loss's own fp32 deviation, computed the same way: fp32 against fp64 on the CPU
    res = {}
    for dt in (torch.float32, torch.float64):
        mel = outs[0].to(dt).clone().requires_grad_(True)
        t = _three_terms(mel, outs[1].to(dt), outs[2].to(dt), tgts[0].to(dt), tgts[1].to(dt))
        t.backward()
        res[dt] = (t.detach(), mel.grad)
    dev3 = [float((res[torch.float32][i].double() - res[torch.float64][i]).abs().max()) for i in (0, 1)]
    x, y = outs[0].unsqueeze(1), tgts[0].unsqueeze(1)
    truth, dev = reference(x, y, 11, True, -1.0)
    total64 = res[torch.float64][0] - truth["out"]
    grad64 = res[torch.float64][1] + truth["dx"][:, 0]
    mel = outs[0].to(DEV).requires_grad_(True)
    crit = Tacotron2Loss(ssim_weight=1.0)
    r = crit((mel, outs[1].to(DEV), outs[2].to(DEV), None, None), (tgts[0].to(DEV), tgts[1].to(DEV), None))
    assert len(r) == 5 and r[3] is None and r[4] is None
    r[0].backward()
    bound3 = lambda d, t: 2 * max(d, 2.0 ** -23 * float(t.abs().max()))
    check("loss", "total", r[0], total64, dev["out"], extra=bound3(dev3[0], res[torch.float64][0]))
    check("loss", "d mel_out", mel.grad, grad64, dev["dx"], extra=bound3(dev3[1], res[torch.float64][1]))
    check("loss", "ssim_loss", crit.ssim_loss, -truth["out"], dev["out"])
    # ssim_weight = 0: the SSIM entry points are not called
    L = LIB()
    calls = []
    for n in ("ssim_plan", "ssim_forward", "ssim_backward"):
        monkeypatch.setattr(L, n, lambda *a, _n=n, **k: calls.append(_n))
    mel0 = outs[0].to(DEV).requires_grad_(True)
    crit0 = Tacotron2Loss(ssim_weight=0.0)
    r0 = crit0((mel0, outs[1].to(DEV), outs[2].to(DEV), None, None), (tgts[0].to(DEV), tgts[1].to(DEV), None))
    r0[0].backward()
    assert calls == [] and crit0.ssim_loss is None
    assert torch.equal(r0[0], _three_terms(mel0, outs[1].to(DEV), outs[2].to(DEV), tgts[0].to(DEV), tgts[1].to(DEV)))


def test_no_grad_allocates_no_backward_scratch(monkeypatch):
    L = LIB()
    x, y = randn((2, 1, 80, 23), 71).to(DEV).requires_grad_(True), randn((2, 1, 80, 23), 72).to(DEV)
    plans, fwds, bwds = [], [], []
    real_plan, real_fwd = L.ssim_plan, L.ssim_forward
    monkeypatch.setattr(L, "ssim_plan", lambda *a: (plans.append(a), real_plan(*a))[1])
    monkeypatch.setattr(L, "ssim_forward", lambda a: (fwds.append((a.need_grad, a.coef)), real_fwd(a))[1])
    monkeypatch.setattr(L, "ssim_backward", lambda a: bwds.append(a))
    with torch.no_grad():
        out = M().ssim(x, y)
        out2 = M().SSIM()(x, y)
    assert not out.requires_grad and torch.equal(out, out2)
    assert [p[4] for p in plans] == [0, 0] and fwds == [(0, None), (0, None)] and bwds == []
    assert real_plan(*plans[0]).map_bytes == 0
    plans.clear(); fwds.clear()
    out3 = M().ssim(x, y)                                           # grad mode, only x requires grad: dx's maps alone
    assert out3.requires_grad and torch.equal(out3.detach(), out)
    assert [p[4] for p in plans] == [1] and fwds[0][0] == 1 and fwds[0][1] is not None
    assert real_plan(*plans[0]).map_bytes == 3 * 8 * x.numel()
