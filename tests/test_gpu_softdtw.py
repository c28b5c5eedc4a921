"""GPU tests of the soft-DTW kernels (csrc/softdtw.hip) and of the SoftDTW module, against the fp64 restatement of
tests/softdtw_ref.py and the vectors recorded from the reference (tests/golden/softdtw.npz).

Bounds.  Values: softmin is 1-Lipschitz in the sup norm, so rounding errors add along a path of at most N + M - 1 cells
without being amplified: |R - R64| <= (N + M) * 2^-24 * (4 * max|R64| + d * max D64) over the finite cells, and infinite
cells are infinite in both.  E, dX, dY: an error in R enters an exponent divided by gamma, so no tight bound can be
derived; the yardstick is the float32 mode of the restatement on the same inputs (the arithmetic of the reference's own
GPU kernel): the max-abs error against fp64 may be at most 4 times that emulation's, plus 1e-6.  Each test prints the
share of the bound it used."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import softdtw_ref as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "softdtw.npz")

# name -> (B, N, M, d, gamma, bandwidth, scale of the N(0,1) inputs); "fixN" take inputs and parameters from the fixture.
# The partition changes at N = 64 k (a further wave) and at N = 1024, 2048, 4096 (a further row per thread): the thin shapes
# sit on both sides.  The long shapes run at gamma = 1 on inputs scaled by 0.3: at gamma = 0.1 on N(0,1) inputs the float32
# recurrence itself no longer delivers E over a thousand frames (the emulation's E error there is 0.3 to 180, beyond E's
# whole range [0, 1]), and a ratio of two such errors would say nothing about the kernel.
CASES = {
    "fix0": None, "fix1": None, "fix2": None, "fix3": None,
    "d80": (2, 65, 64, 80, 0.1, 0, 1.0), "one": (1, 1, 1, 3, 0.1, 0, 1.0), "row": (1, 1, 7, 3, 0.1, 0, 1.0),
    "col": (1, 7, 1, 3, 0.1, 0, 1.0), "wave+1": (1, 64, 65, 4, 1.0, 0, 1.0), "band": (1, 130, 140, 5, 0.1, 20, 1.0),
    "n1024": (1, 1024, 5, 4, 1.0, 0, 0.3), "n1025": (1, 1025, 5, 4, 1.0, 0, 0.3), "m1025": (1, 5, 1025, 4, 1.0, 0, 0.3),
    "n2049": (1, 2049, 6, 4, 1.0, 0, 0.3), "n2100": (1, 2100, 40, 8, 1.0, 0, 0.3), "n4097": (1, 4097, 5, 3, 1.0, 0, 0.3),
    "mel": (1, 300, 280, 80, 1.0, 0, 0.3),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and both restatements of a case, computed once: dict(x, y [B,*,d] float32, gamma, bw, ref64, ref32 (lists per pair))."""
    if name.startswith("fix"):
        g, n = np.load(GOLDEN), int(name[3:])
        x, y = g[f"x{n}"], g[f"y{n}"]
        gamma, bw = float(g["cases"][n][4]), float(g["cases"][n][5])
    else:
        B, N, M, d, gamma, bw, scale = CASES[name]
        rng = np.random.default_rng(sorted(CASES).index(name) + 100)
        x, y = ((rng.standard_normal((B, L, d)) * scale).astype(np.float32) for L in (N, M))
    ref64 = [S.pair(x[b], y[b], gamma, bw) for b in range(x.shape[0])]
    ref32 = [S.pair(x[b], y[b], gamma, bw, np.float32) for b in range(x.shape[0])]
    return dict(x=x, y=y, gamma=gamma, bw=bw, ref64=ref64, ref32=ref32)


def value_bound(r64, N, M, d):
    finite = np.isfinite(r64["R"])
    return (N + M) * 2.0 ** -24 * (4 * np.abs(r64["R"][finite]).max() + d * r64["D"].max())


def hip_raw(x, y, gamma, bw, xl=None, yl=None, D=None):
    """The kernels through the C ABI, with the stored R brought back to row-major: dict(value [B], R [B,N,M], E [B,N,M])."""
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd import soft_dtw_cuda as sd
    X, Y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    B, N, d = X.shape
    M = Y.shape[1]
    plan = L.softdtw_plan(B, N, M, gamma, True)
    Ds = None
    if D is None:
        Ds = torch.empty(plan.d_floats, device="cuda")
        a = L.SoftDtwDistArgs(B, N, M, d, L.ptr(X), L.ptr(Y), L.ptr(Ds))
        L.check(L.lib().t2_softdtw_dist(C.byref(a), L.stream()))
    value, R = sd._run_forward(D, Ds, B, N, M, gamma, bw, xl, yl, True, X.device)
    E = sd._run_backward(D, Ds, R, B, N, M, gamma, bw, xl, yl, X.device)
    rpt, i, j = plan.rows_per_thread, torch.arange(N), torch.arange(M)
    t, k = i // rpt, i % rpt
    Rrow = R.view(B, plan.passes, plan.threads, rpt).cpu()[:, j[None, :] + t[:, None], t[:, None], k[:, None]]
    return dict(value=value.cpu().numpy(), R=Rrow.numpy(), E=E.cpu().numpy())


def hip_module(x, y, gamma, bw, **kw):
    """The module with gradients: (value [B], dX, dY) for grad_output = 1."""
    from tacotron2_subword_amd.soft_dtw_cuda import SoftDTW
    X, Y = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(y).cuda().requires_grad_(True)
    value = SoftDTW(True, gamma=gamma, bandwidth=bw or None)(X, Y, **kw)
    value.sum().backward()
    return value.detach(), X.grad, Y.grad


@pytest.mark.parametrize("name", list(CASES))
def test_values_against_fp64(name):
    c = case(name)
    B, N, d = c["x"].shape
    M = c["y"].shape[1]
    out = hip_raw(c["x"], c["y"], c["gamma"], c["bw"])
    for b in range(B):
        r64 = c["ref64"][b]
        finite = np.isfinite(r64["R"])
        assert np.array_equal(np.isposinf(out["R"][b]), ~finite), "infinite cells must be infinite in both"
        bound = value_bound(r64, N, M, d)
        err = np.abs(out["R"][b][finite] - r64["R"][finite]).max()
        print(f"{name} pair {b}: max |R - R64| = {err:.3e}, bound {bound:.3e}, used {err / bound:.1%}")
        assert err <= bound
        assert out["value"][b] == out["R"][b, N - 1, M - 1]


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_against_fp64(name):
    c = case(name)
    out = hip_raw(c["x"], c["y"], c["gamma"], c["bw"])
    _, dX, dY = hip_module(c["x"], c["y"], c["gamma"], c["bw"])
    got = dict(E=out["E"], dX=dX.cpu().numpy(), dY=dY.cpu().numpy())
    worst = []
    for b in range(c["x"].shape[0]):
        for key in ("E", "dX", "dY"):
            assert np.isfinite(got[key][b]).all()
            err = np.abs(got[key][b] - c["ref64"][b][key]).max()
            emu = np.abs(c["ref32"][b][key].astype(np.float64) - c["ref64"][b][key]).max()
            print(f"{name} pair {b} {key}: error {err:.3e}, float32 emulation {emu:.3e}, ratio {err / emu if emu else 0.0:.2f}")
            worst.append((err, 4 * emu + 1e-6, key, b))
    for err, bound, key, b in worst:
        assert err <= bound, (key, b, err, bound)


@pytest.mark.parametrize("n", range(4))
def test_reference_vectors(n):
    """The CPU test's tolerances (relative 1e-6 on the value, 2e-3 on E) widened by the bounds above."""
    g, c = np.load(GOLDEN), case(f"fix{n}")
    B, N, d = c["x"].shape
    M = c["y"].shape[1]
    out = hip_raw(c["x"], c["y"], c["gamma"], c["bw"])
    for b in range(B):
        want = float(g[f"value{n}"][b])
        assert abs(out["value"][b] - want) <= 1e-6 * abs(want) + value_bound(c["ref64"][b], N, M, d)
        emu = np.abs(c["ref32"][b]["E"].astype(np.float64) - c["ref64"][b]["E"]).max()
        assert np.abs(out["E"][b] - g[f"dD{n}"][b]).max() <= 2e-3 + 4 * emu + 1e-6


RAGGED = [  # (N, M, d, x_lengths, y_lengths): the second batch pads across a partition boundary (two rows per thread, alone one)
    (70, 66, 8, [70, 33, 1, 64], [40, 66, 7, 65]),
    (1030, 12, 4, [1030, 517], [12, 9]),
]


@pytest.mark.parametrize("N,M,d,xl,yl", RAGGED)
def test_ragged_batch_equals_each_pair_alone(N, M, d, xl, yl):
    rng = np.random.default_rng(N)
    B = len(xl)
    x, y = rng.standard_normal((B, N, d)).astype(np.float32), rng.standard_normal((B, M, d)).astype(np.float32)
    value, dX, dY = hip_module(x, y, 0.1, 0, x_lengths=xl, y_lengths=torch.tensor(yl))
    for b in range(B):
        n, m = xl[b], yl[b]
        v1, dX1, dY1 = hip_module(x[b:b + 1, :n], y[b:b + 1, :m], 0.1, 0)
        assert torch.equal(value[b:b + 1], v1)
        assert torch.equal(dX[b, :n], dX1[0]) and torch.equal(dY[b, :m], dY1[0])
        assert not dX[b, n:].any() and not dY[b, m:].any()              # exact zeros in the padding
    raw = hip_raw(x, y, 0.1, 0, torch.tensor(xl, dtype=torch.int32).cuda(), torch.tensor(yl, dtype=torch.int32).cuda())
    for b in range(B):
        assert not raw["E"][b, xl[b]:].any() and not raw["E"][b, :, yl[b]:].any()


@pytest.mark.parametrize("name", ["fix0", "band", "n1025", "n2100"])
def test_no_gradient_forward_and_reruns_are_bit_identical(name):
    from tacotron2_subword_amd.soft_dtw_cuda import SoftDTW
    c = case(name)
    v1, dX1, dY1 = hip_module(c["x"], c["y"], c["gamma"], c["bw"])
    v2, dX2, dY2 = hip_module(c["x"], c["y"], c["gamma"], c["bw"])
    assert torch.equal(v1, v2) and torch.equal(dX1, dX2) and torch.equal(dY1, dY2)
    X, Y = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["y"]).cuda()
    m = SoftDTW(True, gamma=c["gamma"], bandwidth=c["bw"] or None)
    assert torch.equal(m(X, Y), v1)                                       # nothing requires grad: the forward that stores no R
    with torch.no_grad():
        assert torch.equal(m(X.requires_grad_(True), Y), v1)


def _forward_calls(monkeypatch):
    """Records (need_grad, R is None) of every forward launch the module makes."""
    from tacotron2_subword_amd import soft_dtw_cuda as sd
    calls, real = [], sd._run_forward

    def spy(D, Ds, B, N, M, gamma, bandwidth, xl, yl, need_grad, device):
        value, R = real(D, Ds, B, N, M, gamma, bandwidth, xl, yl, need_grad, device)
        calls.append((bool(need_grad), R is None))
        return value, R
    monkeypatch.setattr(sd, "_run_forward", spy)
    return calls


@pytest.mark.parametrize("dist_func", [None, lambda a, b: (a[:, :, None, :] - b[:, None, :, :]).abs().sum(-1)], ids=["euclidean", "dist_func"])
def test_which_forward_runs(monkeypatch, dist_func):
    """The forward that stores no R runs under torch.no_grad() (whatever the inputs require) and when no input requires
    grad; R is stored only when a backward pass can follow.  Values cannot tell the two apart (they are bit-identical), so
    the launches are observed, and under no_grad the allocator's peak stays below the bytes R would take."""
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd.soft_dtw_cuda import SoftDTW
    B, N, M, d = 1, 1400, 1300, 4
    rng = np.random.default_rng(3)
    X, Y = torch.from_numpy(rng.standard_normal((B, N, d)).astype(np.float32)).cuda(), torch.from_numpy(rng.standard_normal((B, M, d)).astype(np.float32)).cuda()
    m = SoftDTW(True, gamma=1.0, dist_func=dist_func)
    calls = _forward_calls(monkeypatch)
    m(X, Y)
    assert calls == [(False, True)]
    Xg = X.clone().requires_grad_(True)
    r_bytes = 4 * L.softdtw_plan(B, N, M, 1.0, True).r_floats
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        v0 = m(Xg, Y)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    assert calls == [(False, True)] * 2
    if dist_func is None:
        assert peak < 2 * r_bytes, (peak, r_bytes)        # the distance scratch (as large as R) is there, R is not
    v1 = m(Xg, Y)
    assert calls == [(False, True)] * 2 + [(True, False)]
    assert torch.equal(v0, v1.detach())
    v1.sum().backward()
    assert Xg.grad is not None and bool(torch.isfinite(Xg.grad).all())


def test_unreachable_end_cell():
    """bandwidth < |N - M|: value +inf, all-zero gradient, as the reference's loops give."""
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((2, 20, 4)).astype(np.float32), rng.standard_normal((2, 30, 4)).astype(np.float32)
    value, dX, dY = hip_module(x, y, 0.1, 5)
    assert torch.isposinf(value).all()
    assert not dX.any() and not dY.any() and not torch.isnan(dX).any() and not torch.isnan(dY).any()
    r64 = S.pair(x[0], y[0], 0.1, 5)
    assert np.isposinf(r64["value"]) and not r64["E"].any()


def test_normalize_against_the_reference():
    from tacotron2_subword_amd.soft_dtw_cuda import SoftDTW
    g = np.load(GOLDEN)
    x, y = g["norm_x"], g["norm_y"]
    X, Y = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(y).cuda()
    value = SoftDTW(True, gamma=0.1, normalize=True)(X, Y)
    value.sum().backward()
    for b in range(x.shape[0]):
        parts = [(S.pair(p, q, 0.1), S.pair(p, q, 0.1, 0.0, np.float32)) for p, q in ((x[b], y[b]), (x[b], x[b]), (y[b], y[b]))]
        vb = sum(value_bound(r64, 24, 24, 8) for r64, _ in parts)
        want = float(g["norm_value"][b])
        assert abs(float(value[b].detach()) - want) <= 1e-6 * max(abs(parts[0][0]["value"]), abs(want)) + vb
        d64, d32 = [r[0]["dX"] - 0.5 * (r[1]["dX"] + r[1]["dY"]) for r in zip(*parts)]
        emu = np.abs(d32 - d64).max()
        # what 2e-3 on every E entry (the CPU test's tolerance against the reference) can move dX_ic by: 2 |dE_ij| |x_ic - y_jc| summed over j
        cpu_tol = 2e-3 * 2 * (np.abs(x[b][:, None] - y[b][None]).sum(1) + np.abs(x[b][:, None] - x[b][None]).sum(1))
        got = X.grad[b].cpu().numpy()
        err = np.abs(got - g["norm_dX"][b])
        err64 = np.abs(got - d64).max()
        print(f"normalize pair {b}: max dX error vs reference {err.max():.3e}, vs fp64 {err64:.3e}, float32 emulation vs fp64 {emu:.3e}")
        assert (err <= cpu_tol + 4 * emu + 1e-6).all()
        assert err64 <= 4 * emu + 1e-6                      # the tight one: the stacking and the -1/2 weights, against fp64


@pytest.mark.parametrize("B,N,M,d", [(2, 45, 52, 6), (1, 1030, 7, 3)])
def test_dist_func_l1(B, N, M, d):
    """A torch distance: the kernels read the caller's row-major D, autograd carries grad * E back through torch."""
    from tacotron2_subword_amd.soft_dtw_cuda import SoftDTW
    rng = np.random.default_rng(N + M)
    x, y = rng.standard_normal((B, N, d)).astype(np.float32), rng.standard_normal((B, M, d)).astype(np.float32)
    l1 = lambda a, b: (a[:, :, None, :] - b[:, None, :, :]).abs().sum(-1)
    X, Y = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(y).cuda()
    value = SoftDTW(True, gamma=0.5, dist_func=l1)(X, Y)
    value.sum().backward()
    for b in range(B):
        D64 = np.abs(x[b].astype(np.float64)[:, None] - y[b].astype(np.float64)[None]).sum(-1)
        r64, r32 = S.pair(None, None, 0.5, D=D64), S.pair(None, None, 0.5, dtype=np.float32, D=D64)
        assert abs(float(value[b]) - r64["value"]) <= value_bound(r64, N, M, d)
        sign = np.sign(x[b].astype(np.float64)[:, None] - y[b].astype(np.float64)[None])       # [N,M,d]
        dX64, dX32 = np.einsum("ij,ijc->ic", r64["E"], sign), np.einsum("ij,ijc->ic", r32["E"].astype(np.float64), sign)
        err, emu = np.abs(X.grad[b].cpu().numpy() - dX64).max(), np.abs(dX32 - dX64).max()
        print(f"L1 pair {b}: dX error {err:.3e}, float32 emulation {emu:.3e}")
        assert err <= 4 * emu + 1e-6


def test_long_input_without_gradient():
    """1500 frames: past the reference's 1024-thread limit, two rows per thread; no R is stored."""
    from tacotron2_subword_amd.soft_dtw_cuda import SoftDTW
    rng = np.random.default_rng(1500)
    x, y = rng.standard_normal((1, 1500, 8)).astype(np.float32), rng.standard_normal((1, 1500, 8)).astype(np.float32)
    D64 = S.sqdist(x[0], y[0])
    R64 = S.forward(D64, 0.1)
    with torch.no_grad():
        value = SoftDTW(True, gamma=0.1)(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    bound = value_bound(dict(R=R64[1:-1, 1:-1], D=D64), 1500, 1500, 8)
    err = abs(float(value[0]) - R64[1500, 1500])
    print(f"N = M = 1500: value {float(value[0]):.4f}, fp64 {R64[1500, 1500]:.4f}, error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
