"""GPU: the element-wise and reduction kernels of one Conv1d + BatchNorm layer (t2_conv_bn_forward / t2_conv_bn_backward, mode
f32) against plain fp64 torch on the CPU, at the edges of their control flow: both lane widths (16-byte groups, V = 4, and one
column per lane, V = 1), the two mixed, column tiles partly outside C, few rows, the refilled row groups of the reductions, and
the second pass of the grid-stride loops of bn_apply_kernel / bn_bwd_dz_kernel with a channel index that moves.

Whatever depends only on z, mean and invstd is evaluated in fp64 FROM THE VALUES THE LIBRARY RETURNED, so the rounding of the
GEMMs stays out of the element-wise bounds.  With xh = (z - mean) * invstd, u = xh * gamma + beta, keep the exported dropout mask
(ops.rng_keep_mask), s = 1 / (1 - p):
    y  = keep * s * act(u) (+ residual)            du = dy * keep * s * act'(u)
    d(beta) = sum du      d(gamma) = sum du * xh
    dz = gamma * invstd * (du - d(beta) / M - xh * d(gamma) / M)   (training)        dz = du * gamma * invstd   (eval)
    d(bias) = sum dz;   dw, dx: fp64 F.conv1d and its autograd with the returned dz as the incoming gradient.
dz is read where t2_conv_bn_backward leaves it: the first B*T*Cout floats of its workspace.

Bounds.  U = 2^-24 is the largest relative error of one fp32 operation; second-order terms are dropped, every count below has
at least one rounding to spare.  mag = |xh * gamma| + |beta|.
  u: the computed xh carries two roundings (subtract, multiply) and the fma one more: |du_| <= 3U * mag.
  y: ReLU and the identity add nothing; the dropout scale is one rounding, the residual add one, each of a value of at most
     s * mag (+ |residual|): 5 roundings, taken as 6U * (mag + |residual|) * s.
     tanh is 1-Lipschitz, so the error of u passes through unamplified, and |tanh u| <= |u| <= mag keeps the other terms as they
     are; the device's tanhf adds an allowance of TANH_ABS = 4U absolute (|tanh| <= 1; the installed ROCm ships no accuracy table
     for its math functions, so the allowance is the stated one and the largest error / bound ratio is printed): + 4U * s.
  ReLU at the kink: an element with |u| <= 8U * mag may take either branch in fp32; it is left out of the y and dz checks (fewer
     than 1e-4 of the layer, asserted), and |dy * keep * s| of it is added to the bounds of the sums it enters.
  du: dropout scale, 1 - t*t (one fma) and the product: 3U * |du|; for tanh an error et = 3U * mag + 4U of t changes 1 - t*t by
     at most 2 * |t| * et <= 2 * et: + 2 * |dy * keep * s| * et.
  column sums (mean, var, d(beta), d(gamma), d(bias)): k * sum|terms| with k = (ceil(rows / 4) + 68) * U as derived in
     test_gpu_colsum_order.py, plus the sum of the terms' own bounds: (z - mean)^2 carries 2U (the subtraction, squared; the
     square is fused into the add), du * xh carries bound(du) * |xh| + 3U * |du * xh|.  mean and var have one division more.
  invstd = (var + eps)^-1/2: invstd^3 / 2 * bound(var) + 3U * invstd (add, square root, divide).
  dz: the two fma roundings act on values of at most inner = |du| + |d(beta)| / M + |xh * d(gamma)| / M; 1/M is rounded (U),
     xh * d(gamma) has the two roundings of xh and its own, and the sums enter with their bounds:
     |gamma * invstd| * (bound(du) + (bound(d(beta)) + 2U |d(beta)|) / M + |xh| * (bound(d(gamma)) + 4U |d(gamma)|) / M + 2U * inner)
     + 2U * |dz| for the last two products.  Eval: |gamma * invstd| * bound(du) + 2U * |dz|.
  z, dw, dx: the classical dot-product bound (k + 8) * U * (|A| . |B|) per element, k the length of the sums (K * Cin, M,
     K * Cout), |A| . |B| the same convolution on absolute values; an accumulated dx adds one rounding of |dx0| + |A| . |B|.
  running statistics: momentum 0.1f and 1 - 0.1f are within U and 2U of 0.1 and 0.9, each product and the sum round once:
     4U * (0.9 |old| + 0.1 |new|); the unbiased variance has a division and a product more: 6U.
  y16: bit-equal to bf16(y), round to nearest even."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from helpers import _partition

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TANH_ABS = 4 * U
EPS = 1e-5
NONE, RELU, TANH = 0, 1, 2
GRID_CAP = 8192 * 256          # threads of the capped grid of bn_apply_kernel / bn_bwd_dz_kernel: a pass covers GRID_CAP * V elements


@pytest.fixture(scope="module")
def env():
    from tacotron2_subword_amd import _lib as L, blocks, ops
    assert (blocks.ACT_NONE, blocks.ACT_RELU, blocks.ACT_TANH) == (NONE, RELU, TANH)
    return L, ops


def _dev(t, off=0):
    """t on the GPU, `off` elements past an allocation's start (off = 1: 4 bytes off for fp32, 2 bytes for bf16)."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v


def _where(m, c, M, Cout):
    slabs, rows = _partition(M)
    slab, r = divmod(m, rows)
    i = m * Cout + c
    return (f"(row {m}, channel {c}): slab {slab} of {slabs} ({rows} rows each), phase {r % 4}, row {r // 4} of the phase "
            f"(16-row group {r // 4 // 16}, 8-row group {r // 4 // 8}); element {i}: pass {i // (GRID_CAP * 4)} of the 16-byte kernels, "
            f"{i // GRID_CAP} of the one-column kernels")


class _Check:
    def __init__(self, tag, M, Cout):
        self.tag, self.M, self.Cout, self.ratios = tag, M, Cout, {}

    def __call__(self, name, got, ref, bound, skip=None):
        """|got - ref| <= bound everywhere but `skip`; [M, Cout] arrays name the first offending row and channel."""
        e = (got.double() - ref).abs()
        ratio = torch.where(bound > 0, e / bound, torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
        if skip is not None:
            ratio = torch.where(skip, torch.zeros_like(ratio), ratio)
        worst = float(ratio.max()) if ratio.numel() else 0.0
        self.ratios[name] = worst
        print(f"{self.tag} {name}: max error / bound = {worst:.3e}")
        if not worst <= 1.0:                                           # also catches NaN
            i = int((~(ratio <= 1.0)).flatten().nonzero()[0])
            if tuple(got.shape) == (self.M, self.Cout):
                at = _where(i // self.Cout, i % self.Cout, self.M, self.Cout)
            else:
                at = f"flat index {i} of shape {tuple(got.shape)}" + (f" (channel {i})" if got.numel() == self.Cout else "")
            raise AssertionError(f"{self.tag} {name}: error / bound = {worst:.3e}, first at {at}: got {float(got.flatten()[i])!r}, "
                                 f"reference {float(ref.flatten()[i])!r}, bound {float(bound.flatten()[i]):.3e}")


def _conv64(x, w, bias, K):
    """x [B, T, Cin], w [Cout, Cin, K] -> [B, T, Cout] (fp64)"""
    return F.conv1d(x.transpose(1, 2), w, bias, padding=K // 2).transpose(1, 2)


def _conv_grads64(x, w, g, K):
    """(d(x), d(w)) of sum(conv(x, w) * g)"""
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    _conv64(x, w, None, K).backward(g)
    return x.grad, w.grad


def run_case(env, tag, B, T, Cin, Cout, K, act, drop_p=0.0, training=1, residual=False, dx="new", mis=(), y16=None, seed=1,
             site="POSTNET0"):
    """One forward and one backward call; every array they write against fp64.  dx: "new", "acc" (accumulate onto randn) or None.
    mis: which of stats / gamma / beta / dgamma / dbeta sit 4 bytes off a 16-byte boundary.  y16: None, 0 or 1 (2 bytes off)."""
    L, ops = env
    assert L.get_precision() == "f32"
    M, n = B * T, B * T * Cout
    drop_p = drop_p if training else 0.0                               # as blocks.py calls it
    g = torch.Generator().manual_seed(seed * 1000003 + M * 131 + Cout)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, w, bias = rn(B, T, Cin), rn(Cout, Cin, K) * 0.2, rn(Cout)
    gamma, beta = 1.0 + 0.3 * rn(Cout), rn(Cout)
    rm0, rv0 = torch.rand(Cout, generator=g) * 0.2 - 0.1, 0.5 + torch.rand(Cout, generator=g)
    res = rn(B, T, Cout) if residual else None
    dy = rn(B, T, Cout)
    dx0 = rn(B, T, Cin) if dx == "acc" else None
    off = lambda name: 1 if name in mis else 0

    xd, wd, biasd, dyd = _dev(x), _dev(w), _dev(bias), _dev(dy)
    gammad, betad = _dev(gamma, off("gamma")), _dev(beta, off("beta"))
    rmd, rvd = _dev(rm0), _dev(rv0)
    resd = _dev(res) if residual else None
    st = _dev(torch.zeros(3, Cout), off("stats"))
    if "stats" in mis:
        assert all(st[i].data_ptr() % 16 == 4 for i in range(3))
    zd, yd = torch.empty(M, Cout, device="cuda"), torch.empty(B, T, Cout, device="cuda")
    y16d = _dev(torch.zeros(B, T, Cout, dtype=torch.bfloat16), y16) if y16 is not None else None
    ws = torch.empty(Cout * Cin * K + 4 + 128 * Cout + (1 << 20), device="cuda")
    seed64 = 0x1234567 + seed
    a = L.ConvBnArgs(B, T, Cin, Cout, K, L.ptr(xd), L.ptr(wd), L.ptr(biasd), L.ptr(gammad), L.ptr(betad), L.ptr(rmd), L.ptr(rvd),
                     training, EPS, act, drop_p, seed64, L.SITE[site], L.ptr(resd), L.ptr(zd), L.ptr(st[0]), L.ptr(st[1]), L.ptr(st[2]),
                     L.ptr(yd), L.ptr(ws), ws.numel(), None, L.ptr(y16d), 0)
    L.check(L.lib().t2_conv_bn_forward(C.byref(a), L.stream()))
    dwd, dbd = torch.empty_like(wd), torch.empty_like(biasd)
    dgd, dbtd = _dev(torch.zeros(Cout), off("dgamma")), _dev(torch.zeros(Cout), off("dbeta"))
    dxd = None if dx is None else (_dev(dx0) if dx == "acc" else torch.empty(B, T, Cin, device="cuda"))
    ws2 = torch.empty(n + 2 * Cout * Cin * K + 128 * Cout + 16 + (1 << 20) + M * K * max(Cin, Cout), device="cuda")
    b = L.ConvBnBwdArgs(B, T, Cin, Cout, K, L.ptr(xd), L.ptr(wd), L.ptr(gammad), L.ptr(betad), L.ptr(zd), L.ptr(st[0]), L.ptr(st[1]),
                        training, EPS, act, drop_p, seed64, L.SITE[site], L.ptr(dyd), L.ptr(dwd), L.ptr(dbd), L.ptr(dgd), L.ptr(dbtd),
                        L.ptr(dxd), int(dx == "acc"), L.ptr(ws2), ws2.numel(), None, 0)
    L.check(L.lib().t2_conv_bn_backward(C.byref(b), L.stream()))
    keep = ops.rng_keep_mask(seed64, L.SITE[site], n, drop_p) if drop_p > 0 else None
    torch.cuda.synchronize()

    chk = _Check(tag, M, Cout)
    d = lambda t: t.detach().cpu().double()
    slabs, rows = _partition(M)
    k = ((rows + 3) // 4 + 68) * U
    z, mean, inv = d(zd), d(st[0]), d(st[1])
    x64, w64, dy64 = d(xd), d(wd), d(dyd).view(M, Cout)
    ga, be = d(gammad), d(betad)

    # the convolution
    z_ref = _conv64(x64, w64, d(biasd), K).reshape(M, Cout)
    z_abs = _conv64(x64.abs(), w64.abs(), d(biasd).abs(), K).reshape(M, Cout)
    chk("z", zd.cpu(), z_ref, (K * Cin + 8) * U * z_abs)

    # statistics
    if training:
        mean_ref = z.sum(0) / M
        chk("mean", st[0].cpu(), mean_ref, (k + U) * z.abs().sum(0) / M)
        d2 = (z - mean) ** 2
        var_ref, var_bound = d2.sum(0) / M, (k + 3 * U) * d2.sum(0) / M
        chk("var", st[2].cpu(), var_ref, var_bound)
        inv_ref = (var_ref + EPS) ** -0.5
        chk("invstd", st[1].cpu(), inv_ref, 0.5 * inv_ref ** 3 * var_bound + 3 * U * inv_ref)
        unb = d(st[2]) * (M / (M - 1) if M > 1 else 1.0)
        rm_ref, rv_ref = 0.9 * d(rm0) + 0.1 * mean, 0.9 * d(rv0) + 0.1 * unb
        chk("run_mean", rmd.cpu(), rm_ref, 4 * U * (0.9 * rm0.double().abs() + 0.1 * mean.abs()))
        chk("run_var", rvd.cpu(), rv_ref, 6 * U * (0.9 * rv0.double().abs() + 0.1 * unb.abs()))
    else:
        assert torch.equal(st[0].cpu(), rm0) and torch.equal(rmd.cpu(), rm0) and torch.equal(rvd.cpu(), rv0), f"{tag}: eval statistics"
        inv_ref = (rv0.double() + EPS) ** -0.5
        chk("invstd", st[1].cpu(), inv_ref, 3 * U * inv_ref)

    # forward, element-wise
    xh = (z - mean) * inv
    mag = (xh * ga).abs() + be.abs()
    u = xh * ga + be
    s = 1.0 / (1.0 - drop_p) if drop_p > 0 else 1.0
    ks = keep.cpu().double().view(M, Cout) * s if keep is not None else torch.ones(M, Cout, dtype=torch.float64)
    if act == TANH:
        t = torch.tanh(u)
        av, da = t, 1.0 - t * t
    elif act == RELU:
        av, da = u.clamp(min=0.0), (u > 0).double()
    else:
        av, da = u, torch.ones_like(u)
    kink = (u.abs() <= 8 * U * mag) if act == RELU else None
    if kink is not None:
        print(f"{tag} elements at the ReLU kink: {int(kink.sum())} of {n}")
        assert int(kink.sum()) < 1e-4 * n, f"{tag}: {int(kink.sum())} of {n} elements at the ReLU kink"
    r64 = d(resd).view(M, Cout) if residual else torch.zeros(M, Cout, dtype=torch.float64)
    y_bound = 6 * U * (mag + r64.abs()) * s + (TANH_ABS * s if act == TANH else 0.0)
    ycpu = yd.cpu().view(M, Cout)
    chk("y_tanh" if act == TANH else "y", ycpu, ks * av + r64, y_bound, skip=kink)
    if y16 is not None:
        got16, want16 = y16d.cpu().view(M, Cout), ycpu.bfloat16()
        if not torch.equal(got16, want16):
            i = int((got16.view(torch.int16) != want16.view(torch.int16)).flatten().nonzero()[0])
            raise AssertionError(f"{tag} y16 != bf16(y), first at {_where(i // Cout, i % Cout, M, Cout)}: "
                                 f"{float(got16.flatten()[i])!r} for y = {float(ycpu.flatten()[i])!r}")

    # backward: du, the two sums, dz
    g0 = dy64 * ks
    du = g0 * da
    du_bound = 3 * U * du.abs()
    if act == TANH:
        du_bound = du_bound + 2 * g0.abs() * (3 * U * mag + TANH_ABS)
    kg = torch.where(kink, g0.abs(), torch.zeros_like(g0)) if kink is not None else torch.zeros_like(g0)
    db_ref = du.sum(0)
    db_bound = k * du.abs().sum(0) + du_bound.sum(0) + kg.sum(0)
    chk("dbeta", dbtd.cpu(), db_ref, db_bound)
    tx = du * xh
    dg_ref = tx.sum(0)
    dg_bound = k * tx.abs().sum(0) + (du_bound * xh.abs() + 3 * U * tx.abs()).sum(0) + (kg * xh.abs()).sum(0)
    chk("dgamma", dgd.cpu(), dg_ref, dg_bound)
    c = ga * inv
    if training:
        dz_ref = c * (du - db_ref / M - xh * dg_ref / M)
        inner = du.abs() + db_ref.abs() / M + (xh * dg_ref).abs() / M
        dz_bound = c.abs() * (du_bound + (db_bound + 2 * U * db_ref.abs()) / M + xh.abs() * (dg_bound + 4 * U * dg_ref.abs()) / M
                              + 2 * U * inner) + 2 * U * dz_ref.abs()
    else:
        dz_ref = c * du
        dz_bound = c.abs() * du_bound + 2 * U * dz_ref.abs()
    dzcpu = ws2[:n].cpu().view(M, Cout)
    chk("dz", dzcpu, dz_ref, dz_bound, skip=kink)
    chk("dbias", dbd.cpu(), dz_ref.sum(0), k * dz_ref.abs().sum(0) + dz_bound.sum(0) + (c.abs() * kg).sum(0))

    # the two products of the backward pass, from the dz they were given
    dz64 = dzcpu.double().view(B, T, Cout)
    dx_ref, dw_ref = _conv_grads64(x64, w64, dz64, K)
    dx_abs, dw_abs = _conv_grads64(x64.abs(), w64.abs(), dz64.abs(), K)
    chk("dw", dwd.cpu(), dw_ref, (M + 8) * U * dw_abs)
    if dx is not None:
        bound = (K * Cout + 8) * U * dx_abs
        if dx == "acc":
            dx_ref, bound = dx_ref + dx0.double(), bound + U * (dx0.double().abs() + dx_abs)
        chk("dx", dxd.cpu(), dx_ref, bound)
    return chk.ratios


def _matrix():
    cases = []
    for act in (NONE, RELU, TANH):
        for training, drop_p in ((1, 0.0), (1, 0.5), (0, 0.0)):
            for residual in (False, True):
                cases.append((act, drop_p, training, residual, "new"))
    # dx accumulated onto a filled array on two of them, no dx on one
    cases += [(RELU, 0.5, 1, True, "acc"), (TANH, 0.0, 0, False, "acc"), (NONE, 0.5, 1, False, None)]
    return cases


@pytest.mark.parametrize("act,drop_p,training,residual,dx", _matrix())
def test_semantics_matrix(env, act, drop_p, training, residual, dx):
    run_case(env, f"matrix act={act} p={drop_p} training={training} residual={int(residual)} dx={dx}:", 3, 50, 16, 80, 5, act,
             drop_p, training, residual, dx, seed=1 + act)


# Cout = 70: three one-column tiles of 32 lanes, the last with 6 live.  Cout = 6, M = 260: four slabs of 65 rows.  No d(input):
# the ABI wants Cout % 4 == 0 for it (test_dx_needs_cout_multiple_of_4).
@pytest.mark.parametrize("B,T,Cout,act,drop_p,training", [(3, 50, 70, TANH, 0.5, 1), (3, 50, 70, RELU, 0.0, 0), (4, 65, 6, RELU, 0.5, 1),
                                                          (4, 65, 6, TANH, 0.0, 1)])
def test_one_column_kernels(env, B, T, Cout, act, drop_p, training):
    run_case(env, f"V=1 M={B * T} Cout={Cout} act={act} training={training}:", B, T, 16, Cout, 5, act, drop_p, training, True, None,
             y16=1 if Cout == 70 else None, seed=7)


def test_dx_needs_cout_multiple_of_4(env):
    L, _ = env
    B, T, Cin, Cout, K = 4, 65, 16, 6, 5
    t = lambda *s: torch.zeros(*s, device="cuda")
    ws2 = t(B * T * Cout + 2 * Cout * Cin * K + 128 * Cout + 16 + (1 << 20))
    b = L.ConvBnBwdArgs(B, T, Cin, Cout, K, L.ptr(t(B, T, Cin)), L.ptr(t(Cout, Cin, K)), L.ptr(t(Cout)), L.ptr(t(Cout)), L.ptr(t(B * T, Cout)),
                        L.ptr(t(Cout)), L.ptr(t(Cout)), 1, EPS, NONE, 0.0, 1, L.SITE["ENC0"], L.ptr(t(B, T, Cout)), L.ptr(t(Cout, Cin, K)),
                        L.ptr(t(Cout)), L.ptr(t(Cout)), L.ptr(t(Cout)), L.ptr(t(B, T, Cin)), 0, L.ptr(ws2), ws2.numel(), None, 0)
    with pytest.raises(RuntimeError, match=r"conv_bn_bwd: Cout=6 must be a multiple of 4"):
        L.check(L.lib().t2_conv_bn_backward(C.byref(b), L.stream()))
    torch.cuda.synchronize()


# the column reductions read z in 16-byte groups, bn_apply_kernel and / or bn_bwd_dz_kernel fall back to one column per lane
@pytest.mark.parametrize("mis", [("stats",), ("dgamma",), ("dbeta",), ("gamma",), ("beta",)])
def test_mixed_widths(env, mis):
    run_case(env, f"mixed off={mis[0]}:", 3, 50, 16, 80, 5, TANH, 0.5, 1, True, "new", mis=mis, seed=11)


@pytest.mark.parametrize("y16", [0, 1])
def test_bf16_copy(env, y16):
    run_case(env, f"y16 {'2 bytes off' if y16 else 'aligned'}:", 3, 50, 16, 80, 5, RELU, 0.5, 1, True, "new", y16=y16, seed=13)


# phases without a row, var = 0 -> invstd = eps^-1/2 (M = 1), the M - 1 guard of the running variance
@pytest.mark.parametrize("B,T,act,training", [(1, 1, TANH, 1), (3, 1, RELU, 1), (1, 3, TANH, 1), (1, 5, RELU, 1), (5, 1, NONE, 0)])
def test_few_rows(env, B, T, act, training):
    r = run_case(env, f"few rows B={B} T={T} act={act} training={training}:", B, T, 16, 80, 5, act, 0.5, training, True, "new", seed=17)
    assert all(v <= 1.0 for v in r.values())


# n = M * Cout exceeds one pass of the capped grid (8192 * 256 * V elements), and the pass's stride is no multiple of the 80
# channels (2^23 mod 80 = 48, 2^21 mod 80 = 32): the channel index moves and wraps.  M = 105000 also has 411 rows per phase.
@pytest.mark.parametrize("B,T,mis,y16", [(100, 1050, (), 0), (100, 263, ("stats",), None)])
def test_second_pass_moving_channel(env, B, T, mis, y16):
    n, V = B * T * 80, 1 if mis else 4
    assert n > GRID_CAP * V and (GRID_CAP * V) % 80 != 0
    run_case(env, f"second pass V={V} M={B * T}:", B, T, 4, 80, 1, TANH, 0.5, 1, False, None, mis=mis, y16=y16, seed=19)
