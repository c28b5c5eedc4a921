"""GPU: the fixed-order column reductions (t2_colsum, the BatchNorm statistics of t2_conv_bn_forward / _backward).

The documented order (csrc/common.h): slabs = 64 if M >= 4096 else max(M // 64, 1) row slabs of ceil(M / slabs) rows;
inside a slab four phases, phase p adding rows m0+p, m0+p+4, ... one after the other from 0; the slab's sum is
((p0 + p1) + p2) + p3; the slabs are added in index order from 0.  Plain fp32 adds are emulated bit-exactly by sequential
torch float32 adds on the CPU (vectorised across slabs and columns), so the plain sums are compared with torch.equal.

The sums whose terms are computed on the way (var, invstd, d(gamma), d(beta)) are compared with an fp64 evaluation of the
same formula on the returned z.  Bound per column: (chain + 68) * 2^-24 * sum|terms|, chain = ceil(rows / 4) the adds of
one phase, 68 = the 4 phase partials + 64 slabs at most; every add contributes at most 2^-24 of the running sum, which
never exceeds sum|terms|.  invstd = (var + eps)^-1/2 turns an error dv of var into at most invstd^3 / 2 * dv, plus three
roundings (add, sqrt, divide) of 2^-24 * invstd each."""
import ctypes as C

import pytest
import torch

from helpers import _partition, ordered_colsum

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def env():
    from tacotron2_subword_amd import _lib as L, blocks
    return L, blocks


def _gpu_colsum(L, base, off, M, N, ld):
    """t2_colsum on the [M, N] view with row stride ld that starts `off` floats into the flat CUDA tensor `base`."""
    out = torch.empty(N, device="cuda")
    sc = torch.empty(64 * N, device="cuda")
    L.check(L.lib().t2_colsum(base.data_ptr() + 4 * off, ld, M, N, L.ptr(out), L.ptr(sc), L.stream()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("M,N,ld,off", [
    (4100, 512, 512, 0),      # 64 slabs of 65 rows, the last one short
    (200, 80, 80, 0),         # 3 slabs, N no multiple of 64
    (63, 6, 6, 0),            # one slab, one column per lane
    (4160, 1, 1, 0),
    (300, 64, 128, 0),        # ld != N
    (260, 64, 64, 1),         # base 4 bytes off a 16-byte boundary
    # The row loop (rows_in_flight, 16 rows per group, two groups a / b in flight) by rows per phase: a phase of a slab of
    # `rows` rows has ceil((rows - p) / 4) of them.  N = 4: one 16-byte group per lane; N = 6, 1: one column per lane.
    (127, 4, 4, 0),           # one slab, phases 32 32 32 31: two groups exactly (a, b, no tail) / one group + a 15-row tail
    (127, 6, 6, 0),
    (8192, 4, 4, 0),          # 64 slabs of 128 rows: 32 per phase
    (8200, 6, 6, 0),          # 129 rows: 33 32 32 32 (a, b, a tail of one row); the last slab has 73
    (8200, 1, 1, 0),
    (12288, 1, 1, 0),         # 192 rows: 48 per phase, b consumed and a requested again
    (12288, 4, 4, 0),
    (12289, 4, 4, 0),         # 193 rows: 49 48 48 48
    (12289, 6, 6, 0),
    (16384, 6, 6, 0),         # 256 rows: 64 per phase, two full rounds
    (16384, 4, 4, 0),
    (16390, 4, 4, 0),         # 257 rows: 65 64 64 64
    (16390, 1, 1, 0),
    (25600, 4, 4, 0),         # the workload's M: 400 rows, 100 per phase (six groups and a 4-row tail)
    (25600, 6, 6, 0),
    (8200, 132, 132, 0),      # the second 128-column tile of the 16-byte kernel is partly outside N
    (12289, 4, 4, 1),         # base 4 bytes off a 16-byte boundary: the one-column kernel through the refill
])
def test_colsum_matches_documented_order(env, M, N, ld, off):
    L, _ = env
    g = torch.Generator().manual_seed(M * 131 + N)
    flat = torch.randn(off + M * ld, generator=g)
    X = flat[off:off + M * ld].view(M, ld)[:, :N].contiguous()
    got = _gpu_colsum(L, flat.cuda(), off, M, N, ld)
    assert torch.equal(got, ordered_colsum(X))


# The ladder of the colsum test for the BatchNorm reductions: 16 rows per group for mean / var (phases of 31/32, 32/33, 47/48,
# 48/49, 64/65 and 100 rows), 8 per group for the backward sums (16/17, 24/25, 32/33 rows: M = 64 * 65, 64 * 97, 64 * 129).
_BN_LADDER = [(1, 127, 4, 4, 5), (4, 1040, 4, 4, 1), (4, 1552, 4, 8, 5), (8, 1032, 4, 4, 1), (8, 1024, 4, 8, 1), (8, 1025, 4, 4, 5),
              (8, 1536, 4, 4, 1), (1, 12289, 4, 8, 5), (16, 1024, 4, 4, 5), (2, 8195, 4, 8, 1), (64, 400, 4, 4, 5), (64, 400, 4, 8, 1),
              (64, 400, 4, 6, 1)]      # Cout = 6: one column per lane (no d(input): the ABI wants Cout % 4 == 0 for it)


@pytest.mark.parametrize("B,T,Cin,Cout,K", [pytest.param(16, 260, 16, 132, 5, id="16-260-16-132"), pytest.param(3, 50, 16, 80, 5, id="3-50-16-80")]
                         + _BN_LADDER)
def test_batchnorm_statistics_order(env, B, T, Cin, Cout, K):
    L, blocks = env
    assert L.get_precision() == "f32"
    M, eps = B * T, 1e-5
    g = torch.Generator().manual_seed(B * 7 + Cout)
    dev = "cuda"
    x = torch.randn(B, T, Cin, generator=g).to(dev)
    w = (torch.randn(Cout, Cin, K, generator=g) * 0.2).to(dev)
    bias = torch.randn(Cout, generator=g).to(dev)
    gamma = (1.0 + 0.3 * torch.randn(Cout, generator=g)).to(dev)
    beta = torch.randn(Cout, generator=g).to(dev)
    rm, rv = torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
    z = torch.empty(M, Cout, device=dev)
    y = torch.empty(B, T, Cout, device=dev)
    st = torch.empty(3, Cout, device=dev)
    ws = torch.empty(Cout * Cin * K + 4 + 128 * Cout + (1 << 20), device=dev)
    a = L.ConvBnArgs(B, T, Cin, Cout, K, L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), 1, eps,
                     blocks.ACT_NONE, 0.0, 1, L.SITE["ENC0"], None, L.ptr(z), L.ptr(st[0]), L.ptr(st[1]), L.ptr(st[2]), L.ptr(y),
                     L.ptr(ws), ws.numel())
    L.check(L.lib().t2_conv_bn_forward(C.byref(a), L.stream()))
    dy = torch.randn(B, T, Cout, generator=g).to(dev)
    dw, db = torch.empty_like(w), torch.empty_like(bias)
    dg, dbt = torch.empty_like(gamma), torch.empty_like(beta)
    dx = torch.empty(B, T, Cin, device=dev) if Cout % 4 == 0 else None
    ws2 = torch.empty(M * Cout + 2 * Cout * Cin * K + 128 * Cout + 16 + (1 << 20) + M * K * max(Cin, Cout), device=dev)
    b = L.ConvBnBwdArgs(B, T, Cin, Cout, K, L.ptr(x), L.ptr(w), L.ptr(gamma), L.ptr(beta), L.ptr(z), L.ptr(st[0]), L.ptr(st[1]), 1, eps,
                        blocks.ACT_NONE, 0.0, 1, L.SITE["ENC0"], L.ptr(dy), L.ptr(dw), L.ptr(db), L.ptr(dg), L.ptr(dbt), L.ptr(dx), 0,
                        L.ptr(ws2), ws2.numel())
    L.check(L.lib().t2_conv_bn_backward(C.byref(b), L.stream()))
    torch.cuda.synchronize()
    zc, mean, invstd, var = z.cpu(), st[0].cpu(), st[1].cpu(), st[2].cpu()

    # MODE 0: plain adds and one correctly rounded division
    assert torch.equal(mean, ordered_colsum(zc) / torch.tensor(float(M), dtype=torch.float32))

    _, rows = _partition(M)
    k = ((rows + 3) // 4 + 68) * U
    z64, m64, i64 = zc.double(), mean.double(), invstd.double()
    d2 = (z64 - m64) ** 2
    var64, var_bound = d2.sum(0) / M, k * d2.sum(0) / M
    e_var = (var.double() - var64).abs()
    inv64 = (var64 + eps) ** -0.5
    inv_bound = 0.5 * inv64 ** 3 * var_bound + 3 * U * inv64
    e_inv = (i64 - inv64).abs()
    xh = (z64 - m64) * i64                                           # the kernel's xhat, from the statistics it was given
    t_g, t_b = dy.cpu().double().view(M, Cout) * xh, dy.cpu().double().view(M, Cout)
    e_dg, e_db = (dg.cpu().double() - t_g.sum(0)).abs(), (dbt.cpu().double() - t_b.sum(0)).abs()
    dg_bound, db_bound = k * t_g.abs().sum(0), k * t_b.abs().sum(0)
    for name, e, bound in (("var", e_var, var_bound), ("invstd", e_inv, inv_bound), ("dgamma", e_dg, dg_bound), ("dbeta", e_db, db_bound)):
        print(f"B={B} T={T} Cout={Cout} {name}: max error / bound = {float((e / bound).max()):.3e}")
        assert bool((e <= bound).all()), (name, float((e / bound).max()))
