"""GPU: every route of the GEMM layer (the plan names of csrc/gemm_dispatch.hip: f32_64, f32_128, bf16conv, src128, src256,
src256km and their split-bf16 "x3" forms) through t2_gemm_ex, against an fp64 product, with the store variants the kernel
families share (csrc/gemm_common.h: direct stores, the row walk through LDS): bias + ReLU + alpha, beta into a random C,
a row map, and C as a column window of a wider zeroed buffer with 16-byte-aligned rows and starting 4 bytes off.  The
split-K shapes run the plain product.  Every case asserts the route it lands on from t2_gemm_plan before it runs.

Bounds: 2e-4 * max(1, sqrt(K) / 8) against fp64 on the exact routes; 2e-3 * max(1, sqrt(K) / 8) against fp64 on the
bf16-rounded operands on the bf16 routes; on the x3 routes the bound of tests/test_gpu_split_gemm.py,
max(8 x the exact kernel's own error, 8 sqrt(K) 2^-17), against fp64 on the unrounded operands."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (route, precision mode, M, N, K, k-major operands (A [K][M], B [K][N]), scratch, row-map divisor of M)
UNSPLIT = [
    ("f32_64", "f32", 65, 33, 40, False, False, 5),
    ("f32_64", "f32", 65, 33, 40, True, False, 5),
    ("f32_128", "f32", 1921, 2047, 24, False, False, 17),
    ("bf16conv", "bf16", 129, 130, 100, False, False, 3),
    ("bf16conv", "bf16", 129, 130, 100, True, False, 3),
    ("src128", "bf16", 384, 384, 192, False, True, 12),
    ("src256", "bf16", 256, 256, 128, False, True, 8),
    ("src256km", "bf16", 256, 256, 128, True, True, 8),
    ("x3src128", "bf16x3", 384, 384, 192, False, True, 12),
    ("x3src256", "bf16x3", 256, 256, 128, False, True, 8),
    ("x3src256km", "bf16x3", 256, 256, 128, True, True, 8),
]
VARIANTS = ["relu", "beta", "rowmap", "window16", "window4"]
# (route, mode, M, N, K, k-major, forced split-K factor (0: the plan's own), the factor the plan must arrive at (0: any > 1))
SPLIT = [
    ("f32_64", "f32", 65, 33, 1040, False, 3, 3),
    ("f32_128", "f32", 130, 129, 1040, False, 0, 0),
    ("bf16conv", "bf16", 129, 130, 1100, False, 3, 3),
    ("src128", "bf16", 384, 384, 1088, False, 3, 3),
    ("src256", "bf16", 256, 256, 448, False, 3, 2),
    ("src256km", "bf16", 256, 256, 448, True, 3, 2),
]


def case_id(c):
    return f"{c[0]}-{c[2]}x{c[3]}x{c[4]}-{'km' if c[5] else 'nt'}"


@pytest.fixture(scope="module")
def L():
    from tacotron2_subword_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def scratch():
    return torch.empty(16 << 20, device="cuda")                         # 64 MB


@functools.lru_cache(maxsize=None)
def operands(M, N, K, km):
    """A, B on the device in the case's layout, a bias and a C to accumulate into, and the fp64 products of the operands as
    they are and rounded to bf16; made once per shape and layout and never written."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + int(km))
    a, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias, c0 = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    prod = a.double() @ b.double().t()
    prod16 = a.bfloat16().double() @ b.bfloat16().double().t()
    A = (a.t().contiguous() if km else a).cuda()
    B = (b.t().contiguous() if km else b).cuda()
    return A, B, bias.cuda(), c0.cuda(), prod, prod16, bias.double(), c0.double()


def gemm_args(L, A, B, out, M, N, K, km, **kw):
    sam, sak = (1, M) if km else (K, 1)
    sbn, sbk = (1, N) if km else (K, 1)
    ws = kw.get("ws")
    return L.GemmArgs(L.ptr(A), L.ptr(B), out.data_ptr(), M, N, K, sam, sak, sbn, sbk, kw.get("ldc", N), 1, 0, 0, 0,
                      kw.get("alpha", 1.0), kw.get("beta", 0.0), L.ptr(kw.get("bias")), kw.get("act", 0), kw.get("crow_mod", 0),
                      kw.get("crow_mul", 0), L.ptr(ws), 0 if ws is None else ws.numel() * 4, kw.get("splitk", 0))


def launch(L, args, route):
    """Runs the product after asserting its route; returns the plan."""
    plan = L.gemm_plan(args)
    assert plan["name"] == route, plan
    L.check(L.lib().t2_gemm_ex(C.byref(args), L.stream()))
    return plan


def run_variant(L, case, variant, route=None):
    """One store variant of an unsplit case in the precision mode in force: (the result, the whole buffer it lies in)."""
    name, _, M, N, K, km, use_ws, rdiv = case
    A, B, bias, c0 = operands(M, N, K, km)[:4]
    ws = scratch() if use_ws else None
    kw = dict(ws=ws)
    buf = torch.empty(M, N, device="cuda")
    out = buf
    if variant == "relu":
        kw.update(bias=bias, act=1, alpha=0.5)
    elif variant == "beta":
        buf.copy_(c0); kw.update(beta=2.0)
    elif variant == "rowmap":
        kw.update(crow_mod=rdiv, crow_mul=M // rdiv)
    else:                                                             # rows of the window 16-byte aligned / 4 bytes off
        ld, off = ((N + 3) // 4 * 4 + 64, 32) if variant == "window16" else (N + 3, 1)
        buf = torch.zeros(M, ld, device="cuda"); out = buf[:, off:off + N]
        kw.update(ldc=ld)
    plan = launch(L, gemm_args(L, A, B, out, M, N, K, km, **kw), route or name)
    assert plan["splitk"] == 1, plan
    return out, buf


def reference(case, variant, prod):
    M, rdiv = case[2], case[7]
    bias64, c064 = operands(*case[2:6])[6:8]
    if variant == "relu":
        return torch.relu(0.5 * prod + bias64)
    if variant == "beta":
        return prod + 2.0 * c064
    if variant == "rowmap":                                           # row m lands at (m % mod) * mul + m / mod
        m = torch.arange(M)
        ref = torch.empty_like(prod); ref[(m % rdiv) * (M // rdiv) + m // rdiv] = prod
        return ref
    return prod


def err(x, ref):
    return float((x.double().cpu() - ref).abs().max())


def set_mode(L, mode):
    """Precision mode `mode`; in "bf16x3" every qualifying product goes to the split route, whatever its size."""
    L.set_precision(mode)
    L.set_gemm_split_min_mflop(0 if mode == "bf16x3" else -1)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", UNSPLIT, ids=case_id)
def test_route_store_variants(L, case, variant):
    name, mode, M, N, K, km = case[:6]
    prod, prod16 = operands(M, N, K, km)[4:6]
    try:
        e0 = None
        if mode == "bf16x3":                                          # the exact kernel's own error is the yardstick
            o0, _ = run_variant(L, case, variant, route="f32_64")
            e0 = err(o0, reference(case, variant, prod))
        set_mode(L, mode)
        out, buf = run_variant(L, case, variant)
    finally:
        set_mode(L, "f32")
    scale = max(1.0, K ** 0.5 / 8.0)
    if mode == "f32":
        ref, bound = reference(case, variant, prod), 2e-4 * scale
    elif mode == "bf16":
        ref, bound = reference(case, variant, prod16), 2e-3 * scale
    else:
        ref, bound = reference(case, variant, prod), max(8.0 * e0, 8.0 * K ** 0.5 * 2.0 ** -17)
    e = err(out, ref)
    print(f"gemm route {case_id(case)} {variant}: max error {e:.3e}  bound {bound:.3e}")
    assert e <= bound, (e, bound)
    if variant.startswith("window"):
        off = 32 if variant == "window16" else 1
        assert buf[:, :off].abs().max().item() == 0.0 and buf[:, off + N:].abs().max().item() == 0.0


@pytest.mark.parametrize("case", SPLIT, ids=case_id)
def test_route_splitk(L, case):
    name, mode, M, N, K, km, force, expect = case
    A, B, _, _, prod, prod16 = operands(M, N, K, km)[:6]
    out = torch.empty(M, N, device="cuda")
    try:
        set_mode(L, mode)
        plan = launch(L, gemm_args(L, A, B, out, M, N, K, km, ws=scratch(), splitk=force), name)
    finally:
        set_mode(L, "f32")
    assert plan["splitk"] == expect if expect else plan["splitk"] > 1, plan
    scale = max(1.0, K ** 0.5 / 8.0)
    ref, bound = (prod, 2e-4 * scale) if mode == "f32" else (prod16, 2e-3 * scale)
    e = err(out, ref)
    print(f"gemm route {case_id(case)} split-K {plan['splitk']}: max error {e:.3e}  bound {bound:.3e}")
    assert e <= bound, (e, bound)
