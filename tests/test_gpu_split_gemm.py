"""GPU: the split-bf16 GEMM path (precision mode "bf16x3": hi.hi + lo.hi + hi.lo on the bf16-source kernels, one launch,
fp32 accumulate) against an fp64 product of the UNROUNDED fp32 operands.

Error bound (every test below): the mode-0 result's own max error against the same fp64 product is the yardstick, and
the split result must stay within max(8 x that, 8 * sqrt(K) * 2^-17) for unit-scale operands (the scheme's own maximum,
emulated with exact accumulation, is about 3 * sqrt(K) * 2^-17; ONE bf16 term is five hundred times that).  Which kernel
family a product took is read from t2_gemm_counts, not inferred from the error."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from tacotron2_subword_amd import _lib as L, blocks, ops
    return L, blocks, ops


@pytest.fixture(autouse=True)
def every_qualifying_product_goes_split(env):
    """The dispatch keeps products below 2^31 FLOP on the exact kernel (they are faster there); these tests are about
    the split kernels on the small shapes of the bf16 grid, so they lift that threshold.  test_split_threshold_default
    covers the default."""
    L = env[0]
    L.set_gemm_split_min_mflop(0)
    yield
    L.set_gemm_split_min_mflop(-1)


def _ref(A, B, ta, tb):
    a, b = A.double().cpu(), B.double().cpu()
    return (a.t() if ta else a) @ (b.t() if tb else b)


def _bound(e0, K, scale=1.0):
    return max(8.0 * e0, 8.0 * K ** 0.5 * 2.0 ** -17 * scale)


def _err(x, ref):
    return float((x.double().cpu() - ref).abs().max())


@pytest.mark.parametrize("M,N,K", [(256, 384, 192), (512, 256, 4096), (1024, 640, 64), (512, 512, 320), (256, 256, 128), (768, 256, 4160)])
@pytest.mark.parametrize("ta,tb", [(False, True), (False, False), (True, True), (True, False)])
def test_split_gemm_staged_operands(env, M, N, K, ta, tb):
    """The shape x layout grid of test_gemm_bf16_staged_operands (256-tile kernel K-contiguous and k-major, 128-tile
    kernel, even / odd / minimal K-tile counts, split-K for the long K), bias, with scratch: every call takes a
    bf16-source kernel on split operands, and meets the bound."""
    L, blocks, ops = env
    g = torch.Generator().manual_seed(M + N + K + 1)
    A = torch.randn((K, M) if ta else (M, K), generator=g).cuda()
    B = torch.randn((N, K) if tb else (K, N), generator=g).cuda()
    ws = torch.empty(8 * M * N + 3 * (M + N) * K, device="cuda")
    bias = torch.randn(N, generator=g).cuda()
    ref = _ref(A, B, ta, tb) + bias.double().cpu()
    C0 = ops.gemm(A, B, trans_a=ta, trans_b=tb, ws=ws, bias=bias)
    L.set_precision("bf16x3")
    try:
        before = L.gemm_counts()
        C3 = ops.gemm(A, B, trans_a=ta, trans_b=tb, ws=ws, bias=bias)
        mid = L.gemm_counts()
        C3b = ops.gemm(A, B, trans_a=ta, trans_b=tb, ws=ws, bias=bias)
        after = L.gemm_counts()
    finally:
        L.set_precision("f32")
    e0, e3 = _err(C0, ref), _err(C3, ref)
    print(f"split gemm M={M} N={N} K={K} ta={ta} tb={tb}: f32 err {e0:.3e}  bf16x3 err {e3:.3e}  bound {_bound(e0, K):.3e}")
    assert tuple(m - b for m, b in zip(mid, before)) == (0, 0, 0, 1)
    assert tuple(a - m for a, m in zip(after, mid)) == (0, 0, 0, 1)
    assert e3 <= _bound(e0, K), (e3, e0)
    assert torch.equal(C3, C3b)                                      # fixed summation order


def test_split_gemm_tile256_epilogue(env):
    """The 256 x 256 kernel's epilogues on split operands (they are the bf16 mode's code, fed a K' = 3K product): bias +
    relu + alpha, beta = 2 into C, a strided C with aligned and with unaligned rows, explicit split-K 3, an odd K-tile
    count (17 K-tiles -> 51 staged ones)."""
    L, blocks, ops = env
    g = torch.Generator().manual_seed(77)
    M, N, K = 512, 768, 1088
    A = torch.randn(M, K, generator=g).cuda(); B = torch.randn(N, K, generator=g).cuda()
    bias = torch.randn(N, generator=g).cuda(); C0 = torch.randn(M, N, generator=g).cuda()
    ws = torch.empty(8 * M * N + 3 * (M + N) * K, device="cuda")
    prod = A.double().cpu() @ B.double().cpu().t()
    bd, c0d = bias.double().cpu(), C0.double().cpu()

    def run():
        o1 = ops.gemm(A, B, bias=bias, act=1, alpha=0.5, ws=ws)
        o2 = C0.clone(); ops.gemm(A, B, alpha=1.0, beta=2.0, out=o2, ws=ws)
        big = torch.zeros(M, N + 64, device="cuda"); o3 = big[:, 32:32 + N]
        raw = lambda out, b: L.check(L.lib().t2_gemm(A.data_ptr(), B.data_ptr(), out.data_ptr(), M, N, K, K, 1, K, 1, out.stride(0),
                                                     b.data_ptr() if b is not None else None, 0, 1.0, 0.0, ws.data_ptr(), ws.numel() * 4, 0, L.stream()))
        raw(o3, bias)
        odd = torch.zeros(M, N + 3, device="cuda"); o4 = odd[:, 1:1 + N]
        raw(o4, None)
        o5 = ops.gemm(A, B, ws=ws, splitk=3)
        return dict(relu=o1, beta=o2, strided=o3, unaligned=o4, splitk=o5), big, odd

    refs = dict(relu=torch.relu(0.5 * prod + bd), beta=prod + 2.0 * c0d, strided=prod + bd, unaligned=prod, splitk=prod)
    r0, _, _ = run()
    L.set_precision("bf16x3")
    try:
        L.gemm_counts(reset=True)
        r3, big, odd = run()
        counts = L.gemm_counts()
    finally:
        L.set_precision("f32")
    assert counts == (0, 0, 0, 5), counts
    for k in refs:
        e0, e3 = _err(r0[k], refs[k]), _err(r3[k], refs[k])
        print(f"split epilogue {k}: f32 err {e0:.3e}  bf16x3 err {e3:.3e}  bound {_bound(e0, K):.3e}")
        assert e3 <= _bound(e0, K), (k, e3, e0)
    assert big[:, :32].abs().max().item() == 0.0 and big[:, 32 + N:].abs().max().item() == 0.0
    assert odd[:, 0].abs().max().item() == 0.0 and odd[:, 1 + N:].abs().max().item() == 0.0


def test_split_mode_falls_back_to_the_exact_kernel(env):
    """A ragged shape, a whole-tile shape without scratch and a batched product do not qualify for the bf16-source
    kernels: in mode bf16x3 they run an exact fp32 kernel, and the result is bit-identical to mode 0's."""
    L, blocks, ops = env
    g = torch.Generator().manual_seed(3)
    A1 = torch.randn(200, 328, generator=g).cuda(); B1 = torch.randn(130, 328, generator=g).cuda()
    ws1 = torch.empty(16 * 200 * 130 + 3 * 330 * 328, device="cuda")
    A2 = torch.randn(512, 512, generator=g).cuda(); B2 = torch.randn(512, 512, generator=g).cuda()
    A3 = torch.randn(2, 256, 256, generator=g).cuda(); B3 = torch.randn(2, 256, 256, generator=g).cuda()

    def run():
        o1 = ops.gemm(A1, B1, ws=ws1)
        o2 = ops.gemm(A2, B2)
        o3 = torch.empty(2, 256, 256, device="cuda")
        blocks.gemm_ex(A3, B3, o3, 256, 256, 256, 256, 1, 256, 1, 256, batch=2, bsA=256 * 256, bsB=256 * 256, bsC=256 * 256)
        return o1, o2, o3

    r0 = run()
    L.set_precision("bf16x3")
    try:
        L.gemm_counts(reset=True)
        r3 = run()
        counts = L.gemm_counts()
    finally:
        L.set_precision("f32")
    assert counts == (3, 0, 0, 0), counts
    for a, b in zip(r0, r3):
        assert torch.equal(a, b)
    assert _err(r3[2][1], A3[1].double().cpu() @ B3[1].double().cpu().t()) < 2e-4 * 2


def test_split_gemm_is_not_a_single_bf16_product(env):
    """Operands near one (1 + 2^-10 * randn): their bf16 hi parts are almost all exactly 1, so hi.hi alone is wrong at the
    1e-3 level per term (0.3 - 2 absolute at this K); the three-term product still meets the bound."""
    L, blocks, ops = env
    g = torch.Generator().manual_seed(41)
    M = N = 512; K = 1024
    A = (1.0 + 2.0 ** -10 * torch.randn(M, K, generator=g)).cuda()
    B = (1.0 + 2.0 ** -10 * torch.randn(N, K, generator=g)).cuda()
    ws = torch.empty(8 * M * N + 3 * (M + N) * K, device="cuda")
    ref = _ref(A, B, False, True)
    C0 = ops.gemm(A, B, ws=ws)
    L.set_precision("bf16x3")
    try:
        L.gemm_counts(reset=True)
        C3 = ops.gemm(A, B, ws=ws)
        counts = L.gemm_counts()
    finally:
        L.set_precision("f32")
    one_term = _err(A.bfloat16().double().cpu() @ B.bfloat16().double().cpu().t(), ref)
    e0, e3 = _err(C0, ref), _err(C3, ref)
    print(f"near-one operands K={K}: f32 err {e0:.3e}  bf16x3 err {e3:.3e}  one bf16 term {one_term:.3e}  bound {_bound(e0, K):.3e}")
    assert counts == (0, 0, 0, 1), counts
    assert one_term > 0.1                                            # what a single-bf16 product would have given
    assert e3 <= _bound(e0, K), (e3, e0)


@pytest.mark.parametrize("B,T", [(2, 256), (4, 192)])
def test_split_implicit_conv_routes(env, B, T):
    """t2_conv_bn_forward / _backward at Cin = Cout = 512, k = 5, B*T a multiple of 256: the forward product and d(input)
    take the implicit-conv A route, d(weight) the k-major route with the implicit-conv B operand (three whole stacks of
    the frames), all three on split operands; z, dx, dw against mode 0's on the same inputs, utterance edges included.
    Bound: 8 * sqrt(K) * 2^-17 * rms(A) * rms(B) with K = 5 * 512 (z, dx) resp. B * T (dw).  (BatchNorm in eval mode
    with unit statistics is the identity.)"""
    L, blocks, ops = env
    g = torch.Generator().manual_seed(B * 1000 + T)
    C = 512
    conv = torch.nn.Conv1d(C, C, 5, padding=2).cuda()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(C, C, 5, generator=g) * 0.05)
    bn = torch.nn.BatchNorm1d(C).cuda().eval()
    bn.running_mean.zero_(); bn.running_var.fill_(1.0 - bn.eps)
    x0 = torch.randn(B, T, C, generator=g).cuda()
    R = torch.randn(B, T, C, generator=g).cuda()

    def run():
        conv.zero_grad()
        xd = x0.clone().requires_grad_(True)
        y = blocks.conv_bn_stack(xd, [(conv, bn)], [blocks.ACT_NONE], training=False, drop_p=0.0, seed=1, site0=L.SITE["ENC0"])
        (y * R).sum().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), xd.grad.clone(), conv.weight.grad.clone()

    y0, dx0, dw0 = run()
    L.set_precision("bf16x3")
    try:
        L.gemm_counts(reset=True)
        y3, dx3, dw3 = run()
        counts = L.gemm_counts()
    finally:
        L.set_precision("f32")
    assert counts == (0, 0, 0, 3), counts
    rms = lambda t: float(t.double().pow(2).mean().sqrt())
    rx, rw, rd = rms(x0), rms(conv.weight.detach()), rms(R)
    for name, a, b, K, scale in (("z", y3, y0, 5 * C, rx * rw), ("dx", dx3, dx0, 5 * C, rd * rw), ("dw", dw3, dw0, B * T, rd * rx)):
        e = float((a.double() - b.double()).abs().max())
        bound = 8.0 * K ** 0.5 * 2.0 ** -17 * scale
        print(f"split conv B={B} T={T} {name}: |bf16x3 - f32| {e:.3e}  bound {bound:.3e}")
        assert e <= bound, (name, e, bound)
        if name != "dw":
            edges = torch.tensor([0, 1, T - 2, T - 1], device=a.device)
            assert float((a[:, edges].double() - b[:, edges].double()).abs().max()) <= bound
    for tap in (0, 4):                                               # edge taps of d(weight): nothing leaks in from the neighbouring utterance or stack
        assert float((dw3[:, :, tap].double() - dw0[:, :, tap].double()).abs().max()) <= 8.0 * (B * T) ** 0.5 * 2.0 ** -17 * rd * rx


def test_split_threshold_default(env):
    """The default dispatch threshold (2*M*N*K >= 2^31, the measured break-even): a 256-tile product below it runs the
    exact kernel bit-identically to mode 0, one above it takes the split path."""
    L, blocks, ops = env
    L.set_gemm_split_min_mflop(-1)
    g = torch.Generator().manual_seed(8)
    small = (torch.randn(512, 512, generator=g).cuda(), torch.randn(512, 512, generator=g).cuda())          # 0.27 GFLOP
    large = (torch.randn(2048, 2560, generator=g).cuda(), torch.randn(512, 2560, generator=g).cuda())      # 5.4 GFLOP
    ws = torch.empty(16 << 20, device="cuda")
    s0, l0 = ops.gemm(*small, ws=ws), ops.gemm(*large, ws=ws)
    L.set_precision("bf16x3")
    try:
        L.gemm_counts(reset=True)
        s3 = ops.gemm(*small, ws=ws)
        c_small = L.gemm_counts(reset=True)
        l3 = ops.gemm(*large, ws=ws)
        c_large = L.gemm_counts(reset=True)
    finally:
        L.set_precision("f32")
    assert c_small == (1, 0, 0, 0) and torch.equal(s3, s0)
    assert c_large == (0, 0, 0, 1)
    ref = _ref(*large, False, True)
    assert _err(l3, ref) <= _bound(_err(l0, ref), 2560)


@pytest.mark.parametrize("ta,tb", [(False, True), (True, False)])
def test_prof_gemm_in_split_mode(env, ta, tb):
    """t2_prof_gemm in mode bf16x3: ms_total with the split staging on every call, ms_kernel with both hi / lo copies made
    beforehand and handed over (GemmDesc::split16); both leave the product in C; K-contiguous and k-major copies."""
    import ctypes as C
    L, blocks, ops = env
    g = torch.Generator().manual_seed(19)
    M, N, K = 1024, 512, 768
    A = torch.randn((K, M) if ta else (M, K), generator=g).cuda()
    B = torch.randn((N, K) if tb else (K, N), generator=g).cuda()
    out = torch.zeros(M, N, device="cuda")
    ws = torch.empty(8 << 20, device="cuda")
    a = L.GemmArgs()
    a.A, a.B, a.C, a.M, a.N, a.K = A.data_ptr(), B.data_ptr(), out.data_ptr(), M, N, K
    a.sam, a.sak = (1, M) if ta else (K, 1)
    a.sbn, a.sbk = (K, 1) if tb else (1, N)
    a.ldc, a.batch, a.alpha, a.beta = N, 1, 1.0, 0.0
    a.ws, a.ws_bytes, a.splitk = ws.data_ptr(), ws.numel() * 4, 0
    mt, mk = C.c_float(), C.c_float()
    ref = _ref(A, B, ta, tb)
    e0 = _err(ops.gemm(A, B, trans_a=ta, trans_b=tb, ws=ws), ref)
    L.set_precision("bf16x3")
    try:
        L.gemm_counts(reset=True)
        L.check(L.lib().t2_prof_gemm(C.byref(a), 5, C.byref(mt), C.byref(mk), L.stream()))
        counts = L.gemm_counts()
    finally:
        L.set_precision("f32")
    assert counts == (0, 0, 0, 12), counts                           # (1 + 5) calls with staging, (1 + 5) on the copies
    assert _err(out, ref) <= _bound(e0, K)
    assert 0.0 < mk.value <= mt.value * 1.5 and mt.value < 50.0
    with pytest.raises(RuntimeError):                                   # fp32 mode: still refused
        L.check(L.lib().t2_prof_gemm(C.byref(a), 5, C.byref(mt), C.byref(mk), L.stream()))
    # default threshold: this product (0.8 GFLOP) runs the exact kernel in mode bf16x3, so there is no bf16-source kernel
    # to time: refused with a message, nothing launched, instead of the exact kernel's time under the name ms_kernel
    L.set_precision("bf16x3")
    L.set_gemm_split_min_mflop(-1)
    try:
        L.gemm_counts(reset=True)
        with pytest.raises(RuntimeError, match="t2_prof_gemm.*f32_64"):
            L.check(L.lib().t2_prof_gemm(C.byref(a), 5, C.byref(mt), C.byref(mk), L.stream()))
        assert L.gemm_counts() == (0, 0, 0, 0)
    finally:
        L.set_gemm_split_min_mflop(0)
        L.set_precision("f32")
