"""CPU-only: the hand-over rule of the conv stacks (csrc/gemm_dispatch.hip gemm_handoff) through t2_gemm_plan / t2_conv_handoff_plan.

A conv layer may hand the GEMM layer bf16 copies it wrote itself (the previous layer's output, dz, the re-laid-out weights)
only where the product then runs exactly as it would have on copies staged by gemm(): the plan without copies stages the
operands in question, and the plan with them names the same kernel, split-K factor and K-chunks per split.  Nothing is
launched; the pointers count for their alignment only."""
import pytest

PLACEHOLDER = dict(A=0x10000000, B=0x20000000, C=0x30000000, ws=0x40000000)
WS = 64 << 20


def conv_a_product(L, M, N, K, conv_T, conv_C, ws=WS):
    """The forward / d(input) product of a conv layer: A = frames [M][conv_C] (implicit im2col), B = weights [N][K]."""
    a = L.GemmArgs()
    a.A, a.B, a.C, a.M, a.N, a.K = PLACEHOLDER["A"], PLACEHOLDER["B"], PLACEHOLDER["C"], M, N, K
    a.sam, a.sak, a.sbn, a.sbk, a.ldc, a.batch, a.alpha, a.beta = 0, 1, K, 1, N, 1, 1.0, 0.0
    a.ws, a.ws_bytes = PLACEHOLDER["ws"], ws
    plain = dict(conv_a=1, conv_T=conv_T, conv_C=conv_C)
    offered = dict(plain, a16=1, lda16=conv_C, b16=1, ldb16=K)
    return a, plain, offered


@pytest.fixture
def bf16_mode():
    from tacotron2_subword_amd import _lib as L
    L.set_precision("bf16")
    yield L
    L.set_precision("f32")


ROUTE = ("name", "kernel", "split", "splitk", "kchunks")

TAKEN = [
    (25600, 512, 2560, 400, 512),      # the three conv_a shapes of the training bench
    (6400, 512, 2560, 100, 512),
    (3840, 512, 2560, 60, 512),
    (256, 256, 1280, 128, 256),        # the smallest 256-tile case
    (384, 384, 640, 128, 128),         # a 128-tile case
]


@pytest.mark.parametrize("M,N,K,conv_T,conv_C", TAKEN)
def test_products_that_take_the_copies(bf16_mode, M, N, K, conv_T, conv_C):
    L = bf16_mode
    a, plain, offered = conv_a_product(L, M, N, K, conv_T, conv_C)
    p0 = L.gemm_plan(a, **plain)
    assert p0["a_src"] == 1 and p0["b_src"] == 1 and p0["stage_bytes_a"] > 0 and p0["stage_bytes_b"] > 0
    p1 = L.gemm_plan(a, **offered)
    assert p1["a_src"] == 2 and p1["b_src"] == 2
    assert p1["stage_bytes_a"] == 0 and p1["stage_bytes_b"] == 0
    assert all(p1[k] == p0[k] for k in ROUTE), (p0, p1)
    h = L.conv_handoff_plan(a, **offered)
    assert h.pop("taken") is True and h == p1


def test_expected_kernels(bf16_mode):
    L = bf16_mode
    names = [L.gemm_plan(conv_a_product(L, *s)[0], **conv_a_product(L, *s)[1])["name"] for s in TAKEN]
    assert names == ["src256", "src256", "src256", "src256", "src128"], names


IGNORED = [
    ("N = 80", "bf16", (6400, 80, 2560, 100, 512)),
    ("conv_C = 80", "bf16", (6400, 512, 400, 100, 80)),
    ("M = 150", "bf16", (150, 256, 1280, 50, 256)),
    ("mode f32", "f32", (6400, 512, 2560, 100, 512)),
    ("mode bf16x3", "bf16x3", (6400, 512, 2560, 100, 512)),
    ("N = 128, nothing staged", "bf16", (3840, 128, 640, 60, 128)),
]


@pytest.mark.parametrize("what,mode,shape", IGNORED, ids=[w for w, _, _ in IGNORED])
def test_products_that_ignore_the_copies(what, mode, shape):
    from tacotron2_subword_amd import _lib as L
    L.set_precision(mode)
    try:
        a, plain, offered = conv_a_product(L, *shape)
        p0 = L.gemm_plan(a, **plain)
        h = L.conv_handoff_plan(a, **offered)
    finally:
        L.set_precision("f32")
    if what.startswith("N = 128"):
        assert p0["a_src"] == 0 and p0["b_src"] == 0          # the plan without copies stages nothing
    assert h.pop("taken") is False
    assert h == p0


def test_a_copy_that_would_move_the_product_is_refused(bf16_mode):
    """a16 lifts the N >= 256 condition of the staged routes: handed to t2_gemm_plan directly, the N = 128 product moves to
    a bf16-source kernel — which is exactly what the rule exists to prevent."""
    L = bf16_mode
    a, plain, offered = conv_a_product(L, 3840, 128, 640, 60, 128)
    assert L.gemm_plan(a, **plain)["name"] != L.gemm_plan(a, **offered)["name"]
    assert L.conv_handoff_plan(a, **offered)["taken"] is False


def test_only_the_offered_operand(bf16_mode):
    """A stack's first layer has no bf16 x: the weights alone are handed over, x is staged as before."""
    L = bf16_mode
    a, plain, offered = conv_a_product(L, 6400, 512, 2560, 100, 512)
    only_b = dict(plain, b16=1, ldb16=2560)
    p0, h = L.gemm_plan(a, **plain), L.conv_handoff_plan(a, **only_b)
    assert h["taken"] is True and h["a_src"] == 1 and h["b_src"] == 2 and h["stage_bytes_a"] == p0["stage_bytes_a"]
    assert all(h[k] == p0[k] for k in ROUTE)


def test_scratch_that_changes_the_split_refuses(bf16_mode):
    """Copies leave more scratch for split-K partials: with a scratch that holds the staged operands and not one partial
    more, the plan with copies would split where the plan without cannot, and the copies are ignored."""
    L = bf16_mode
    M, N, K = 6400, 512, 2560
    stage = 2 * (M * 512 + N * K)
    roomy = L.gemm_plan(conv_a_product(L, M, N, K, 100, 512)[0], conv_a=1, conv_T=100, conv_C=512)
    assert roomy["splitk"] > 1                                   # this shape splits when it can
    ws = stage + 2 * M * N * 4 - 256                             # staged operands + almost two partials
    a, plain, offered = conv_a_product(L, M, N, K, 100, 512, ws=ws)
    p0, p1 = L.gemm_plan(a, **plain), L.gemm_plan(a, **offered)
    assert (p0["splitk"], p1["splitk"]) == (1, 2)
    h = L.conv_handoff_plan(a, **offered)
    assert h.pop("taken") is False and h == p0
