"""The 256 x 256 GEMM's k-major operand variant (A[k][m], B[k][n] read as they lie in memory through transposed LDS
reads; implicit-conv B operand without an im2col copy): against fp64 on the bf16-rounded operands, bit-for-bit against
the K-contiguous variant on the same matrices, and a check that the variant is the one that runs."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd import blocks, ops
    return L, blocks, ops


def _tol(K):
    return 2e-3 * max(1.0, K ** 0.5 / 8)                     # the bound of tests/test_gpu_kernels.py


# (M, N, K, splitk, beta): K-tile counts 2 (minimal), 5 / 17 / 65 (odd: one padding tile), 64 (even); split-K chosen by
# the dispatch (tiles < 512 and a long K) and given explicitly; M = N = 256 exactly; an accumulate into C (no split);
# two weight-gradient shapes of the training iteration (attention-LSTM W_hh, a postnet conv's d(weight) as a plain product)
SHAPES = [(256, 256, 128, 0, 0.0), (512, 256, 320, 0, 0.0), (256, 512, 4096, 0, 0.0), (768, 256, 4160, 0, 0.0),
          (512, 768, 1088, 3, 0.0), (256, 256, 704, 0, 1.0), (4096, 1024, 25536, 0, 0.0), (512, 2560, 6400, 0, 0.0)]


@pytest.mark.parametrize("M,N,K,splitk,beta", SHAPES)
def test_gemm_kmajor_vs_fp64_and_kcontiguous(env, M, N, K, splitk, beta):
    """A[k][m] B[k][n] through ops.gemm (t2_gemm), bf16 mode, scratch given.  The k-major variant keeps every k of a
    16-wide MFMA step in the lane slot the K-contiguous fragment read puts it in, so besides the fp64 bound it must
    equal, bit for bit, the K-contiguous variant run on transposed copies of the same matrices."""
    L, blocks, ops = env
    g = torch.Generator(device="cuda").manual_seed(M + 3 * N + 7 * K)
    A = torch.randn(K, M, device="cuda", generator=g)
    B = torch.randn(K, N, device="cuda", generator=g)
    C0 = torch.randn(M, N, device="cuda", generator=g)
    ws = torch.empty(16 * M * N + (M + N) * K, device="cuda")
    At, Bt = A.t().contiguous(), B.t().contiguous()          # the same matrices, K contiguous
    L.set_precision("bf16")
    try:
        out = C0.clone()
        ops.gemm(A, B, trans_a=True, trans_b=False, ws=ws, splitk=splitk, beta=beta, out=out)
        out_kc = C0.clone()
        ops.gemm(At, Bt, trans_a=False, trans_b=True, ws=ws, splitk=splitk, beta=beta, out=out_kc)
        torch.cuda.synchronize()
    finally:
        L.set_precision("f32")
    ref = A.bfloat16().double().t() @ B.bfloat16().double() + beta * C0.double()      # fp64 on the GPU
    err = float((out.double() - ref).abs().max())
    err_kc = float((out_kc.double() - ref).abs().max())
    print(f"k-major M={M} N={N} K={K} splitk={splitk} beta={beta}: max-abs error vs fp64 {err:.3e} (K-contiguous {err_kc:.3e}), "
          f"bound {_tol(K):.3e}, max |k-major - K-contiguous| {float((out - out_kc).abs().max()):.3e}")
    assert err < _tol(K), err
    assert torch.equal(out, out_kc)


def _conv_dw(L, blocks, x0, R, Cout):
    """d(weight) of one k = 5 conv layer through t2_conv_bn_backward (eval-mode BatchNorm with unit statistics: dz = dy)."""
    Cin = x0.shape[-1]
    torch.manual_seed(3)
    conv = torch.nn.Conv1d(Cin, Cout, 5, padding=2).cuda()
    bn = torch.nn.BatchNorm1d(Cout).cuda().eval()
    bn.running_mean.zero_(); bn.running_var.fill_(1.0 - bn.eps)
    L.set_precision("bf16")
    try:
        xd = x0.clone().requires_grad_(True)
        y = blocks.conv_bn_stack(xd, [(conv, bn)], [blocks.ACT_NONE], training=False, drop_p=0.0, seed=1, site0=L.SITE["ENC0"])
        (y * R).sum().backward()
        torch.cuda.synchronize()
    finally:
        L.set_precision("f32")
    scale = (bn.weight.detach() * (1.0 / torch.sqrt(bn.running_var + bn.eps)))[None, None, :]
    return conv.weight.grad.detach(), (R * scale).detach()


@pytest.mark.parametrize("B,T", [(4, 400), (64, 77)])
def test_conv_weight_gradient_implicit_kmajor(env, B, T):
    """d(weight) of a C = 512, k = 5 conv (the postnet's layers): the B operand is the k-major frame matrix with its rows
    shifted per tap, no im2col copy.  Reference: the same product in fp64 with the im2col matrix built in torch from the
    bf16-rounded activations.  T is not a multiple of 64, so utterance boundaries fall inside K-tiles; B * T is a whole
    (odd) number of K-tiles."""
    L, blocks, ops = env
    C = 512
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + T)
    x0 = torch.randn(B, T, C, device="cuda", generator=g)
    R = torch.randn(B, T, C, device="cuda", generator=g)
    dw, dz = _conv_dw(L, blocks, x0, R, C)                   # dw[co][ci][dk]
    xb = x0.bfloat16().double()
    cols = torch.zeros(B, T, 5, C, dtype=torch.float64, device="cuda")       # im2col: V[m, dk, ci] = X[m + dk - 2, ci] inside the utterance
    for dk in range(5):
        s = dk - 2
        lo, hi = max(0, -s), min(T, T - s)
        cols[:, lo:hi, dk] = xb[:, lo + s:hi + s]
    ref = dz.bfloat16().double().reshape(B * T, C).t() @ cols.reshape(B * T, 5 * C)       # [co][dk*C + ci]
    ref = ref.reshape(C, 5, C).permute(0, 2, 1)
    err = (dw.double() - ref).abs()
    print(f"conv d(weight) B={B} T={T}: max-abs error vs fp64 {float(err.max()):.3e}, per tap "
          f"{[round(float(err[:, :, k].max()), 6) for k in range(5)]}, bound {_tol(B * T):.3e}")
    assert float(err.max()) < _tol(B * T), float(err.max())


@pytest.mark.parametrize("side", ["before", "after"])
def test_conv_weight_gradient_taps_past_the_utterance_are_zero(env, side):
    """dz is non-zero only in the first (last) frame of utterance 1 and the input only in the neighbouring utterance's
    edge frames next to it: every tap that pairs them reaches past the utterance, so d(weight) is exactly zero."""
    L, blocks, ops = env
    B, T, C = 4, 400, 512
    g = torch.Generator(device="cuda").manual_seed(17)
    x0 = torch.zeros(B, T, C, device="cuda"); R = torch.zeros(B, T, C, device="cuda")
    if side == "before":
        R[1, 0] = torch.randn(C, device="cuda", generator=g); x0[0, T - 2:] = torch.randn(2, C, device="cuda", generator=g)
    else:
        R[1, T - 1] = torch.randn(C, device="cuda", generator=g); x0[2, :2] = torch.randn(2, C, device="cuda", generator=g)
    dw, _ = _conv_dw(L, blocks, x0, R, C)
    assert float(dw.abs().max()) == 0.0
    # the same frames inside ONE utterance do pair (the check above is not vacuous)
    x1 = torch.zeros_like(x0)
    if side == "before":
        x1[1, 1:3] = x0[0, T - 2:]
    else:
        x1[1, T - 3:T - 1] = x0[2, :2]
    dw1, _ = _conv_dw(L, blocks, x1, R, C)
    assert float(dw1.abs().max()) > 0.0


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
from tacotron2_subword_amd import _lib as L, blocks, ops
L.set_precision("bf16")
for M, N, K in [(256, 256, 128), (768, 256, 4160), (4096, 1024, 25536), (512, 2560, 6400)]:
    A = torch.randn(K, M, device="cuda"); B = torch.randn(K, N, device="cuda")
    ws = torch.empty(16 * M * N + (M + N) * K, device="cuda")
    ops.gemm(A, B, trans_a=True, trans_b=False, ws=ws)
conv = torch.nn.Conv1d(512, 512, 5, padding=2).cuda(); bn = torch.nn.BatchNorm1d(512).cuda().eval()
x = torch.randn(4, 400, 512, device="cuda", requires_grad=True)
blocks.conv_bn_stack(x, [(conv, bn)], [blocks.ACT_NONE], training=False, drop_p=0.0, seed=1, site0=L.SITE["ENC0"]).sum().backward()
torch.cuda.synchronize()
"""


def test_kmajor_variant_is_taken():
    """T2_GEMM_LOG=1 (read once per process, hence the child): every A[k][m] B[k][n] product of whole 256-tiles and the
    conv weight gradient run the k-major variant, with the operands staged by the plain cast."""
    env = dict(os.environ, T2_GEMM_LOG="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stderr.splitlines() if l.startswith("t2gemm") and "A[k][m] B[k][n]" in l]
    plain = [l for l in lines if "convB=0" in l]
    conv = [l for l in lines if "convB=1" in l]
    assert len(plain) == 4 and len(conv) == 1, lines
    for l in plain + conv:
        assert "kernel=src256km " in l, l
    assert "M=512 N=2560 K=1600" in conv[0], conv[0]
