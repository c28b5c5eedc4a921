"""GPU, bf16 mode: blocks.conv_bn_stack with the bf16 hand-offs on and off (blocks.CONV_HANDOFF) gives the same bits.

With the switch on, a layer writes its output also as bf16 for the next layer's GEMM, dz is written once as bf16 for both
backward products, and the re-laid-out weights go straight to bf16; with it off every operand is cast by the GEMM layer.
The copies hold the same roundings and the products keep their kernel and split-K (tests/test_conv_handoff_plan_cpu.py),
so every result must be torch.equal: y, d(input), the gradients of every weight, bias, gamma and beta, the running
statistics."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 5


@pytest.fixture(scope="module")
def env():
    from tacotron2_subword_amd import _lib as L, blocks
    return L, blocks


def _run(L, blocks, handoff, convs, bns, x0, R, acts, training, residual):
    dconvs, dbns = [copy.deepcopy(c) for c in convs], [copy.deepcopy(b) for b in bns]
    xd = x0.clone().requires_grad_(True)
    old = blocks.CONV_HANDOFF
    blocks.CONV_HANDOFF = handoff
    L.set_precision("bf16")
    try:
        L.gemm_counts(reset=True)
        y = blocks.conv_bn_stack(xd, list(zip(dconvs, dbns)), acts, training=training, drop_p=0.5, seed=7, site0=L.SITE["POSTNET0"],
                                 residual=residual)
        (y * R).sum().backward()
        torch.cuda.synchronize()
        counts = L.gemm_counts()
    finally:
        L.set_precision("f32")
        blocks.CONV_HANDOFF = old
    out = dict(y=y.detach(), dx=xd.grad)
    for i, (c, b) in enumerate(zip(dconvs, dbns)):
        out.update({f"dw{i}": c.weight.grad, f"dbias{i}": c.bias.grad, f"dgamma{i}": b.weight.grad, f"dbeta{i}": b.bias.grad,
                    f"run_mean{i}": b.running_mean, f"run_var{i}": b.running_var})
    return out, counts


CASES = [
    # B, T, channels, acts, residual, bf16-source products expected (forward + d(weight) + d(input) per qualifying layer)
    (2, 128, [256, 256, 256, 256], [2, 2, 0], False, 9),      # src256, src256km + conv_b, the conv_a d(input) product
    (2, 128, [80, 256, 256, 80], [2, 2, 0], True, 3),         # first / last layer on the converting kernel next to a bf16 consumer
    (3, 128, [128, 128, 128], [2, 0], False, 0),              # 128-tile shapes below the staging threshold (N = 128): all ignored
    (3, 128, [384, 384, 384], [2, 0], False, 4),              # the 128-tile bf16-source route: forward and d(input) take the copies,
                                                              # d(weight) runs on fp32 operands next to the live dz copy
    (3, 50, [256, 256], [2], False, 0),                       # M = 150: nothing qualifies, the copies must be ignored
]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,T,chans,acts,residual,n_src", CASES)
def test_handoff_is_bit_identical(env, B, T, chans, acts, residual, n_src, training):
    L, blocks = env
    g = torch.Generator().manual_seed(B * 100 + T + chans[0])
    n = len(acts)
    convs = [torch.nn.Conv1d(chans[i], chans[i + 1], K, padding=K // 2).cuda() for i in range(n)]
    bns = [torch.nn.BatchNorm1d(chans[i + 1]).cuda() for i in range(n)]
    with torch.no_grad():
        for c, b in zip(convs, bns):
            c.weight.copy_(torch.randn(c.weight.shape, generator=g) * 0.05)
            b.weight.copy_(torch.empty(b.weight.shape).uniform_(0.5, 1.5, generator=g))
            b.bias.copy_(torch.empty(b.bias.shape).uniform_(-0.2, 0.2, generator=g))
            b.running_mean.copy_(torch.randn(b.running_mean.shape, generator=g) * 0.1)
            b.running_var.copy_(torch.empty(b.running_var.shape).uniform_(0.5, 1.5, generator=g))
    x0 = torch.randn(B, T, chans[0], generator=g).cuda()
    R = torch.randn(B, T, chans[-1], generator=g).cuda()
    off, c_off = _run(L, blocks, False, convs, bns, x0, R, acts, training, residual)
    on, c_on = _run(L, blocks, True, convs, bns, x0, R, acts, training, residual)
    assert c_on == c_off, (c_on, c_off)                       # the same kernel families either way
    assert c_on[2] == n_src, c_on                             # and the routes this case is here for
    for k in off:
        assert torch.equal(on[k], off[k]), (k, float((on[k] - off[k]).abs().max()))
