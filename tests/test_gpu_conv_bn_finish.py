"""GPU: a Conv1d + BatchNorm layer with its column reductions finished in the consuming kernel's prologue (t2_set_bn_fuse,
the default: the mean in the pass over the centred squares, d(beta) / d(gamma) and the d(bias) partials in the dz kernel, var /
invstd and the running statistics in one stage 2) against the same layer with a stage-2 launch per reduction (the switch off).

The fused layer changes who finishes a sum and how the rows are spread over the device, never the order of a column's
additions (csrc/common.h), so every array a forward and a backward call write must be torch.equal: z, mean, invstd, var, the
running statistics, y and its bf16 copy, dz (the head of the backward workspace), d(beta), d(gamma), d(bias), dw, dx.  In mode
"f32", and in mode "bf16" with the bf16 hand-offs requested.  Shapes: the smallest that reach every branch (one slab, a few
slabs, all 64 with a ragged last slab and ragged phases; one column per lane with a column block partly outside C, 16-byte
groups with a partly filled second block; at all 64 slabs the forward keeps 16-byte groups and the fused backward takes one
column per lane up to 512 columns and 8-byte groups for 1024; a layer whose re-laid-out weights have no room for the
d(bias) partials).
Further: a workspace full of NaN from an earlier call changes nothing, and two layers on two streams give what each gives
alone."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
NONE, RELU, TANH = 0, 1, 2
FWD = ("z", "mean", "invstd", "var", "run_mean", "run_var", "y", "y16")
BWD = ("dz", "dbeta", "dgamma", "dbias", "dw", "dx")
# training, act, drop_p, residual
CONFIGS = [(1, NONE, 0.0, False), (1, RELU, 0.5, True), (1, TANH, 0.5, False), (1, TANH, 0.0, True), (0, RELU, 0.0, True),
           (0, TANH, 0.0, False)]


@pytest.fixture(scope="module")
def L():
    from tacotron2_subword_amd import _lib
    assert _lib.get_bn_fuse(), "the fused layer is the default"
    yield _lib
    _lib.set_bn_fuse(True)
    _lib.set_precision("f32")


def _inputs(shape, residual, seed):
    B, T, Cin, Cout, K = shape
    g = torch.Generator().manual_seed(seed * 7919 + B * T * 31 + Cout)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = dict(x=rn(B, T, Cin), w=rn(Cout, Cin, K) * 0.2, bias=rn(Cout), gamma=1.0 + 0.3 * rn(Cout), beta=rn(Cout),
             rm=torch.rand(Cout, generator=g) * 0.2 - 0.1, rv=0.5 + torch.rand(Cout, generator=g), dy=rn(B, T, Cout),
             res=rn(B, T, Cout) if residual else None)
    return {k: (v.cuda() if v is not None else None) for k, v in d.items()}


def _workspaces(shape):
    B, T, Cin, Cout, K = shape
    M = B * T
    extra = (1 << 20) + M * K * max(Cin, Cout)
    return (torch.empty(Cout * Cin * K + 4 + 128 * Cout + extra, device="cuda"),
            torch.empty(M * Cout + 2 * Cout * Cin * K + 128 * Cout + 16 + extra, device="cuda"))


def _layer(L, shape, inp, cfg, handoff, ws=None, poison=False):
    """One forward and one backward call on the current stream; everything they write."""
    B, T, Cin, Cout, K = shape
    training, act, drop_p, _ = cfg
    M = B * T
    ws1, ws2 = ws if ws is not None else _workspaces(shape)
    if poison:
        ws1.fill_(float("nan"))
        ws2.fill_(float("nan"))
    rm, rv = inp["rm"].clone(), inp["rv"].clone()
    st = torch.zeros(3, Cout, device="cuda")
    z, y = torch.empty(M, Cout, device="cuda"), torch.empty(B, T, Cout, device="cuda")
    y16 = torch.zeros(B, T, Cout, dtype=torch.bfloat16, device="cuda")
    x16 = inp["x"].bfloat16() if handoff else None
    a = L.ConvBnArgs(B, T, Cin, Cout, K, L.ptr(inp["x"]), L.ptr(inp["w"]), L.ptr(inp["bias"]), L.ptr(inp["gamma"]), L.ptr(inp["beta"]),
                     L.ptr(rm), L.ptr(rv), training, EPS, act, drop_p, 99, L.SITE["POSTNET0"], L.ptr(inp["res"]), L.ptr(z), L.ptr(st[0]),
                     L.ptr(st[1]), L.ptr(st[2]), L.ptr(y), L.ptr(ws1), ws1.numel(), L.ptr(x16), L.ptr(y16), int(handoff))
    L.check(L.lib().t2_conv_bn_forward(C.byref(a), L.stream()))
    dw, dbias = torch.empty_like(inp["w"]), torch.empty(Cout, device="cuda")
    dgamma, dbeta = torch.empty(Cout, device="cuda"), torch.empty(Cout, device="cuda")
    dx = torch.empty(B, T, Cin, device="cuda") if Cout % 4 == 0 else None
    b = L.ConvBnBwdArgs(B, T, Cin, Cout, K, L.ptr(inp["x"]), L.ptr(inp["w"]), L.ptr(inp["gamma"]), L.ptr(inp["beta"]), L.ptr(z), L.ptr(st[0]),
                        L.ptr(st[1]), training, EPS, act, drop_p, 99, L.SITE["POSTNET0"], L.ptr(inp["dy"]), L.ptr(dw), L.ptr(dbias),
                        L.ptr(dgamma), L.ptr(dbeta), L.ptr(dx), 0, L.ptr(ws2), ws2.numel(), L.ptr(x16), int(handoff))
    L.check(L.lib().t2_conv_bn_backward(C.byref(b), L.stream()))
    out = dict(z=z, mean=st[0], invstd=st[1], var=st[2], run_mean=rm, run_var=rv, y=y, y16=y16, dz=ws2[:M * Cout].clone(), dbeta=dbeta,
               dgamma=dgamma, dbias=dbias, dw=dw)
    if dx is not None:
        out["dx"] = dx
    return out, (ws1, ws2, x16)                                       # the buffers stay alive until the caller has synchronised


def _same(tag, got, want):
    for k in want:
        assert not torch.isnan(want[k]).any(), f"{tag} {k}: NaN in the reference"
        if not torch.equal(got[k], want[k]):
            g, w = got[k].flatten().float(), want[k].flatten().float()
            i = int((~(g == w)).nonzero()[0])
            raise AssertionError(f"{tag} {k}: first difference at flat index {i} of shape {tuple(want[k].shape)}: {float(g[i])!r} != {float(w[i])!r}")


SHAPES = [
    # B, T, Cin, Cout, K                 M, slabs; lanes
    (1, 5, 16, 80, 5),                 # 5, one slab, phases with one or two rows; 16-byte groups
    (3, 64, 16, 132, 5),               # 192, 3 slabs; 16-byte groups, the second column block holds 4 columns
    (3, 64, 16, 70, 5),                # 192, 3 slabs; one column per lane, the third block holds 6
    (4, 65, 16, 6, 5),                 # 260, 4 slabs of 65 rows; one column per lane, one block of 6
    (1, 4099, 16, 70, 5),              # 4099, 64 slabs of 65 rows, the last with 4; one column per lane
    (1, 4099, 16, 132, 5),             # the same rows with 16-byte groups forward (2 blocks), one column per lane backward (5 blocks)
    (4, 1024, 64, 512, 3),             # 4096 x 512: 64 slabs x 4 blocks forward, x 16 blocks backward; whole GEMM tiles for the hand-offs
    (2, 2048, 16, 1024, 5),            # 4096 x 1024: 64 slabs x 8 blocks forward, x 16 blocks of 8-byte groups backward
]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_equals_unfused(L, shape, mode):
    handoff = mode == "bf16"
    L.set_precision(mode)
    try:
        for n, cfg in enumerate(CONFIGS):
            inp = _inputs(shape, cfg[3], n + 1)
            L.set_bn_fuse(False)
            L.bn_fuse_counts(reset=True)
            off, keep0 = _layer(L, shape, inp, cfg, handoff)
            assert L.bn_fuse_counts() == (0, 0, 0)
            L.set_bn_fuse(True)
            on, keep1 = _layer(L, shape, inp, cfg, handoff)
            torch.cuda.synchronize()
            assert L.bn_fuse_counts(reset=True) == (cfg[0], 1, 0), "training forward and the backward fused, d(bias) from the dz kernel"
            assert set(on) == set(off) and set(off) >= set(FWD + BWD) - ({"dx"} if shape[3] % 4 else set())
            _same(f"{mode} {shape} training={cfg[0]} act={cfg[1]} p={cfg[2]} residual={cfg[3]}:", on, off)
    finally:
        L.set_bn_fuse(True)
        L.set_precision("f32")


# Cin * K < 64: the re-laid-out weights hold fewer than 64 * Cout floats, so d(bias) comes from the separate column sum
@pytest.mark.parametrize("shape", [(3, 64, 4, 80, 1), (1, 4099, 16, 132, 3), (4, 65, 4, 6, 5)], ids=lambda s: "x".join(map(str, s)))
def test_dbias_fallback_without_room(L, shape):
    assert shape[2] * shape[4] < 64
    for n, cfg in enumerate(CONFIGS[1:4]):
        inp = _inputs(shape, cfg[3], n + 11)
        L.set_bn_fuse(False)
        off, keep0 = _layer(L, shape, inp, cfg, False)
        L.set_bn_fuse(True)
        L.bn_fuse_counts(reset=True)
        on, keep1 = _layer(L, shape, inp, cfg, False)
        torch.cuda.synchronize()
        assert L.bn_fuse_counts(reset=True) == (1, 0, 1), "the fused backward took the separate column sum"
        _same(f"fallback {shape} act={cfg[1]}:", on, off)


@pytest.mark.parametrize("shape", [(3, 64, 16, 132, 5), (1, 4099, 16, 70, 5), (4, 1024, 64, 512, 3)], ids=lambda s: "x".join(map(str, s)))
def test_stale_workspace(L, shape):
    """The same layer twice on one workspace, filled with NaN before each call, with different inputs: as on a fresh one."""
    cfg = CONFIGS[1]
    ws = _workspaces(shape)
    for n in range(2):
        inp = _inputs(shape, cfg[3], n + 21)
        fresh, keep0 = _layer(L, shape, inp, cfg, False, poison=True)
        reused, keep1 = _layer(L, shape, inp, cfg, False, ws=ws, poison=True)
        torch.cuda.synchronize()
        _same(f"stale workspace, call {n}, {shape}:", reused, fresh)


def test_two_streams(L):
    """Two layers at once on two streams with workspaces of their own, as the two encoder stacks run."""
    shapes = [(4, 1024, 64, 512, 3), (1, 4099, 16, 132, 5)]
    cfgs = [CONFIGS[1], CONFIGS[2]]
    inps = [_inputs(s, c[3], 31 + i) for i, (s, c) in enumerate(zip(shapes, cfgs))]
    alone = [_layer(L, s, i, c, False)[0] for s, i, c in zip(shapes, inps, cfgs)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    both, keep = [], []
    for rep in range(3):                                               # a few rounds, so the two really overlap
        for st, s, i, c in zip(streams, shapes, inps, cfgs):
            with torch.cuda.stream(st):
                out, k = _layer(L, s, i, c, False)
            both.append(out)
            keep.append(k)
    torch.cuda.synchronize()
    for n, out in enumerate(both):
        _same(f"two streams, round {n // 2}, layer {n % 2}:", out, alone[n % 2])
