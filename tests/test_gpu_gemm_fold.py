"""GPU: work folded into the GEMM stores (t2_set_gemm_fold) against the passes it replaces, and the embedding gradient.

The fold moves no arithmetic: the gate term of dDOUT is added where the mel product stores its element, as a rounded product
and a rounded sum (what the K = 1, beta = 1 product on top computed), and the conv weight gradient is written through a
column map instead of being copied into the reference layout afterwards.  So every comparison here is torch.equal, fold
on against fold off, in modes "bf16" and "f32".  The embedding gradient is checked against a CPU loop that adds the rows
in ascending order in fp32, which is the kernel's documented order, and the converting kernel's 16-byte stores against
the exact result of integer-valued products through each of its store routes."""
import pytest
import torch

from oracle import recipe

from helpers import SMA, hp_for, oracle_memories, tiny_hp, to_dev

pytestmark = pytest.mark.gpu

MODES = ["bf16", "f32"]


@pytest.fixture(scope="module")
def env():
    from tacotron2_subword_amd import _lib as L
    from tacotron2_subword_amd import blocks, ops
    yield L, blocks, ops
    L.set_gemm_fold(True)
    L.set_precision("f32")


def _both_folds(L, mode, run):
    """run() with the fold on, off and on again, in `mode`; the switch and the mode are restored whatever happens."""
    L.set_precision(mode)
    try:
        res = []
        for on in (True, False, True):
            L.set_gemm_fold(on)
            res.append(run())
            torch.cuda.synchronize()
        return res
    finally:
        L.set_gemm_fold(True)
        L.set_precision("f32")


# ---------------------------------------------------------------------------------------------- decoder backward
# (dims, B, T, Tin, Tsub): rows B*T that are no multiple of any tile.  The third case has 136 rows at the default dims,
# where the mel product leaves the 64-tile fp32 kernel in mode bf16 (converting kernel, M >= 64).
DECODER_CASES = [pytest.param("tiny", 2, 3, 5, 4, id="tiny-B2-T3"), pytest.param("tiny", 3, 17, 7, 5, id="tiny-B3-T17"),
                 pytest.param("default", 3, 17, 7, 5, id="default-B3-T17"), pytest.param("default", 8, 17, 7, 5, id="default-B8-T17")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims_name,B,T,Tin,Tsub", DECODER_CASES)
def test_decoder_backward_gate_term_in_the_store(env, mode, dims_name, B, T, Tin, Tsub):
    L, blocks, ops = env
    hp = tiny_hp(SMA) if dims_name == "tiny" else hp_for(SMA)
    P = recipe.make_weights(hp, seed=5)
    x, y = recipe.parse_batch(recipe.make_batch(hp, B, Tin, Tsub, T, seed=B))
    mem, mem_sub = oracle_memories(P, hp, x)
    dims = L.dims_from_hparams(hp)
    Pd = to_dev(P)
    W = L.decoder_weights(Pd, dims.attention_kind)
    memd, memsd = mem.cuda().contiguous(), mem_sub.cuda().contiguous()
    # Gradients as the loss produces them: d_gate = (sigmoid(logit) - target) / (B*T) from the BCE, d_mel = 2 * diff / (B*T*M)
    # from the MSE, and frames past an item's length exactly zero in both (the model masks them).  The products d_gate * w
    # are then far above 1e-38: a subnormal product is outside the contract (the matrix cores and the vector unit need not
    # treat it alike), so none is made here.
    g = torch.Generator().manual_seed(100 * B + T)
    M = hp["n_mel_channels"]
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    live = (torch.arange(T)[None, :] < lens[:, None]).float()                                 # [B,T]
    target = (torch.arange(T)[None, :] >= (lens[:, None] - 1)).float()
    d_gate = ((torch.sigmoid(torch.randn(B, T, generator=g)) - target) / (B * T)) * live
    d_mel = (2.0 * torch.randn(B, T, M, generator=g) / (B * T * M)) * live[:, :, None]
    d_gate[B - 1, T - 1] = 0.0                                                             # at least one frame exactly zero
    d_mel[B - 1, T - 1] = 0.0
    d_gate, d_mel = d_gate.cuda().contiguous(), d_mel.cuda().contiguous()

    def run():
        dp = ops.decoder_forward(W, dims, memd, memsd, x[1].cuda(), x[2].cuda(), x[3].cuda().contiguous(),
                                 training=True, prenet_dropout=True, seed=7)
        G, dmem, dmems = ops.decoder_backward(W, Pd, dims, dp, memd, memsd, d_mel, d_gate, training=True, prenet_dropout=True, seed=7)
        torch.cuda.synchronize()
        out = {k: v.clone() for k, v in G.items()}
        out["d_memory"], out["d_memory_sub"] = dmem.clone(), dmems.clone()
        return out

    on, off, on2 = _both_folds(L, mode, run)
    assert any(float(v.abs().max()) > 0 for v in on.values())
    for k in off:
        assert bool(torch.isfinite(off[k]).all()), k
        assert torch.equal(on[k], off[k]), (k, float((on[k] - off[k]).abs().max()))
        assert torch.equal(on2[k], off[k]), k


# ---------------------------------------------------------------------------------------------- conv backward
# (Cout, Cin, K, B, T) -> what the d(weight) product [Cout] x [K*Cin] over B*T frames runs as in mode bf16 / f32 (plan name,
# split-K > 1).  The first three are one per kernel family the store can come from; at their frame counts no plan splits
# K, so the two longer ones add the split-K reduce behind the converting and the k-major 256-tile kernel (f32: the 128-tile
# exact kernel and its reduce).
CONV_CASES = [
    pytest.param(8, 8, 5, 2, 9, ("f32_64", False), ("f32_64", False), id="8-8-2x9"),
    pytest.param(128, 64, 5, 4, 160, ("bf16conv", False), ("f32_64", False), id="128-64-4x160"),
    pytest.param(256, 256, 5, 8, 64, ("src256km", False), ("f32_64", False), id="256-256-8x64"),
    pytest.param(128, 64, 5, 8, 160, ("bf16conv", True), ("f32_128", True), id="128-64-8x160-splitk"),
    pytest.param(256, 256, 5, 8, 256, ("src256km", True), ("f32_128", True), id="256-256-8x256-splitk"),
]


def _dw_plan(L, Cout, Cin, K, B, T, ws_bytes):
    """The plan of the d(weight) product as conv_bn_bwd describes it (host query, nothing is launched)."""
    a = L.GemmArgs()
    a.A, a.B, a.C, a.M, a.N, a.K = 0x10000000, 0x20000000, 0x30000000, Cout, K * Cin, B * T
    a.sam, a.sak, a.sbn, a.sbk, a.ldc, a.batch, a.alpha, a.beta = 1, Cout, 1, 0, K * Cin, 1, 1.0, 0.0
    a.ws, a.ws_bytes = 0x40000000, ws_bytes
    return L.gemm_plan(a, conv_b=1, conv_T=T, conv_C=Cin)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Cout,Cin,K,B,T,plan_bf16,plan_f32", CONV_CASES)
def test_conv_backward_weight_gradient_in_its_layout(env, mode, Cout, Cin, K, B, T, plan_bf16, plan_f32):
    L, blocks, ops = env
    torch.manual_seed(Cout + B * T)
    conv = torch.nn.Conv1d(Cin, Cout, K, padding=(K - 1) // 2).cuda()
    bn = torch.nn.BatchNorm1d(Cout).cuda()
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.3 * torch.randn(Cout)); bn.bias.copy_(0.2 * torch.randn(Cout))
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + T)
    x0 = torch.randn(B, T, Cin, device="cuda", generator=g)
    R = torch.randn(B, T, Cout, device="cuda", generator=g)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()

    def run():
        bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
        for p in (conv.weight, conv.bias, bn.weight, bn.bias):
            p.grad = None
        xd = x0.clone().requires_grad_(True)
        L.gemm_counts(reset=True)
        yv = blocks.conv_bn_stack(xd, [(conv, bn)], [blocks.ACT_TANH], training=True, drop_p=0.5, seed=11, site0=L.SITE["ENC0"])
        (yv * R).sum().backward()
        torch.cuda.synchronize()
        return dict(dw=conv.weight.grad.clone(), dx=xd.grad.clone(), dgamma=bn.weight.grad.clone(), dbeta=bn.bias.grad.clone(),
                    dbias=conv.bias.grad.clone(), counts=list(L.gemm_counts()))

    on, off, on2 = _both_folds(L, mode, run)
    # the kernel family the store came from: the plan of the product, and the counters of the calls that ran
    L.set_precision(mode)
    try:
        plan = _dw_plan(L, Cout, Cin, K, B, T, 32 << 20)
    finally:
        L.set_precision("f32")
    name, split = plan_bf16 if mode == "bf16" else plan_f32
    assert plan["name"] == name and (plan["splitk"] > 1) == split, plan
    fam = {"f32_64": 0, "f32_128": 0, "bf16conv": 1, "src256km": 2}[name]
    assert on["counts"][fam] > 0 and on["counts"] == off["counts"], (on["counts"], off["counts"])
    if mode == "f32":
        assert on["counts"][1:] == [0, 0, 0], on["counts"]
    assert float(off["dw"].abs().max()) > 0
    for k in ("dw", "dx", "dgamma", "dbeta", "dbias"):
        assert bool(torch.isfinite(off[k]).all()), k
        assert torch.equal(on[k], off[k]), (k, float((on[k] - off[k]).abs().max()))
        assert torch.equal(on2[k], off[k]), k


# ---------------------------------------------------------------------------------------------- embedding backward
def _embedding_bwd_ref(ids, dout, vocab):
    """dtable[v] = the rows with ids == v added one after the other in ascending row order, fp32, from zero."""
    out = torch.zeros(vocab, dout.shape[1], dtype=torch.float32)
    for r in range(ids.numel()):
        out[int(ids[r])] += dout[r]
    return out


_EMB_REFS = {}


@pytest.mark.parametrize("D", [4, 512])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 6400])
def test_embedding_backward_ascending_rows(env, rows, D):
    """Vocabulary of 12: entry 3 never occurs, entry 5 exists only in the last partial block of 256 rows (in every row of it
    where the block is the only one) and the rest are spread at random; a second table has one entry that takes every
    row.  6400 rows is the training batch (one pass of the scan), 255 / 256 / 257 its round boundary."""
    L, blocks, ops = env
    vocab = 12
    g = torch.Generator().manual_seed(rows * 7 + D)
    pool = torch.tensor([0, 1, 2, 4, 6, 7, 8, 9, 10, 11])
    ids = pool[torch.randint(0, len(pool), (rows,), generator=g)]
    last = (rows - 1) // 256 * 256
    ids[last + torch.randperm(rows - last, generator=g)[:max(1, (rows - last) // 3)]] = 5
    dout = torch.randn(rows, D, generator=g)
    every = torch.full((rows,), 7, dtype=torch.long)
    for name, idv in (("mixed", ids), ("one entry takes every row", every)):
        key = (name, rows, D)
        if key not in _EMB_REFS:
            _EMB_REFS[key] = _embedding_bwd_ref(idv, dout, vocab)
        ref = _EMB_REFS[key]
        dtable = torch.full((vocab, D), float("nan"), device="cuda")
        ids_d, dout_d = idv.cuda(), dout.cuda()
        L.check(L.lib().t2_embedding_backward(L.ptr(ids_d), L.ptr(dout_d), L.ptr(dtable), rows, D, vocab, L.stream()))
        torch.cuda.synchronize()
        got = dtable.cpu()
        assert bool((got[3] == 0).all()), name
        if name == "mixed":
            assert int((idv == 5).sum()) > 0 and int((idv[:last] == 5).sum()) == 0
        assert torch.equal(got, ref), (name, float((got - ref).abs().max()))


# ---------------------------------------------------------------------------------------------- converting kernel's stores
def _gemm_ex(L, A, B, out, M, N, K, nt, batch, *, bias=None, beta=0.0, ws=None, splitk=0):
    """t2_gemm_ex on A [batch][M][K], B [batch][N][K] (nt) or [batch][K][N], out [batch][M][N] (a view may start off a 16-byte boundary)."""
    import ctypes as C
    sbn, sbk = (K, 1) if nt else (1, N)
    a = L.GemmArgs(A.data_ptr(), B.data_ptr(), out.data_ptr(), M, N, K, K, 1, sbn, sbk, N, batch, M * K, N * K, M * N, 1.0, beta,
                   L.ptr(bias), 0, 0, 0, L.ptr(ws), 0 if ws is None else ws.numel() * 4, splitk)
    L.check(L.lib().t2_gemm_ex(C.byref(a), L.stream()))
    plan = L.gemm_plan(a)
    return plan["name"], plan["splitk"]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "C-4-bytes-off"])
@pytest.mark.parametrize("nt", [True, False], ids=["NT", "NN"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("M,N,K", [(129, 80, 80), (256, 2048, 80)])
def test_converting_kernel_stores_through_lds(env, M, N, K, batch, nt, off):
    """The converting kernel (mode bf16, no whole tiles to stage) lays its tile out in LDS and stores 16 bytes per lane.  The
    same product is run three ways: stored by the kernel itself (no scratch), through split-K partials and the reduce (a
    scratch and a forced factor of 2: K = 80 is one 64-wide chunk per split), and with beta = 1 onto a C that holds values.
    Operands, bias and C are small integers, so every product and every sum in any order is exact in fp32: the three
    must equal the fp64 result bit for bit, whatever the order of the additions.  M = 129 and N = 80 leave the last row tile
    with one row and put the tile edge inside a 16-byte group's neighbourhood; C four bytes off takes the scalar stores."""
    L, blocks, ops = env
    g = torch.Generator().manual_seed(M + N + batch)
    A = torch.randint(-3, 4, (batch, M, K), generator=g).float().cuda()
    B = torch.randint(-3, 4, (batch, N, K) if nt else (batch, K, N), generator=g).float().cuda()
    bias = torch.randint(-5, 6, (N,), generator=g).float().cuda()
    C0 = torch.randint(-9, 10, (batch, M, N), generator=g).float().cuda()
    ref = (A.double() @ (B.double().transpose(1, 2) if nt else B.double())) + bias.double()
    ws = torch.empty(2 * batch * M * N + 64, device="cuda")
    guard = 7.0

    def fresh(fill=None):
        flat = torch.full((off + batch * M * N + 8,), guard, device="cuda")
        out = flat[off:off + batch * M * N].view(batch, M, N)
        if fill is not None:
            out.copy_(fill)
        return flat, out

    L.set_precision("bf16")
    try:
        L.gemm_counts(reset=True)
        f1, direct = fresh()
        p1 = _gemm_ex(L, A, B, direct, M, N, K, nt, batch, bias=bias)
        f2, split = fresh()
        p2 = _gemm_ex(L, A, B, split, M, N, K, nt, batch, bias=bias, ws=ws, splitk=2)
        f3, accum = fresh(C0)
        p3 = _gemm_ex(L, A, B, accum, M, N, K, nt, batch, bias=bias, beta=1.0)
        torch.cuda.synchronize()
        counts = L.gemm_counts()
    finally:
        L.set_precision("f32")
    assert p1 == ("bf16conv", 1) and p2 == ("bf16conv", 2) and p3 == ("bf16conv", 1), (p1, p2, p3)
    assert counts[1] == 3, counts
    assert torch.equal(direct.double(), ref)
    assert torch.equal(split.double(), ref)
    assert torch.equal(accum.double(), ref + C0.double())
    for flat in (f1, f2, f3):                                     # nothing written outside the result
        assert bool((flat[:off] == guard).all()) and bool((flat[off + batch * M * N:] == guard).all())
