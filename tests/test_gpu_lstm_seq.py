"""GPU tests of t2_lstm_seq_forward / t2_lstm_seq_backward (include/t2amd.h) through the C ABI, against fp64 truth from
tests/lstm_seq_ref.py: the per-step route (csrc/lstm.hip, every Exact forward and ExactKN backward instance) and the
persistent route (csrc/chain_enc.hip), at their stream, row-tile, stage-width and length edges.  Precision mode "f32".

Every output buffer is filled with NaN before the call and every element is compared, h, c, gates, dpre and dw_hh alike.
Bound of every check: F * max(dev_ref, 2^-23 * max|truth|) per compared tensor (lstm_seq_ref.bound; the CPU tests show
that it rejects five deliberate mistakes).  dev_ref: the fp32 statement against itself in fp64 on that case.

F was measured, not chosen: all cases were run on the unchanged kernels with the bounds opened, and per route and quantity
F is the smallest power of two that leaves at least 2 x over the worst err / max(dev_ref, floor) seen (the 2 x is for a
summation order that differs from torch's: eight waves' partial tiles summed through LDS, split-K in the dw_hh GEMM).
Worst shares seen (profiles/r32_lstm_seq_tests.txt), per-step route / persistent route, and the case that gave them:
    h      1.08 (chain_b33_t7, chain off)  / 1.05 (chain_b31_t2)    F = 4
    c      1.15 (h512_b31_t4)              / 1.21 (chain_b31_t2)    F = 4
    gates  0.89 (h64_b5_t2)                / 0.78 (chain_b31_t2)    F = 2
    dpre   1.42 (h512_b64_t3)              / 1.33 (chain_b128_t5)   F = 4
    dw_hh  3.29 (h256_b256_t3)             / 2.20 (chain_b33_t7)    F = 8
dw_hh is the one quantity above the 4 of tests/test_gpu_bert.py: it is a sum over (T-1) * B products of two computed
factors (dpre, which is itself 1.4 x dev_ref from fp64, and h), summed by the split-K GEMM in another order than
torch's, and the worst of 4H * H elements is compared with the worst of one other fp32 evaluation; the largest share
came with the longest sum per step pair (B = 256).  No case stood out: every share of every case lies within 3.3.
The two routes differ from each other by at most 1.37 x max(dev_ref, floor) (h, chain_b128_t5), gates by 0.67 x.

Instances reached (forward Exact<row tiles, stage> of csrc/lstm.hip: step 0 has no recurrent segment and takes the widest
stage of its row-tile count, later steps the instance of K = H; backward ExactKN of K = 4H / ksplit):
    Exact<1,256>   h256_b32_t6_4streams, h512_b31_t4 (and step 0 of every case of at most 32 rows)
    Exact<1,64>    h64_b5_t2
    Exact<2,256>   h512_b64_t3 (and step 0 of every case of 33..64 rows)
    Exact<2,64>    h64_b64_t9_padded, h192_b33_t5_3streams
    Exact<4,128>   h128_b97_t4, h256_b128_t3
    Exact<4,64>    h192_b128_t3_short
    Exact<8,64>    h256_b129_t3, h256_b256_t3
    ExactKN<1,256> h512_b31_t4          ExactKN<1,64>  h64_b5_t2, h256_b32_t6_4streams
    ExactKN<2,256> h512_b64_t3          ExactKN<2,64>  h64_b64_t9_padded, h192_b33_t5_3streams (ksplit 4)
    ExactKN<4,128> h256_b128_t3         ExactKN<4,64>  h128_b97_t4, h192_b128_t3_short
    ExactKN<8,64>  h256_b129_t3, h256_b256_t3
h64_b1_t1 runs step 0 only (Exact<1,256> with no stage) and no backward product: its dw_hh comes from the zero fill.
"""
import ctypes as C
import functools

import pytest
import torch

import lstm_seq_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 12345.0
WORST = {}


@functools.lru_cache(maxsize=None)
def env():
    from tacotron2_subword_amd import _lib, ops
    return _lib, ops


def need_claim():
    if not env()[0].lib().t2_chain_claimed():
        pytest.skip("another process holds this GPU's persistent-kernel claim")


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def bwd_ws_floats(ns, B, H):
    L, _ = env()
    return max(ns * 9 * B * H + 64, int(L.lib().t2_lstm_seq_chain_ws_floats(ns, B, H, 1))) + (8 << 20)


def plan(ns, B, H, backward):
    """What the library's plan says for the encoder chain of this shape on this device (t2_chain_plan: launches nothing)."""
    L, _ = env()
    ws = bwd_ws_floats(ns, B, H) if backward else int(L.lib().t2_lstm_seq_chain_ws_floats(ns, B, H, 0))
    return L.chain_plan("enc", backward, cus=torch.cuda.get_device_properties(0).multi_processor_count,
                        claimed=bool(L.lib().t2_chain_claimed()), NS=ns, B=B, H=H, ws_floats=ws)


def gpu_run(H, B, T, streams, lengths, *, chain, pad=0, backward=True, nan_pre=False):
    """One forward (and backward) call.  streams: [(pre, w_hh, reverse, dh)] on the CPU.  The streams share one h and one dh
    buffer [T,B,ns*H + pad] as the two directions of a BiLSTM do; the pad columns of h hold SENTINEL, those of dh NaN.
    nan_pre: pre is NaN at every position past its item's length.  Returns per stream {h, c, gates, dpre, dw_hh} on the
    CPU, and the pad columns of h."""
    L, ops = env()
    ns, ld = len(streams), len(streams) * H + pad
    pre = torch.stack([s[0] for s in streams]).to(DEV)
    if nan_pre:
        dead = torch.arange(T)[:, None] >= lengths[None, :]
        pre[:, dead.to(DEV)] = float("nan")
    w = torch.stack([s[1] for s in streams]).to(DEV)
    ln = None if lengths is None else lengths.to(device=DEV, dtype=torch.int32)
    hbuf = nan(T, B, ld)
    hbuf[:, :, ns * H:] = SENTINEL
    c, gates = nan(ns, T, B, H), nan(ns, T, B, 4 * H)
    xws = torch.empty(int(L.lib().t2_lstm_seq_chain_ws_floats(ns, B, H, 0)), dtype=torch.float32, device=DEV)
    a = L.LstmSeqArgs()
    a.nstreams, a.B, a.T, a.H = ns, B, T, H
    a.lengths, a.ldh = L.ptr(ln), ld
    a.ws, a.ws_floats = L.ptr(xws), xws.numel()
    for s in range(ns):
        a.pre[s], a.w_hh[s], a.reverse[s] = pre[s].data_ptr(), w[s].data_ptr(), int(streams[s][2])
        a.h[s], a.c[s], a.gates[s] = hbuf.data_ptr() + 4 * s * H, c[s].data_ptr(), gates[s].data_ptr()
    dpre, dw = nan(ns, T, B, 4 * H), nan(ns, 4 * H, H)
    before = L.get_precision(), L.get_chain()
    L.set_precision("f32")
    L.set_chain(chain)
    try:
        L.check(L.lib().t2_lstm_seq_forward(C.byref(a), L.stream()))
        if backward:
            dhbuf = nan(T, B, ld)
            for s in range(ns):
                dhbuf[:, :, s * H:(s + 1) * H] = streams[s][3].to(DEV)
            ws = torch.empty(bwd_ws_floats(ns, B, H), dtype=torch.float32, device=DEV)
            b = L.LstmSeqBwdArgs()
            b.nstreams, b.B, b.T, b.H = ns, B, T, H
            b.ldh, b.lddh = ld, ld
            b.ws, b.ws_floats = L.ptr(ws), ws.numel()
            for s in range(ns):
                b.w_hh[s], b.reverse[s] = w[s].data_ptr(), int(streams[s][2])
                b.h[s], b.c[s], b.gates[s] = a.h[s], a.c[s], a.gates[s]
                b.dh[s], b.dpre[s], b.dw_hh[s] = dhbuf.data_ptr() + 4 * s * H, dpre[s].data_ptr(), dw[s].data_ptr()
            L.check(L.lib().t2_lstm_seq_backward(C.byref(b), L.stream()))
        torch.cuda.synchronize()
    finally:
        L.set_precision(before[0])
        L.set_chain(before[1])
    if chain:
        ops.check_chain_status(block=True)
    out = [{"h": hbuf[:, :, s * H:(s + 1) * H].cpu(), "c": c[s].cpu(), "gates": gates[s].cpu()} for s in range(ns)]
    if backward:
        for s in range(ns):
            out[s].update(dpre=dpre[s].cpu(), dw_hh=dw[s].cpu())
    return out, hbuf[:, :, ns * H:].cpu()


def run_case(name, chain, **kw):
    z, x = R.CASES[name], R.inputs(name)
    streams = [(x.pre[s], x.w_hh[s], z.reverse[s], x.dh[s]) for s in range(len(z.reverse))]
    kw.setdefault("pad", z.pad)
    return gpu_run(z.H, z.B, z.T, streams, x.lengths, chain=chain, **kw)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def assert_same_bits(got, want, what, quantities=R.QUANTITIES):
    for s, (g, w) in enumerate(zip(got, want)):
        for q in quantities:
            assert same_bits(g[q], w[q]), (what, s, q)


def compare(route, name, got):
    """Every element of every output of every stream against fp64, each check printed; then: exactly zero past the lengths."""
    z, x = R.CASES[name], R.inputs(name)
    t64, dev = R.truth(name)
    bad = []
    for s in range(len(z.reverse)):
        for q in R.QUANTITIES:
            assert got[s][q].shape == t64[s][q].shape
            err = float((got[s][q].double() - t64[s][q]).abs().max())
            unit, bound = R.unit(dev[s][q], t64[s][q]), R.bound(route, q, dev[s][q], t64[s][q])
            share = 0.0 if err == 0.0 else err / unit if unit else float("inf")      # truth and dev_ref all zero: only 0 passes
            WORST[route, q] = max(WORST.get((route, q), 0.0), share)
            print(f"[{route}] {name} stream {s} {q}: err {err:.3e} dev_ref {dev[s][q]:.3e} bound {bound:.3e} err/unit {share:.3f} "
                  f"err/bound {share / R.F[route][q]:.3f} (worst err/unit of {route} {q} {WORST[route, q]:.3f})")
            if not err <= bound:
                bad.append((s, q, err, bound))
    assert not bad, (route, name, bad)
    if x.lengths is not None:
        dead = torch.arange(z.T)[:, None] >= x.lengths[None, :]
        for s in range(len(z.reverse)):
            for q in ("h", "c", "gates", "dpre"):
                assert not got[s][q][dead].any(), (route, name, s, q)


# ---------------------------------------------------------------------------------------------------------------
# the per-step route
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [z.name for z in R.PER_STEP])
def test_per_step_route(name):
    z = R.CASES[name]
    if z.chain:                                                           # the switch stays on: the plan refuses the shape
        for backward in (False, True):
            p = plan(len(z.reverse), z.B, z.H, backward)
            assert not p["covered"] and p["reason"] == env()[0].CHAIN_REFUSE_SHAPE, p
    got, padcols = run_case(name, z.chain)
    compare("per_step", name, got)
    assert bool((padcols == SENTINEL).all())
    if z.T == 1:
        assert not got[0]["dw_hh"].any()                                  # no step pair: filled with zero


# ---------------------------------------------------------------------------------------------------------------
# the persistent route, and the per-step route on the same shapes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [z.name for z in R.CHAIN])
def test_persistent_route(name):
    need_claim()
    z = R.CASES[name]
    for backward in (False, True):
        p = plan(len(z.reverse), z.B, z.H, backward)
        assert p["covered"] and p["instance_name"] == ("enc_bwd" if backward else "enc_fwd"), p
    on, _ = run_case(name, True)
    compare("chain", name, on)
    off, _ = run_case(name, False)
    compare("per_step", name, off)
    t64, dev = R.truth(name)
    for s in range(len(z.reverse)):                                       # the two routes against each other
        for q in R.QUANTITIES:
            diff = float((on[s][q].double() - off[s][q].double()).abs().max())
            bound = R.bound("chain", q, dev[s][q], t64[s][q])
            print(f"[routes] {name} stream {s} {q}: chain - per-step {diff:.3e} bound {bound:.3e} diff/bound {diff / bound if bound else 0.0:.3f}")
            if q in ("h", "c", "gates"):
                assert diff <= bound, (name, s, q, diff, bound)


# ---------------------------------------------------------------------------------------------------------------
# exact properties
# ---------------------------------------------------------------------------------------------------------------
ROUTES = [("h64_b64_t9_padded", False), ("chain_b33_t7", True)]
ROUTE_IDS = ["per_step", "chain"]


@pytest.mark.parametrize("name,chain", ROUTES, ids=ROUTE_IDS)
def test_second_run_gives_the_same_bits(name, chain):
    if chain:
        need_claim()
    first, _ = run_case(name, chain)
    second, _ = run_case(name, chain)
    assert_same_bits(second, first, name)


@pytest.mark.parametrize("name,chain", [("h512_b64_t3", False), ("chain_b32_t3", True)], ids=ROUTE_IDS)
def test_no_lengths_is_lengths_all_T(name, chain):
    if chain:
        need_claim()
    z, x = R.CASES[name], R.inputs(name)
    assert x.lengths is None
    streams = [(x.pre[s], x.w_hh[s], z.reverse[s], x.dh[s]) for s in range(len(z.reverse))]
    none, _ = gpu_run(z.H, z.B, z.T, streams, None, chain=chain)
    full, _ = gpu_run(z.H, z.B, z.T, streams, torch.full((z.B,), z.T), chain=chain)
    assert_same_bits(full, none, name)


@pytest.mark.parametrize("name,chain,k", [("h256_b32_t6_4streams", False, 1), ("chain_b33_t7", True, 1)], ids=ROUTE_IDS)
def test_stream_alone_gives_the_same_bits(name, chain, k):
    """One block works for one stream and the kernel instance depends on H and B only: stream k launched alone (its own h
    buffer, row stride H) gives what it gives among the others."""
    if chain:
        need_claim()
        assert plan(1, R.CASES[name].B, R.CASES[name].H, False)["covered"]
    z, x = R.CASES[name], R.inputs(name)
    together, _ = run_case(name, chain)
    alone, _ = gpu_run(z.H, z.B, z.T, [(x.pre[k], x.w_hh[k], z.reverse[k], x.dh[k])], x.lengths, chain=chain)
    assert_same_bits(alone, [together[k]], name)


@pytest.mark.parametrize("name,chain", [("h64_b5_t2", False), ("chain_b31_t2", True)], ids=ROUTE_IDS)
def test_wide_row_stride_leaves_the_pad_columns_alone(name, chain):
    if chain:
        need_claim()
    tight, _ = run_case(name, chain, pad=0)
    wide, padcols = run_case(name, chain, pad=64)
    assert padcols.shape[2] == 64 and bool((padcols == SENTINEL).all())
    assert_same_bits(wide, tight, name)


@pytest.mark.parametrize("name,chain", ROUTES, ids=ROUTE_IDS)
def test_forward_never_reads_pre_past_the_lengths(name, chain):
    """NaN in pre at every t >= lengths[b] changes no bit of h, c, gates.  (Not so for dh: the backward multiplies it by the
    zero gates, see t2_lstm_seq_bwd_args.)"""
    if chain:
        need_claim()
    clean, _ = run_case(name, chain, backward=False)
    dirty, _ = run_case(name, chain, backward=False, nan_pre=True)
    assert_same_bits(dirty, clean, name, ("h", "c", "gates"))


# ---------------------------------------------------------------------------------------------------------------
# refusals: argument checks in front of any launch
# ---------------------------------------------------------------------------------------------------------------
def forward_args(H, B, T=2):
    L, _ = env()
    keep = [torch.zeros(T, B, 4 * H, device=DEV), torch.zeros(4 * H, H, device=DEV), nan(T, B, H), nan(T, B, H), nan(T, B, 4 * H)]
    a = L.LstmSeqArgs()
    a.nstreams, a.B, a.T, a.H, a.ldh = 1, B, T, H, H
    a.pre[0], a.w_hh[0], a.h[0], a.c[0], a.gates[0] = (t.data_ptr() for t in keep)
    return a, keep


def test_forward_refuses_H_96():
    L, _ = env()
    a, keep = forward_args(96, 4)
    with pytest.raises(RuntimeError, match="H=96"):
        L.check(L.lib().t2_lstm_seq_forward(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in keep[2:])              # nothing ran


def test_forward_refuses_B_257():
    L, _ = env()
    a, keep = forward_args(64, 257)
    with pytest.raises(RuntimeError, match="257"):
        L.check(L.lib().t2_lstm_seq_forward(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in keep[2:])
