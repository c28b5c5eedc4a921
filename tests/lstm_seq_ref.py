"""The operation behind t2_lstm_seq_forward / t2_lstm_seq_backward (include/t2amd.h) restated plainly in torch on the CPU,
parameterised by dtype, together with what the CPU tests (test_lstm_seq_ref_cpu.py) and the GPU tests
(test_gpu_lstm_seq.py) share: the cases, their inputs, the truth of a case and the bound of a comparison.

One stream: pre [T,B,4H] (input pre-activations, biases included), w_hh [4H,H], reverse, lengths [B] or None.
Gate order i, f, g, o.  The state is zero before the first processed step.  At a time index t >= lengths[b] the item's h,
c and all four saved gates are zero and so is the state it carries on: a reverse stream (t = T-1 ... 0) therefore starts
each item at its own last frame.  Returns h [T,B,H], c [T,B,H], gates [T,B,4H]; with dh, dpre and dw_hh by autograd.

`defect` names one deliberate mistake (DEFECTS): the sensitivity tests apply each to the fp64 statement and ask the
bound to reject it."""
import collections
import functools

import torch

DEFECTS = ("drop_k", "swap_fo", "state_kept_past_length", "reverse_starts_from_kept_state", "dw_misses_first_pair")
QUANTITIES = ("h", "c", "gates", "dpre", "dw_hh")


def forward(pre, w_hh, reverse, lengths=None, defect=None, kept=None):
    """h, c, gates of one stream.  kept: the (h, c) a run before this one left behind (only the defect
    reverse_starts_from_kept_state reads it)."""
    T, B, H4 = pre.shape
    H = H4 // 4
    zero = pre.new_zeros(B, H)
    h, c = zero, zero
    if defect == "reverse_starts_from_kept_state" and reverse and kept is not None:
        h, c = kept
    hs, cs, gs = [None] * T, [None] * T, [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        if defect == "drop_k":                                            # the last 64 columns of K are not summed
            z = pre[t] + h[:, :H - 64] @ w_hh[:, :H - 64].T
        else:
            z = pre[t] + h @ w_hh.T
        i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
        if defect == "swap_fo":
            f, o = o, f
        c_new = f * c + i * g
        h_new = o * torch.tanh(c_new)
        gates = torch.cat((i, f, g, o), 1)
        if lengths is not None:
            live = (t < lengths)[:, None]
            hs[t], cs[t], gs[t] = torch.where(live, h_new, zero), torch.where(live, c_new, zero), torch.where(live, gates, gates.new_zeros(()))
            h, c = (h_new, c_new) if defect == "state_kept_past_length" else (hs[t], cs[t])
        else:
            hs[t], cs[t], gs[t] = h_new, c_new, gates
            h, c = h_new, c_new
    return torch.stack(hs), torch.stack(cs), torch.stack(gs)


def run(pre, w_hh, reverse, lengths, dh, dtype, defect=None, kept=None):
    """{h, c, gates, dpre, dw_hh} of one stream in `dtype`; the gradients are those of sum(h * dh)."""
    p = pre.to(dtype).requires_grad_(True)
    w = w_hh.to(dtype).requires_grad_(True)
    if kept is not None:
        kept = tuple(k.to(dtype) for k in kept)
    h, c, gates = forward(p, w, reverse, lengths, defect, kept)
    dpre, dw = torch.autograd.grad((h * dh.to(dtype)).sum(), (p, w), allow_unused=True)
    if dw is None:                                                        # T = 1: the recurrent weights are never read
        dw = torch.zeros_like(w)
    if defect == "dw_misses_first_pair" and pre.shape[0] > 1:             # (second processed step's dpre)^T . (first one's h)
        T = pre.shape[0]
        t0, t1 = (T - 1, T - 2) if reverse else (0, 1)
        dw = dw - dpre[t1].T @ h[t0].detach()
    return {"h": h.detach(), "c": c.detach(), "gates": gates.detach(), "dpre": dpre, "dw_hh": dw}


# ------------------------------------------------------------------------------------------------------------------
# The cases of the GPU tests.  lengths: None, a list, or the name of a rule of make_lengths.
# ------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name H B T reverse lengths pad chain")

# The per-step route (csrc/lstm.hip).  Forward: step 0 has no recurrent segment and takes the widest stage of its row-tile
# count; every later step takes the instance of K = H.  Backward: the instance of K = 4H / ksplit.  `chain`: the switch is
# left on and the plan must refuse the shape.
PER_STEP = (
    Case("h64_b1_t1", 64, 1, 1, (0,), None, 0, False),                         # fwd step 0 <1,256>; no bwd product: dw_hh filled with 0
    Case("h64_b5_t2", 64, 5, 2, (0, 1), [2, 1, 2, 1, 1], 0, False),            # fwd <1,64>        bwd <1,64>
    Case("h64_b64_t9_padded", 64, 64, 9, (0, 1), "unsorted", 64, False),       # fwd <2,64>        bwd <2,64>   ldh = lddh = 2H + 64
    Case("h192_b33_t5_3streams", 192, 33, 5, (1, 0, 1), "unsorted", 0, False), # fwd <2,64>        bwd <2,64>   ksplit 4
    Case("h128_b97_t4", 128, 97, 4, (0, 1), "unsorted", 0, False),             # fwd <4,128>       bwd <4,64>
    Case("h192_b128_t3_short", 192, 128, 3, (1, 0), "below_T", 0, False),      # fwd <4,64>        bwd <4,64>   max(lengths) = 2 < T
    Case("h256_b32_t6_4streams", 256, 32, 6, (0, 1, 0, 1), "unsorted", 0, True),   # fwd <1,256>   bwd <1,64>   refused: 4 streams
    Case("h256_b129_t3", 256, 129, 3, (0, 1), "tail_group_1", 0, True),        # fwd <8,64>        bwd <8,64>   refused: B = 129
    Case("h256_b256_t3", 256, 256, 3, (1,), None, 0, False),                   # fwd <8,64>        bwd <8,64>   largest batch
    Case("h256_b128_t3", 256, 128, 3, (0, 1), "unsorted", 0, False),           # fwd <4,128>       bwd <4,128>
    Case("h512_b31_t4", 512, 31, 4, (0, 1), "unsorted", 0, False),             # fwd <1,256>       bwd <1,256>
    Case("h512_b64_t3", 512, 64, 3, (0, 1), None, 0, False),                   # fwd <2,256>       bwd <2,256>
)
# The persistent route (csrc/chain_enc.hip): H = 256, the switch on, the plan covers the shape.
CHAIN = (
    Case("chain_b1_t1", 256, 1, 1, (1,), None, 0, True),
    Case("chain_b31_t2", 256, 31, 2, (0, 1), "unsorted", 0, True),
    Case("chain_b32_t3", 256, 32, 3, (0, 1), None, 0, True),                   # T = 3: both parities of the exchange buffers once
    Case("chain_b33_t7", 256, 33, 7, (0, 1), "tail_group_1", 0, True),         # the one item of the second row group has length 1
    Case("chain_b97_t4", 256, 97, 4, (1, 0), "unsorted", 0, True),
    Case("chain_b128_t5", 256, 128, 5, (0, 1), "group1_short", 0, True),       # every item of rows 32..63 has length <= 2
    Case("chain_b33_t50", 256, 33, 50, (0, 1), "below_T", 0, True),            # max(lengths) = 47 < T
)
CASES = {c.name: c for c in PER_STEP + CHAIN}
# the cases the sensitivity tests run: per-step, a chain shape, one more with two reverse streams
SENSITIVITY = ("h64_b64_t9_padded", "chain_b33_t7", "h192_b33_t5_3streams")


def make_lengths(rule, B, T, g):
    if rule is None:
        return None
    if isinstance(rule, list):
        n = torch.tensor(rule)
    else:
        top = {"below_T": T - (3 if T > 10 else 1)}.get(rule, T)
        n = torch.randint(1, top + 1, (B,), generator=g)
        n[B // 2] = top                                                   # the longest item sits in the middle,
        n[0] = 1                                                          # the first one is the shortest: not sorted
        n[B - 1] = max(1, top - 1)
        if rule == "tail_group_1":
            n[(B - 1) // 32 * 32:] = 1
        if rule == "group1_short":
            n[32:64] = torch.randint(1, 3, (32,), generator=g)
    assert n.shape == (B,) and int(n.min()) >= 1 and int(n.max()) <= T
    return n


Inputs = collections.namedtuple("Inputs", "pre w_hh dh lengths")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """fp32 inputs of a case: pre ~ 1.5 N(0,1), w_hh ~ N(0,1) / sqrt(H), dh ~ N(0,1) everywhere (padding included)."""
    z = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 1)
    ns = len(z.reverse)
    pre = [1.5 * torch.randn(z.T, z.B, 4 * z.H, generator=g) for _ in range(ns)]
    w = [torch.randn(4 * z.H, z.H, generator=g) / z.H ** 0.5 for _ in range(ns)]
    dh = [torch.randn(z.T, z.B, z.H, generator=g) for _ in range(ns)]
    return Inputs(pre, w, dh, make_lengths(z.lengths, z.B, z.T, g))


def statement(name, dtype, defect=None):
    """[{h, c, gates, dpre, dw_hh}] per stream of a case, stated in `dtype`."""
    z, x = CASES[name], inputs(name)
    out, kept = [], None
    for s, rev in enumerate(z.reverse):
        out.append(run(x.pre[s], x.w_hh[s], rev, x.lengths, x.dh[s], dtype, defect, kept))
        t_last = 0 if rev else z.T - 1
        kept = (out[-1]["h"][t_last], out[-1]["c"][t_last]) if kept is None else kept   # what the first stream's run leaves behind
    return out


@functools.lru_cache(maxsize=None)
def truth(name):
    """(truth, dev_ref): the fp64 statement per stream, and per stream and quantity the deviation of the fp32 statement
    from it."""
    t64, t32 = statement(name, torch.float64), statement(name, torch.float32)
    dev = [{q: float((a[q].double() - b[q]).abs().max()) for q in QUANTITIES} for a, b in zip(t32, t64)]
    return t64, dev


# ------------------------------------------------------------------------------------------------------------------
# The bound of a comparison: F * max(dev_ref, 2^-23 * max|truth|), as tests/test_gpu_bert.py.  F per route and quantity
# was measured on the kernels against the fp64 statement (test_gpu_lstm_seq.py has the figures): the smallest power of
# two that leaves at least 2 x over the worst err / max(dev_ref, floor) seen.
# ------------------------------------------------------------------------------------------------------------------
F = {
    "per_step": {"h": 4.0, "c": 4.0, "gates": 2.0, "dpre": 4.0, "dw_hh": 8.0},
    "chain": {"h": 4.0, "c": 4.0, "gates": 2.0, "dpre": 4.0, "dw_hh": 8.0},
}


def unit(dev_ref, truth_tensor):
    """max(dev_ref, one fp32 rounding of the largest truth value): what F multiplies."""
    return max(float(dev_ref), 2.0 ** -23 * float(truth_tensor.abs().max()))


def bound(route, quantity, dev_ref, truth_tensor):
    return F[route][quantity] * unit(dev_ref, truth_tensor)
