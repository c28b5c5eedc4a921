"""Reference side of the split-bf16 recurrent steps (t2_set_split_steps, csrc/lstm.hip): a torch emulation of the
three-term product in the kernels' order of K slices, the per-element error bound the GPU tests hold the kernels to, and
the fp64 evaluation of one LSTM step's gates from the operands a pass saved.  CPU only."""
import torch

NW = 8                      # waves of a workgroup: each owns one eighth of every K stage (csrc/lstm.hip)
BOUND_C = 8 * 2.0 ** -17    # bound = BOUND_C * sqrt(sum_k x_k^2 w_k^2) per output element


def split_hi_lo(x):
    """fp32 -> (hi, lo) as fp32 tensors holding bf16 values: hi = bf16(x), lo = bf16(x - hi), round to nearest even."""
    assert x.dtype == torch.float32
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


def split_product(x, w, bkt, ksplit=1, terms=("hh", "lh", "hl")):
    """x [M,K] . w [N,K]^T as the split kernels compute it.  K is cut into `ksplit` spans (the K-split grid of the gradient
    kernel; 1 for the forward step), a span into stages of `bkt` columns, a stage into NW wave slices, a slice into 16-wide
    MFMA steps.  Every wave keeps one fp32 accumulator over all stages of its span and adds, per step, the terms in the order
    given ("hh" = hi.hi, "lh" = x_lo.w_hi, "hl" = x_hi.w_lo); the NW accumulators are then summed in wave order from 0, the
    spans in span order from 0.  (The sum inside one 16-wide step is taken in fp32 here; the hardware's order there is its own.)"""
    M, K = x.shape
    assert w.shape[1] == K and K % ksplit == 0 and (K // ksplit) % bkt == 0 and bkt % (NW * 16) == 0
    xh, xl = split_hi_lo(x)
    wh, wl = split_hi_lo(w)
    ops = {"hh": (xh, wh), "lh": (xl, wh), "hl": (xh, wl)}
    span, per_wave = K // ksplit, bkt // NW
    total = torch.zeros(M, w.shape[0])
    for z in range(ksplit):
        acc = [torch.zeros(M, w.shape[0]) for _ in range(NW)]
        for c in range(span // bkt):
            for wave in range(NW):
                for kk in range(0, per_wave, 16):
                    k0 = z * span + c * bkt + wave * per_wave + kk
                    for name in terms:
                        a, b = ops[name]
                        acc[wave] = acc[wave] + a[:, k0:k0 + 16] @ b[:, k0:k0 + 16].T
        part = torch.zeros(M, w.shape[0])
        for wave in range(NW):
            part = part + acc[wave]
        total = total + part
    return total


def product_bound(x, w):
    """Per output element [M,N]: BOUND_C * sqrt(sum_k x[m,k]^2 w[n,k]^2), in fp64."""
    return BOUND_C * torch.sqrt((x.double() ** 2) @ (w.double() ** 2).T)


def error_ratio(got, x, w):
    """max over the output of |got - fp64 product| / bound"""
    ref = x.double() @ w.double().T
    return float(((got.double() - ref).abs() / product_bound(x, w)).max())


def bf16_product_bound(x, w):
    """Per output element [M,N], for operands that hold bf16 values (the bf16-operand steps): products of two bf16 numbers
    are exact in fp32, so only the accumulation rounds — K additions, the sum of the NW wave partials and the addition of
    the pre-activation, (K + 16) * 2^-23 * sum_k |x||w| (2^-23, not 2^-24: the matrix core's internal additions are not
    promised to round to nearest)."""
    return (x.shape[1] + 16) * 2.0 ** -23 * (x.double().abs() @ w.double().abs().T)


def step_gates_fp64(pre, x_prev, w, bound_fn=product_bound):
    """Activated gates (i, f, g, o blocks of H columns) of one LSTM step in fp64, and the bound of the recurrent product per
    element: pre [B,4H] = the hoisted input-side pre-activations (biases included), x_prev [B,K] = the recurrent operand
    rows of step t-1 (None at t = 0), w [4H,K].  The activations' derivatives are <= 1, so the pre-activation's bound holds
    for the activated gate."""
    z = pre.double()
    bound = torch.zeros_like(z)
    if x_prev is not None:
        z = z + x_prev.double() @ w.double().T
        bound = bound_fn(x_prev, w)
    H = z.shape[1] // 4
    g = torch.cat([torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])], 1)
    return g, bound
