"""Soft-DTW on the MI355X: drop-in for the reference's ``soft_dtw_cuda.SoftDTW`` (checkpoint scoring in
best_checkpoint.py / softdtw.py), on the HIP kernels of csrc/softdtw.hip.

Differences from the reference module: sequences of any length up to 8192 frames run on the GPU (the reference leaves
the GPU above 1024), ``forward`` takes optional per-pair lengths, and there is no CPU path: CPU tensors or
``use_cuda=False`` raise."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L


def _lengths(lengths, B: int, limit: int, device) -> torch.Tensor | None:
    if lengths is None:
        return None
    t = torch.as_tensor(lengths).to(device=device, dtype=torch.int32).contiguous()
    if t.shape != (B,):
        raise RuntimeError(f"SoftDTW: lengths must have shape ({B},), got {tuple(t.shape)}")
    if int(t.min()) < 1 or int(t.max()) > limit:
        raise RuntimeError(f"SoftDTW: lengths must lie in 1..{limit}")
    return t


def _f32(t: torch.Tensor, what: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"SoftDTW: {what} must live on the GPU (the product path has no CPU fallback)")
    return t.detach().to(torch.float32).contiguous()


def _run_forward(D, Ds, B, N, M, gamma, bandwidth, xl, yl, need_grad, device):
    plan = L.softdtw_plan(B, N, M, gamma, need_grad)
    value = torch.empty(B, device=device, dtype=torch.float32)
    R = torch.empty(plan.r_floats, device=device, dtype=torch.float32) if need_grad else None
    a = L.SoftDtwFwdArgs(B, N, M, gamma, bandwidth, L.ptr(D), L.ptr(Ds), L.ptr(xl), L.ptr(yl), L.ptr(R), L.ptr(value))
    L.check(L.lib().t2_softdtw_forward(C.byref(a), L.stream()))
    return value, R


def _run_backward(D, Ds, R, B, N, M, gamma, bandwidth, xl, yl, device):
    E = torch.empty(B, N, M, device=device, dtype=torch.float32)
    a = L.SoftDtwBwdArgs(B, N, M, gamma, bandwidth, L.ptr(D), L.ptr(Ds), L.ptr(xl), L.ptr(yl), L.ptr(R), L.ptr(E))
    L.check(L.lib().t2_softdtw_backward(C.byref(a), L.stream()))
    return E


class _SoftDTWOverD(torch.autograd.Function):
    """value(D) for a caller's distance matrix; backward returns grad * E."""

    @staticmethod
    def forward(ctx, D, gamma, bandwidth, xl, yl, grad_mode):
        Dc = _f32(D, "D")
        B, N, M = Dc.shape
        need = grad_mode and ctx.needs_input_grad[0]
        value, R = _run_forward(Dc, None, B, N, M, gamma, bandwidth, xl, yl, need, Dc.device)
        if need:
            ctx.save_for_backward(Dc, R)
            ctx.meta = (gamma, bandwidth, xl, yl)
        return value.to(D.dtype)

    @staticmethod
    def backward(ctx, grad):
        Dc, R = ctx.saved_tensors
        gamma, bandwidth, xl, yl = ctx.meta
        B, N, M = Dc.shape
        E = _run_backward(Dc, None, R, B, N, M, gamma, bandwidth, xl, yl, Dc.device)
        return (grad.to(torch.float32).view(-1, 1, 1) * E).to(grad.dtype), None, None, None, None, None


class _SoftDTWEuclidean(torch.autograd.Function):
    """value(X, Y) with the squared Euclidean distance: distance kernel + recurrence, gradients to X and Y."""

    @staticmethod
    def forward(ctx, X, Y, gamma, bandwidth, xl, yl, grad_mode):
        Xc, Yc = _f32(X, "X"), _f32(Y, "Y")
        B, N, d = Xc.shape
        M = Yc.shape[1]
        need = grad_mode and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        plan = L.softdtw_plan(B, N, M, gamma, need)
        Ds = torch.empty(plan.d_floats, device=Xc.device, dtype=torch.float32)
        a = L.SoftDtwDistArgs(B, N, M, d, L.ptr(Xc), L.ptr(Yc), L.ptr(Ds))
        L.check(L.lib().t2_softdtw_dist(C.byref(a), L.stream()))
        value, R = _run_forward(None, Ds, B, N, M, gamma, bandwidth, xl, yl, need, Xc.device)
        if need:
            ctx.save_for_backward(Xc, Yc, Ds, R)
            ctx.meta = (gamma, bandwidth, xl, yl)
        return value.to(X.dtype)

    @staticmethod
    def backward(ctx, grad):
        Xc, Yc, Ds, R = ctx.saved_tensors
        gamma, bandwidth, xl, yl = ctx.meta
        B, N, d = Xc.shape
        M = Yc.shape[1]
        E = _run_backward(None, Ds, R, B, N, M, gamma, bandwidth, xl, yl, Xc.device)
        g = grad.detach().to(torch.float32).contiguous()
        dX, dY = torch.empty_like(Xc), torch.empty_like(Yc)
        a = L.SoftDtwDistBwdArgs(B, N, M, d, L.ptr(Xc), L.ptr(Yc), L.ptr(E), L.ptr(g), L.ptr(xl), L.ptr(yl), L.ptr(dX), L.ptr(dY))
        L.check(L.lib().t2_softdtw_dist_backward(C.byref(a), L.stream()))
        return dX.to(grad.dtype), dY.to(grad.dtype), None, None, None, None, None


class SoftDTW(torch.nn.Module):
    """SoftDTW(use_cuda, gamma=1.0, normalize=False, bandwidth=None, dist_func=None), as the reference's module.

    forward(X [B,N,d], Y [B,M,d], x_lengths=None, y_lengths=None) -> [B].  With lengths, pair b is X[b, :x_lengths[b]] against
    Y[b, :y_lengths[b]] (bit-identical to running it alone); gradients are zero in the padding.  dist_func=None: squared
    Euclidean distance in HIP, gradients flow to X and Y.  dist_func given: torch computes D = dist_func(X, Y) and the
    recurrence is differentiated with respect to D."""

    def __init__(self, use_cuda, gamma=1.0, normalize=False, bandwidth=None, dist_func=None):
        super().__init__()
        if not use_cuda:
            raise RuntimeError("SoftDTW(use_cuda=False): this package has no CPU path for soft-DTW")
        self.use_cuda = True
        self.normalize = normalize
        self.gamma = float(gamma)
        self.bandwidth = 0.0 if bandwidth is None else float(bandwidth)
        self.dist_func = dist_func

    def _value(self, X, Y, xl, yl):
        # R is stored only when a backward pass can follow.  The caller's grad mode has to be read here: inside a Function's
        # forward grad mode is always off, and ctx.needs_input_grad looks at requires_grad alone, not at torch.no_grad().
        grad_mode = torch.is_grad_enabled()
        if self.dist_func is None:
            return _SoftDTWEuclidean.apply(X, Y, self.gamma, self.bandwidth, xl, yl, grad_mode)
        D = self.dist_func(X, Y)
        return _SoftDTWOverD.apply(D, self.gamma, self.bandwidth, xl, yl, grad_mode)

    def forward(self, X, Y, x_lengths=None, y_lengths=None):
        if not (X.is_cuda and Y.is_cuda):
            raise RuntimeError("SoftDTW: X and Y must live on the GPU (the product path has no CPU fallback)")
        if X.dim() != 3 or Y.dim() != 3 or X.shape[0] != Y.shape[0] or X.shape[2] != Y.shape[2]:
            raise RuntimeError(f"SoftDTW: expected X [B,N,d] and Y [B,M,d], got {tuple(X.shape)} and {tuple(Y.shape)}")
        if (x_lengths is None) != (y_lengths is None):
            raise RuntimeError("SoftDTW: give both x_lengths and y_lengths or neither")
        B, N, M = X.shape[0], X.shape[1], Y.shape[1]
        xl, yl = _lengths(x_lengths, B, N, X.device), _lengths(y_lengths, B, M, X.device)
        if not self.normalize:
            return self._value(X, Y, xl, yl)
        x, y = torch.cat([X, X, Y]), torch.cat([Y, X, Y])
        if xl is not None:
            xl, yl = torch.cat([xl, xl, yl]), torch.cat([yl, xl, yl])
        out_xy, out_xx, out_yy = torch.split(self._value(x, y, xl, yl), B)
        return out_xy - 1 / 2 * (out_xx + out_yy)
