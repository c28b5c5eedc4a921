"""SSIM on the MI355X: drop-in for the reference's ``ssim`` module (``from ssim import SSIM``, the loss term of
loss_function.py:10,24), on the HIP kernels of csrc/ssim.hip.

fp32 images on the GPU with an odd window go through one fused forward launch (+ a finishing launch) and one backward
launch; moments, the subtraction E[xx] - mu^2 and the algebra run in fp64 there, so value and gradient stay accurate on
log-mel silence, where the torch-op statement below loses most of its digits in fp32.  Everything else
(CPU tensors, other dtypes, an even window) takes ``_ssim``, the torch-op statement of ssim.py:17-37."""
from __future__ import annotations

from math import exp

import torch
import torch.nn.functional as F

from . import _lib as L

_SIGMA = 1.5


def gaussian(window_size, sigma):
    """ssim.py:7-9: the normalised 1-D taps, rounded to fp32 before and after the division as torch.Tensor does."""
    centre = window_size // 2
    g = torch.tensor([exp(-(i - centre) ** 2 / float(2 * sigma ** 2)) for i in range(window_size)], dtype=torch.float32)
    return g / g.sum()


def create_window(window_size, channel):
    """ssim.py:11-15: the fp32 outer product of the taps, one copy per channel, [channel, 1, ws, ws]."""
    col = gaussian(window_size, _SIGMA).unsqueeze(1)
    return col.mm(col.t()).float().unsqueeze(0).unsqueeze(0).expand(channel, 1, window_size, window_size).contiguous()


def _ssim(img1, img2, window, window_size, channel, size_average=True):
    """ssim.py:17-37 in torch ops: depthwise convolutions under zero padding for the five moments, then S and its mean."""
    pad = window_size // 2
    blur = lambda t: F.conv2d(t, window, padding=pad, groups=channel)
    mu1, mu2 = blur(img1), blur(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = blur(img1 * img1) - mu1_sq
    sigma2_sq = blur(img2 * img2) - mu2_sq
    sigma12 = blur(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean() if size_average else ssim_map.mean(1).mean(1).mean(1)


# ------------------------------------------------------------------------------------------------------------------
# the HIP path
# ------------------------------------------------------------------------------------------------------------------
_taps_cache: dict = {}


def _taps(window_size: int, device) -> torch.Tensor:
    """The taps on the device, uploaded once per (window, device): a call never copies from the host again."""
    key = (int(window_size), str(device))
    t = _taps_cache.get(key)
    if t is None:
        t = _taps_cache[key] = gaussian(window_size, _SIGMA).to(device)
    return t


def _on_hip_path(img1, img2, window_size) -> bool:
    return (img1.is_cuda and img2.is_cuda and img1.dtype == torch.float32 and img2.dtype == torch.float32
            and img1.dim() == 4 and img1.shape == img2.shape and window_size % 2 == 1 and 1 <= window_size <= 31 and img1.numel() > 0)


def _image(t: torch.Tensor) -> torch.Tensor:
    """t itself where the kernels can address it (one inner stride 1, evenly spaced planes), else a contiguous copy."""
    B, Cn, H, W = t.shape
    sb, sc, sh, sw = t.stride()
    inner = sw == 1 or W == 1 or sh == 1 or H == 1
    planes = B == 1 or Cn == 1 or sb == Cn * sc
    return t if inner and planes else t.contiguous()


def _forward(x, y, window_size, need, want_value, want_items, want_map):
    B, Cn, H, W = x.shape
    plan = L.ssim_plan(B * Cn, H, W, window_size, need)
    dev = x.device
    partial = torch.empty(plan.partial_bytes // 8, device=dev, dtype=torch.float64)
    coef = torch.empty(plan.map_bytes // 8, device=dev, dtype=torch.float64) if need else None
    value = torch.empty(1, device=dev, dtype=torch.float32) if want_value else None
    items = torch.empty(B, device=dev, dtype=torch.float32) if want_items else None
    smap = torch.empty(B, Cn, H, W, device=dev, dtype=torch.float32) if want_map else None
    taps = _taps(window_size, dev)
    a = L.SsimFwdArgs(B, Cn, H, W, window_size, need, L.ssim_image(x), L.ssim_image(y), L.ssim_image(smap), L.ptr(taps), L.ptr(partial),
                      L.ptr(coef), L.ptr(value), L.ptr(items))
    L.ssim_forward(a)
    return value, items, smap, coef


class _SSIMFunction(torch.autograd.Function):
    """mean SSIM (a 0-dim tensor, or [B] with size_average=False); backward filters the stored coefficient maps."""

    @staticmethod
    def forward(ctx, img1, img2, window_size, size_average, grad_mode):
        x, y = _image(img1.detach()), _image(img2.detach())
        need = ((1 if ctx.needs_input_grad[0] else 0) | (2 if ctx.needs_input_grad[1] else 0)) if grad_mode else 0
        value, items, _, coef = _forward(x, y, window_size, need, size_average, not size_average, False)
        if need:
            ctx.save_for_backward(x, y, coef)
            ctx.meta = (window_size, need, size_average)
        return value.reshape(()) if size_average else items

    @staticmethod
    def backward(ctx, grad):
        x, y, coef = ctx.saved_tensors
        window_size, need, size_average = ctx.meta
        B, Cn, H, W = x.shape
        g = grad.detach().to(torch.float32).reshape(-1).contiguous()
        dx = torch.empty_like(x) if need & 1 else None
        dy = torch.empty_like(y) if need & 2 else None
        a = L.SsimBwdArgs(B, Cn, H, W, window_size, need, 0 if size_average else 1, L.ssim_image(x), L.ssim_image(y), L.ssim_image(dx),
                          L.ssim_image(dy), L.ptr(_taps(window_size, x.device)), L.ptr(coef), L.ptr(g))
        L.ssim_backward(a)
        return dx, dy, None, None, None


def _hip_ssim(img1, img2, window_size, size_average):
    # grad mode is read here: inside a Function's forward it is always off, and needs_input_grad ignores torch.no_grad()
    return _SSIMFunction.apply(img1, img2, int(window_size), bool(size_average), torch.is_grad_enabled())


class SSIM(torch.nn.Module):
    """SSIM(window_size=11, size_average=True), ssim.py:39-63, with its attributes; forward(img1, img2) on [B,C,H,W]."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        self.window_size = window_size
        self.size_average = size_average
        self.channel = 1
        self.window = create_window(window_size, self.channel)

    def forward(self, img1, img2):
        channel = img1.size(1)
        if channel == self.channel and self.window.type() == img1.type():
            window = self.window
        else:                                   # ssim.py:52-60: a new window for another channel count or tensor type
            window = create_window(self.window_size, channel)
            if img1.is_cuda:
                window = window.cuda(img1.get_device())
            window = window.type_as(img1)
            self.window = window
            self.channel = channel
        if _on_hip_path(img1, img2, self.window_size):
            return _hip_ssim(img1, img2, self.window_size, self.size_average)
        return _ssim(img1, img2, window, self.window_size, channel, self.size_average)


def ssim(img1, img2, window_size=11, size_average=True):
    """ssim.py:65-73."""
    if _on_hip_path(img1, img2, window_size):
        return _hip_ssim(img1, img2, window_size, size_average)
    channel = img1.size(1)
    window = create_window(window_size, channel)
    if img1.is_cuda:
        window = window.cuda(img1.get_device())
    window = window.type_as(img1)
    return _ssim(img1, img2, window, window_size, channel, size_average)


def ssim_map(img1, img2, window_size=11):
    """S per pixel, [B,C,H,W] (no gradient): the map whose mean ``ssim`` returns.  GPU fp32 images, odd window."""
    if not _on_hip_path(img1, img2, window_size):
        raise RuntimeError("ssim_map: needs two fp32 [B,C,H,W] images of one shape on the GPU and an odd window of at most 31")
    return _forward(_image(img1.detach()), _image(img2.detach()), int(window_size), 0, False, False, True)[2]
