"""fp64 restatement of SSIM (ssim.py:17-37 of the reference) for the tests: separable, built from the fp32 1-D taps
exactly as the kernels receive them, zero padding of ws // 2.  The truth of every kernel test.

It differs from the reference's own statement in one place: the reference's 2-D window is the fp32-rounded outer
product of the taps, this one is the exact product of the two 1-D passes.  The fixture records what that perturbation
is worth per case (win_*)."""
from math import exp

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps32(ws: int, sigma: float = 1.5) -> torch.Tensor:
    """ssim.py:7-9 with torch's own fp32 rounding."""
    g = torch.tensor([exp(-(i - ws // 2) ** 2 / float(2 * sigma ** 2)) for i in range(ws)], dtype=torch.float32)
    return g / g.sum()


def blur(t: torch.Tensor, ws: int) -> torch.Tensor:
    """The zero-padded separable window on [B,C,H,W] fp64: along W, then along H."""
    B, Cn, H, W = t.shape
    w = taps32(ws).to(torch.float64)
    r = ws // 2
    t = t.reshape(B * Cn, 1, H, W)
    t = F.conv2d(t, w.view(1, 1, 1, ws), padding=(0, r))
    t = F.conv2d(t, w.view(1, 1, ws, 1), padding=(r, 0))
    return t.reshape(B, Cn, H, W)


def parts(x: torch.Tensor, y: torch.Tensor, ws: int) -> dict:
    x, y = x.to(torch.float64), y.to(torch.float64)
    mu1, mu2 = blur(x, ws), blur(y, ws)
    s1, s2, s12 = blur(x * x, ws) - mu1 * mu1, blur(y * y, ws) - mu2 * mu2, blur(x * y, ws) - mu1 * mu2
    A1, A2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    return dict(x=x, y=y, mu1=mu1, mu2=mu2, A1=A1, A2=A2, B1=B1, B2=B2, S=A1 * A2 / (B1 * B2))


def ssim_map(x, y, ws: int = 11) -> torch.Tensor:
    return parts(x, y, ws)["S"]


def ssim_value(x, y, ws: int = 11, size_average: bool = True) -> torch.Tensor:
    S = ssim_map(x, y, ws)
    return S.mean() if size_average else S.mean(dim=(1, 2, 3))


def ssim_grad(x, y, ws: int = 11, grad=1.0, size_average: bool = True):
    """Analytic (dx, dy) of grad * value (size_average) or of sum_b grad[b] * items[b]: with a = dS/dmu1 at fixed
    sigmas, b = dS/dsigma1^2 = -S/B2, c = dS/dsigma12 = 2 A1 / (B1 B2),
    dx = g * (F[a - 2 b mu1 - c mu2] + 2 x F[b] + y F[c]); dy with the roles swapped."""
    p = parts(x, y, ws)
    x, y, mu1, mu2, S = p["x"], p["y"], p["mu1"], p["mu2"], p["S"]
    B, Cn, H, W = x.shape
    g = torch.as_tensor(grad, dtype=torch.float64)
    g = g / (B * Cn * H * W) if size_average else (g / (Cn * H * W)).reshape(B, 1, 1, 1)
    b = -S / p["B2"]
    c = 2 * p["A1"] / (p["B1"] * p["B2"])
    a1 = 2 * mu2 * p["A2"] / (p["B1"] * p["B2"]) - 2 * mu1 * S / p["B1"]
    a2 = 2 * mu1 * p["A2"] / (p["B1"] * p["B2"]) - 2 * mu2 * S / p["B1"]
    Fb, Fc = blur(b, ws), blur(c, ws)
    dx = g * (blur(a1 - 2 * b * mu1 - c * mu2, ws) + 2 * x * Fb + y * Fc)
    dy = g * (blur(a2 - 2 * b * mu2 - c * mu1, ws) + 2 * y * Fb + x * Fc)
    return dx, dy


def reference_form(x, y, ws: int = 11, size_average: bool = True, dtype=torch.float64):
    """The reference's own arrangement (a 2-D window that is the fp32 outer product of the taps, one grouped conv2d per
    moment) in `dtype`, written out here so a test can measure its fp32 deviation on shapes the fixture does not hold.
    Returns (value, map)."""
    Cn = x.shape[1]
    col = taps32(ws).unsqueeze(1)
    win = col.mm(col.t()).to(dtype).expand(Cn, 1, ws, ws).contiguous()
    x, y = x.to(dtype), y.to(dtype)
    cv = lambda t: F.conv2d(t, win, padding=ws // 2, groups=Cn)
    mu1, mu2 = cv(x), cv(y)
    s1, s2, s12 = cv(x * x) - mu1 * mu1, cv(y * y) - mu2 * mu2, cv(x * y) - mu1 * mu2
    S = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return (S.mean() if size_average else S.mean(1).mean(1).mean(1)), S
