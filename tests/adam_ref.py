"""fp64 restatement (numpy only) of torch.nn.utils.clip_grad_norm_ followed by one torch.optim.Adam step, for one tensor:

    g' = g*clip + wd*p
    m' = m + (1-b1)(g'-m)
    v' = b2*v + (1-b2)*g'^2
    p' = p - lr/(1-b1^t) * m' / (sqrt(v')/sqrt(1-b2^t) + eps)

and the elementwise error bounds a float32 implementation of it is held to (tests/test_gpu_optim.py).

The hyper-parameters enter as the C floats the ABI receives (`hyper()`): 1.0f - 0.999f differs from 0.001 by 1.3e-5
relative, which is consistent Adam with beta2 = float32(0.999), not an error.  (1 - b is exact in float32 for b in
[0.5, 1], so 1 - b in fp64 from the rounded b is the very number the kernel multiplies with.)

Bounds, u = 2^-24, tiny = 2^-126, a = |g*clip| + |wd*p| (not |g'|: g' can cancel), l1 = lr/(1-b1^t),
den = sqrt(v'64)/sqrt(1-b2^t) + eps, step64 = l1*m'64/den:

    m:  bm = 6u(|m| + a) + tiny
    v:  bv = 12u(b2*v + (1-b2)*a^2) + tiny
    p:  bp = 2u|p'64| + 14u|step64| + l1*bm/den + 2|step64|*dden/den + tiny,
        dden = min(sqrt(bv), bv/(2 sqrt(v'64))) / sqrt(1-b2^t)

Norm: |norm - norm64| <= 32u*norm64 (one product, 32 sequential adds, 6 wave levels and 2 block adds on non-negative terms,
then an fp64 finish, a square root that halves the relative error and one cast; 32u is that with a margin of about 1.5)."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
NORM_BOUND = 32 * U


def f32(x):
    """The double a C float argument holds."""
    return float(np.float32(x))


def hyper(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """Hyper-parameters as the C floats t2_adam_step receives: dict(lr, b1, b2, eps, wd) of Python floats."""
    return dict(lr=f32(lr), b1=f32(betas[0]), b2=f32(betas[1]), eps=f32(eps), wd=f32(weight_decay))


def total_norm(grads):
    """fp64 2-norm over all elements of all arrays."""
    return float(np.sqrt(sum(float(np.sum(np.square(np.asarray(g, dtype=np.float64)))) for g in grads)))


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient in fp64: min(1, max_norm / (norm + 1e-6)); NaN when the norm is NaN."""
    c = max_norm / (norm + 1e-6)
    return c if (c < 1.0 or c != c) else 1.0


def clip_coef_f32(norm, max_norm):
    """The coefficient in float32 arithmetic from a float32 norm, bit for bit what the device must hold (IEEE add and
    divide, no fast-math); max_norm <= 0: no clipping."""
    if not max_norm > 0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return c if (c < np.float32(1.0) or c != c) else np.float32(1.0)


def step(p, g, m, v, clip, t, lr, b1, b2, eps, wd):
    """One step in fp64 from inputs of any float type.  Returns dict(p, m, v: the new values; bp, bm, bv: the bounds of
    the module docstring, same shape)."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    clip, t = float(clip), int(t)
    with np.errstate(all="ignore"):
        g1 = g * clip + wd * p
        m1 = m + (1.0 - b1) * (g1 - m)
        v1 = b2 * v + (1.0 - b2) * g1 * g1
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        l1 = lr / bc1
        den = np.sqrt(v1) / np.sqrt(bc2) + eps
        step64 = l1 * m1 / den
        p1 = p - step64
        a = np.abs(g * clip) + np.abs(wd * p)
        bm = 6 * U * (np.abs(m) + a) + TINY
        bv = 12 * U * (b2 * v + (1.0 - b2) * a * a) + TINY
        dden = np.minimum(np.sqrt(bv), bv / (2.0 * np.sqrt(v1))) / np.sqrt(bc2)
        bp = 2 * U * np.abs(p1) + 14 * U * np.abs(step64) + l1 * bm / den + 2.0 * np.abs(step64) * dden / den + TINY
    return dict(p=p1, m=m1, v=v1, bp=bp, bm=bm, bv=bv)
