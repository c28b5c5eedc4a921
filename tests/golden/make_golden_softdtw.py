#!/usr/bin/env python3
"""Golden vectors for soft-DTW, recorded from the reference's own soft_dtw_cuda.py: the values and dD gradients of its
host implementation (_SoftDTW, :185-270) on four cases, and one SoftDTW(False, gamma=0.1, normalize=True) case with value
and dX.  The reference module imports numba, which is not installed: a stand-in module whose jit / cuda.jit decorators
return the function unchanged lets its host loops run as plain Python.  Run in the build container only (needs
/root/reference); writes softdtw.npz next to this file."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

# (B, N, M, d, gamma, bandwidth, scale): inputs are N(0,1) * scale, float32
CASES = [(2, 37, 53, 8, 0.1, 0, 1.0), (1, 40, 40, 8, 1.0, 5, 1.0), (2, 33, 70, 16, 0.1, 0, 0.3), (1, 48, 45, 8, 0.1, 12, 1.0)]


def _identity_jit(*args, **kwargs):
    if len(args) == 1 and callable(args[0]) and not kwargs:       # @jit
        return args[0]
    return lambda fn: fn                                           # @jit(nopython=True)


def import_reference():
    numba, cuda = types.ModuleType("numba"), types.ModuleType("numba.cuda")
    numba.jit = cuda.jit = _identity_jit
    numba.cuda = cuda
    sys.modules["numba"], sys.modules["numba.cuda"] = numba, cuda
    sys.path.insert(0, "/root/reference")
    import soft_dtw_cuda as ref  # noqa
    return ref


def main():
    ref = import_reference()
    g = torch.Generator().manual_seed(2025)
    out = dict(cases=np.array(CASES, dtype=np.float64))
    for n, (B, N, M, d, gamma, bw, scale) in enumerate(CASES):
        x = torch.randn(B, N, d, generator=g) * scale
        y = torch.randn(B, M, d, generator=g) * scale
        D = ref.SoftDTW._euclidean_dist_func(x, y).requires_grad_(True)
        value = ref._SoftDTW.apply(D, gamma, float(bw))
        value.sum().backward()
        out[f"x{n}"], out[f"y{n}"] = x.numpy(), y.numpy()
        out[f"value{n}"], out[f"dD{n}"] = value.detach().numpy(), D.grad.numpy()
        print("case", n, CASES[n], "values", value.detach().numpy())
    B, N, d = 2, 24, 8
    x = torch.randn(B, N, d, generator=g).requires_grad_(True)
    y = torch.randn(B, N, d, generator=g)
    value = ref.SoftDTW(False, gamma=0.1, normalize=True)(x, y)
    value.sum().backward()
    out.update(norm_x=x.detach().numpy(), norm_y=y.numpy(), norm_value=value.detach().numpy(), norm_dX=x.grad.numpy())
    print("normalize", value.detach().numpy())
    path = os.path.join(HERE, "softdtw.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
