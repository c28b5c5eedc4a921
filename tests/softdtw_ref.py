"""Soft-DTW restated for the tests: the recurrence of the reference's soft_dtw_cuda.py (forward :185-206, backward
:209-239) for ONE pair, vectorised along anti-diagonals with numpy.  dtype=np.float64 is the yardstick; dtype=np.float32
does the arithmetic of the reference's GPU kernel (:34-111: float32 throughout, r = -R * (1/gamma)) and serves as the
measure of what float32 can deliver on the same inputs."""
import numpy as np


def sqdist(x, y, dtype=np.float64):
    """D[i,j] = sum_c (x[i,c] - y[j,c])^2, c ascending."""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    D = np.zeros((x.shape[0], y.shape[0]), dtype)
    for c in range(x.shape[1]):
        df = x[:, c][:, None] - y[:, c][None, :]
        D += df * df
    return D


def _diagonal(s, N, M, bandwidth):
    """1-based (i, j) of the in-band cells with i + j = s."""
    i = np.arange(max(1, s - M), min(N, s - 1) + 1)
    j = s - i
    if bandwidth > 0:
        keep = np.abs(i - j) <= bandwidth
        i, j = i[keep], j[keep]
    return i, j


def forward(D, gamma, bandwidth=0.0, dtype=np.float64):
    """The padded R, [N+2, M+2]; the value of the pair is R[N, M]."""
    D = np.asarray(D, dtype)
    N, M = D.shape
    g, ig = dtype(gamma), dtype(1.0) / dtype(gamma)
    R = np.full((N + 2, M + 2), np.inf, dtype)
    R[0, 0] = 0
    with np.errstate(all="ignore"):
        for s in range(2, N + M + 1):
            i, j = _diagonal(s, N, M, bandwidth)
            if i.size == 0:
                continue
            r0, r1, r2 = -R[i - 1, j - 1] * ig, -R[i - 1, j] * ig, -R[i, j - 1] * ig
            rmax = np.maximum(np.maximum(r0, r1), r2)
            rsum = (np.exp(r0 - rmax) + np.exp(r1 - rmax)) + np.exp(r2 - rmax)
            R[i, j] = D[i - 1, j - 1] + (-g * (np.log(rsum) + rmax))
    return R


def backward(D, R, gamma, bandwidth=0.0, dtype=np.float64):
    """E = d R[N,M] / d D, [N, M], from the padded R of forward() (not modified)."""
    D = np.asarray(D, dtype)
    N, M = D.shape
    ig = dtype(1.0) / dtype(gamma)
    R = np.array(R, dtype)
    Dp = np.zeros((N + 2, M + 2), dtype)
    Dp[1:N + 1, 1:M + 1] = D
    E = np.zeros((N + 2, M + 2), dtype)
    E[-1, -1] = 1
    R[:, -1] = -np.inf
    R[-1, :] = -np.inf
    R[-1, -1] = R[-2, -2]
    with np.errstate(all="ignore"):
        for s in range(N + M, 1, -1):
            ia, ja = _diagonal(s, N, M, 0.0)                      # the reference turns infinities over before its band test
            inf = np.isinf(R[ia, ja])
            R[ia[inf], ja[inf]] = -np.inf
            i, j = _diagonal(s, N, M, bandwidth)
            if i.size == 0:
                continue
            a = np.exp(((R[i + 1, j] - R[i, j]) - Dp[i + 1, j]) * ig)
            b = np.exp(((R[i, j + 1] - R[i, j]) - Dp[i, j + 1]) * ig)
            c = np.exp(((R[i + 1, j + 1] - R[i, j]) - Dp[i + 1, j + 1]) * ig)
            E[i, j] = (E[i + 1, j] * a + E[i, j + 1] * b) + E[i + 1, j + 1] * c
    return E[1:N + 1, 1:M + 1]


def dist_backward(x, y, E, dtype=np.float64):
    """(dX, dY) of sum(E * sqdist(x, y)) with E held fixed: 2 sum_j E_ij (x_i - y_j), -2 sum_i E_ij (x_i - y_j)."""
    x, y, E = np.asarray(x, dtype), np.asarray(y, dtype), np.asarray(E, dtype)
    dX = 2 * (E.sum(1, dtype=dtype)[:, None] * x - E @ y)
    dY = -2 * (E.T @ x - E.sum(0, dtype=dtype)[:, None] * y)
    return dX.astype(dtype), dY.astype(dtype)


def pair(x, y, gamma, bandwidth=0.0, dtype=np.float64, D=None):
    """Everything the tests compare for one pair: dict(D, R [N,M] unpadded, value, E, dX, dY)."""
    D = sqdist(x, y, dtype) if D is None else np.asarray(D, dtype)
    Rp = forward(D, gamma, bandwidth, dtype)
    N, M = D.shape
    E = backward(D, Rp, gamma, bandwidth, dtype)
    out = dict(D=D, R=Rp[1:N + 1, 1:M + 1], value=Rp[N, M], E=E)
    if x is not None:
        out["dX"], out["dY"] = dist_backward(x, y, E, dtype)
    return out
