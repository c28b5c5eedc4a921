"""CPU-only soft-DTW checks: the fp64 restatement (tests/softdtw_ref.py) reproduces the vectors recorded from the
reference (tests/golden/make_golden_softdtw.py), t2_softdtw_plan partitions every N as documented and refuses what the
kernels cannot take, and the module refuses the CPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import softdtw_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "softdtw.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_restatement_reproduces_the_reference(golden):
    """Values to a relative 1e-6.  E within 2e-3 absolute: the reference rounds R to float32 between its two passes,
    which moves E by up to 5.3e-4 against fp64 on these cases; the bound is about 4 times that."""
    for n, (B, N, M, d, gamma, bw, scale) in enumerate(golden["cases"]):
        for b in range(int(B)):
            r = S.pair(golden[f"x{n}"][b], golden[f"y{n}"][b], gamma, bw)
            want = float(golden[f"value{n}"][b])
            assert abs(r["value"] - want) <= 1e-6 * abs(want), (n, b)
            err = np.abs(r["E"] - golden[f"dD{n}"][b]).max()
            print(f"case {n} pair {b}: value {r['value']:.6f} vs {want:.6f}, max |E - dD| = {err:.2e}")
            assert err <= 2e-3, (n, b)


def test_restatement_reproduces_the_normalized_case(golden):
    x, y = golden["norm_x"], golden["norm_y"]
    for b in range(x.shape[0]):
        xy, xx, yy = S.pair(x[b], y[b], 0.1), S.pair(x[b], x[b], 0.1), S.pair(y[b], y[b], 0.1)
        value = xy["value"] - 0.5 * (xx["value"] + yy["value"])
        want = float(golden["norm_value"][b])
        assert abs(value - want) <= 1e-6 * max(abs(xy["value"]), abs(want))
        dX = xy["dX"] - 0.5 * (xx["dX"] + xx["dY"])
        # dX = sum_j E_ij * 2 (x_i - y_j): |x - y| <= 10 on N(0,1) inputs turns the 2e-3 on E into 24 * 2 * 10 * 2e-3 at the very most
        assert np.abs(dX - golden["norm_dX"][b]).max() <= 24 * 2 * 10 * 2e-3


def test_float32_mode_stays_float32(golden):
    r = S.pair(golden["x0"][0], golden["y0"][0], 0.1, 0.0, np.float32)
    assert all(r[k].dtype == np.float32 for k in ("D", "R", "E", "dX", "dY"))
    r64 = S.pair(golden["x0"][0], golden["y0"][0], 0.1, 0.0)
    assert 0 < np.abs(r["R"] - r64["R"]).max() < 1e-2


def _plan(B, N, M, gamma=1.0, need_grad=False):
    from tacotron2_subword_amd import _lib as L
    return L.softdtw_plan(B, N, M, gamma, need_grad)


# every N at which the partition changes: a further wave (64 -> 65, ...), the full workgroup, a further row per thread
PLAN_EDGES = [1, 2, 63, 64, 65, 128, 129, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050, 4095, 4096, 4097, 4100, 6000, 8191, 8192]


@pytest.mark.parametrize("N", PLAN_EDGES)
def test_plan_partition(N):
    B, M = 3, 77
    p = _plan(B, N, M)
    rpt = next(r for r in (1, 2, 4, 8) if r * 1024 >= N)           # the smallest rung of the ladder that fits 1024 threads
    owners = -(-N // rpt)
    assert p.rows_per_thread == rpt
    assert p.threads % 64 == 0 and 64 <= p.threads <= 1024
    assert p.threads * p.rows_per_thread >= N
    assert p.threads - 64 < owners <= p.threads                    # no idle wave
    assert p.passes == M + owners - 1                              # thread t starts t passes late and then does M columns
    assert p.d_floats == B * p.passes * p.threads * rpt
    assert p.r_floats == 0 and p.e_floats == 0                     # no gradient: O(N) state, nothing stored
    g = _plan(B, N, M, need_grad=True)
    assert (g.threads, g.rows_per_thread, g.passes, g.d_floats) == (p.threads, p.rows_per_thread, p.passes, p.d_floats)
    assert g.r_floats == g.d_floats and g.e_floats == B * N * M


def test_plan_refuses_what_the_kernels_cannot_take():
    from tacotron2_subword_amd import _lib as L
    info = L.SoftDtwPlanInfo()
    for args, word in (((1, 8193, 10, 1.0), b"8192"), ((1, 8192 + 500, 10, 1.0), b"8192"), ((1, 10, 8193, 1.0), b"8192"),
                       ((1, 10, 0, 1.0), b"at least 1"), ((1, 0, 10, 1.0), b"at least 1"), ((0, 10, 10, 1.0), b"at least 1"),
                       ((1, 10, 10, 0.0), b"gamma"), ((1, 10, 10, -0.5), b"gamma"), ((1, 10, 10, float("nan")), b"gamma")):
        B, N, M, gamma = args
        rc = L.lib().t2_softdtw_plan(B, N, M, gamma, 0, C.byref(info))
        assert rc != 0 and word in L.lib().t2_last_error(), (args, L.lib().t2_last_error())
    with pytest.raises(RuntimeError, match="8192"):
        _plan(1, 9000, 9000)
    assert _plan(1, 8192, 8192).rows_per_thread == 8


def test_entry_points_validate_before_touching_the_device():
    """Size and gamma errors come back from the working entry points too, without a GPU."""
    from tacotron2_subword_amd import _lib as L
    a = L.SoftDtwFwdArgs(1, 10, 10, 0.0, 0.0, None, None, None, None, None, None)
    assert L.lib().t2_softdtw_forward(C.byref(a), None) != 0 and b"gamma" in L.lib().t2_last_error()
    a = L.SoftDtwFwdArgs(1, 9000, 10, 1.0, 0.0, None, None, None, None, None, None)
    assert L.lib().t2_softdtw_forward(C.byref(a), None) != 0 and b"8192" in L.lib().t2_last_error()
    a = L.SoftDtwFwdArgs(1, 10, 10, 1.0, 0.0, None, None, None, None, None, None)
    assert L.lib().t2_softdtw_forward(C.byref(a), None) != 0 and b"exactly one of" in L.lib().t2_last_error()
    d = L.SoftDtwDistArgs(1, 10, 10, 0, None, None, None)
    assert L.lib().t2_softdtw_dist(C.byref(d), None) != 0 and b"d=0" in L.lib().t2_last_error()


def test_module_refuses_the_cpu():
    from tacotron2_subword_amd.soft_dtw_cuda import SoftDTW
    with pytest.raises(RuntimeError, match="no CPU"):
        SoftDTW(use_cuda=False)
    with pytest.raises(RuntimeError, match="GPU"):
        SoftDTW(use_cuda=True, gamma=0.1)(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3))
    m = SoftDTW(True, gamma=0.5, bandwidth=None)
    assert m.bandwidth == 0.0 and m.gamma == 0.5 and m.normalize is False
