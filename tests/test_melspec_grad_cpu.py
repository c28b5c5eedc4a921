"""CPU checks of the log-mel backward's fp64 restatement (melspec_grad_ref.py) and of its plan (t2_melspec_grad_plan).

The restatement is held to torch autograd where both are defined, to central finite differences at the reflected edges and
the mirror points, and to the zero rule at digital silence, where autograd yields NaN: that case is why the rule exists."""
import pytest
import torch

import melspec_grad_ref as G
import melspec_ref as M


def _basis(name):
    from tacotron2_subword_amd import stft as S
    N, hop, win, n_mels = M.CONFIGS[name]
    fwd = S.STFT(N, hop, win).forward_basis[:, 0, :].clone()
    melb = torch.from_numpy(S.mel_filterbank(22050, N, n_mels, 0.0, 8000.0))
    return N, hop, n_mels, fwd, melb


def _convs(N, hop):
    return ((N // 2, 0.0), ((N - hop) // 2, 1e-9))


@pytest.mark.parametrize("name", ["small", "short_window"])
def test_explicit_backward_equals_autograd_fp64(name):
    N, hop, n_mels, fwd, melb = _basis(name)
    for pad, eps in _convs(N, hop):
        n = 9 * hop + hop // 3
        lens = [n, n - hop - 7, pad + 1 + hop]
        x = M.signal(3, n)
        g = G.upstream(3, n_mels, M.frames(n, N, hop, pad))
        ref = G.backward64(x, fwd, melb, N, hop, pad, g, eps, lengths=lens)
        assert ref["clipped"] == 0 and ref["min_mag"] > 0          # neither rule differs from torch here
        auto = G.autograd(x, fwd, melb, N, hop, pad, g, eps, lengths=lens)
        err = max(G.rel_err(ref["dx"], auto))
        print(f"{name} pad={pad}: explicit against autograd {err:.2e}, min mel {ref['min_mel']:.2e}, min mag {ref['min_mag']:.2e}")
        assert err <= 1e-10
        for b, L in enumerate(lens):
            assert bool((ref["dx"][b, L:] == 0).all()) and float(ref["dx"][b, :L].abs().max()) > 0


def test_finite_differences_at_edges_and_mirror_points():
    N, hop, n_mels, fwd, melb = _basis("small")
    for pad, eps in _convs(N, hop):
        L = 10 * hop + 5
        x = M.signal(1, L).double()
        nf = M.frames(L, N, hop, pad)
        g = G.upstream(1, n_mels, nf).double()
        dx = G.backward64(x, fwd, melb, N, hop, pad, g, eps)["dx"][0]

        def loss(v):
            re, im = G.forward64(v, fwd, N, hop, pad)
            s = melb.double() @ torch.sqrt(re ** 2 + im ** 2 + eps)
            assert float(s.min()) > 1e-5
            return float((torch.log(s) * g[0]).sum())

        gen = torch.Generator().manual_seed(3)
        inner = torch.randint(pad + 1, L - 1 - pad, (6,), generator=gen).tolist()
        spots = [0, L - 1, 1, pad // 2, pad, L - 2, L - 1 - pad // 2, L - 1 - pad] + inner   # mirror points, both reflected edges, interior
        h, scale, worst = 1e-6, float(dx.abs().max()), 0.0
        for i in spots:
            up, dn = x[0].clone(), x[0].clone()
            up[i] += h
            dn[i] -= h
            fd = (loss(up) - loss(dn)) / (2 * h)
            worst = max(worst, abs(fd - float(dx[i])) / scale)
        print(f"pad={pad}: {len(spots)} positions, worst |fd - dx| / max|dx| = {worst:.2e}")
        # central differences: h^2 * f''' / 6 truncation and 2^-53 * |loss| / h rounding, both far below 1e-6 of the scale here
        assert worst <= 1e-6


def test_silence_zero_rule_against_torch_nan():
    N, hop, n_mels, fwd, melb = _basis("small")
    pad, n = N // 2, 160
    x = G.silence_signal(N, hop, n)
    nf = M.frames(n, N, hop, pad)
    g = G.upstream(1, n_mels, nf)
    auto = G.autograd(x, fwd, melb, N, hop, pad, g, 0.0)
    nans = int(torch.isnan(auto).sum())
    print(f"torch autograd at five silent hops: {nans} NaN of {n} input gradients")
    assert nans > 0                                               # 0 * inf in sqrt's backward: the reason for the rule
    ref = G.backward64(x, fwd, melb, N, hop, pad, g, 0.0)
    dx = ref["dx"]
    assert torch.isfinite(dx).all() and ref["min_mag"] == 0.0 and ref["clipped"] > 0
    re, im = G.forward64(x[0], fwd, N, hop, pad)
    silent = ((re ** 2 + im ** 2).sum(0) == 0)
    n_silent = int(silent.sum())
    assert n_silent == 4 and bool(silent[:n_silent].all())        # frames 0..3 see zeros only; frame 4 starts at sample 2*hop
    only_silent = (n_silent * hop - pad)                           # samples below the first non-silent frame's start
    assert only_silent == 32 and bool((dx[0, :only_silent] == 0).all()) and float(dx[0, only_silent:].abs().max()) > 0
    g0 = g.clone()
    g0[:, :, :n_silent] = 0
    want = G.autograd(x, fwd, melb, N, hop, pad, g0, 0.0, mag_floor=1e-30)
    assert torch.isfinite(want).all()
    assert max(G.rel_err(dx, want)) <= 1e-10


def test_grad_plan_sizes_and_refusals():
    from tacotron2_subword_amd import _lib as L
    N, hop, _, n_mels = M.CONFIGS["default"]
    p = L.melspec_grad_plan(N, hop, N // 2, n_mels, 8192, 16)
    assert (p.bins, p.passes, p.row_tiles, p.overlap, p.nf_max) == (513, 9, 3, 4, 33)
    assert (p.grid_x, p.grid_y, p.grid_z) == (2, 9, 16) and (p.fold_grid_x, p.fold_grid_y) == (2, 1)
    assert p.melt_floats == 33 * 3 * 1024 and p.basis_floats == L.stft_plan(N, hop).inv_floats == 8 * 33 * 4 * 1024
    assert p.packed_bytes == 4 * (p.melt_floats + p.basis_floats)
    assert p.dz_floats == 2 * 16 * 513 * 33 and p.dxpad_floats == 16 * (8192 + 1024) and p.workspace_floats == p.dz_floats + p.dxpad_floats
    q = L.melspec_grad_plan(N, hop, (N - hop) // 2, n_mels, 8192, 16)       # the HiFi-GAN training segment: 32 frames, one tile per item
    assert q.nf_max == 32 and (q.grid_x, q.grid_y, q.grid_z) == (1, 9, 16) and q.dxpad_floats == 16 * (8192 + 768)
    with pytest.raises(RuntimeError, match=r"filter_length=1024 is not a multiple of hop_length=300"):
        L.melspec_grad_plan(1024, 300, 512, 80, 8192, 1)
    with pytest.raises(RuntimeError, match=r"hop_length=8 is 128 overlaps, at most 64"):
        L.melspec_grad_plan(1024, 8, 512, 80, 8192, 1)
    assert L.melspec_plan(1024, 300, 512, 80, 8192, 1).nf_max == 28             # the forward's own limits are unchanged
