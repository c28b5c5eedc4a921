"""The one weight pack of the slab GEMM (csrc/slab_gemm.h, slab_pack in csrc/vocoder.hip), through every unit entry point
that writes it into the caller's packed_ws: weights are distinct integers in torch layout, and the buffer read back must
equal, element for element, the documented layout written out in numpy:

    packed[mtile][step][gate][pg][lane][i] = W[row = 32*mtile + (lane & 31) (+ gate * rows)][k = 16*chunk + 2*(4*pg + i) + (lane >> 5)][tap]

zero outside the matrix, step = chunk * taps + tap over segment 0, then the chunks of segment 1; the vocoder's transposed
conv has one such block per output phase.  The buffer is as long as the entry point's *_packed_floats query says.  The
layers' outputs are checked elsewhere (test_gpu_hifigan.py, test_gpu_waveglow*.py); here the time extent is a few samples."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -7.5                       # no weight has this value: what the pack must not leave behind, and must not write past its end


def _L():
    from tacotron2_subword_amd import _lib as L
    return L


def _arange(*shape):
    return np.arange(1, 1 + int(np.prod(shape)), dtype=np.float32).reshape(shape)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _zeros(*shape):
    return torch.zeros(*shape, device=DEV)


def _layout(rows, gates, segs):
    """segs: (K, taps, f) per segment, f(gate, row, k, tap) on index arrays that are inside the matrix."""
    mtiles = (rows + 31) // 32
    blocks = []
    for K, taps, f in segs:
        nch = (K + 15) // 16
        mt, c, j, g, pg, lane, i = np.meshgrid(np.arange(mtiles), np.arange(nch), np.arange(taps), np.arange(gates), np.arange(2), np.arange(64),
                                               np.arange(4), indexing="ij")
        row, k = 32 * mt + (lane & 31), 16 * c + 2 * (4 * pg + i) + (lane >> 5)
        inside = (row < rows) & (k < K)
        v = np.zeros(row.shape, dtype=np.float32)
        v[inside] = f(g[inside], row[inside], k[inside], j[inside])
        blocks.append(v.reshape(mtiles, nch * taps, gates, 2, 64, 4))
    return np.concatenate(blocks, axis=1).reshape(-1)


def _same(tag, packed, want, query):
    torch.cuda.synchronize()
    got = packed.cpu().numpy()
    assert want.size == query, (tag, want.size, query)
    assert np.count_nonzero(want) > 0
    assert np.array_equal(got[:want.size], want), tag
    assert np.all(got[want.size:] == SENTINEL), tag + ": written past the pack"


def _buffer(n, slack=64):
    return torch.full((n + slack,), SENTINEL, device=DEV)


# ------------------------------------------------------------------------------------------------------------------ vocoder
@pytest.mark.parametrize("Cin, Cout, k", [(24, 40, 3), (8, 8, 11)])      # ragged 16-channel chunk and ragged 32-row tile; eleven taps
def test_conv1d_pack(Cin, Cout, k):
    L = _L()
    Lt = 8
    w = _arange(Cout, Cin, k)
    query = L.lib().t2_vocoder_packed_floats(Cin, Cout, k, 0)
    packed = _buffer(query)
    held = [_zeros(1, Cin, Lt), _dev(w), _zeros(1, Cout, Lt)]
    a = L.VocoderConvArgs(1, Cin, Cout, Lt, k, 1, 0, L.ptr(held[0]), L.ptr(held[1]), L.ptr(None), L.ptr(None), L.ptr(held[2]), L.ptr(packed), 0.1, 0, 1.0)
    L.check(L.lib().t2_vocoder_conv1d(C.byref(a), L.stream()))
    _same("conv1d", packed, _layout(Cout, 1, [(Cin, k, lambda g, r, kk, j: w[r, kk, j])]), query)


@pytest.mark.parametrize("Cin, Cout, u", [(16, 8, 2), (24, 40, 8)])       # at u = 8, pad = 4: phase and (phase + pad) % u both non-trivial
def test_conv_transpose1d_pack(Cin, Cout, u):
    L = _L()
    Lt, k = 4, 2 * u
    pad = (k - u) // 2
    w = _arange(Cin, Cout, k)
    query = L.lib().t2_vocoder_packed_floats(Cin, Cout, k, u)
    packed = _buffer(query)
    held = [_zeros(1, Cin, Lt), _dev(w), _zeros(1, Cout, Lt * u)]
    a = L.VocoderConvArgs(1, Cin, Cout, Lt, k, 1, u, L.ptr(held[0]), L.ptr(held[1]), L.ptr(None), L.ptr(None), L.ptr(held[2]), L.ptr(packed), 0.1, 0, 1.0)
    L.check(L.lib().t2_vocoder_conv_transpose1d(C.byref(a), L.stream()))
    # phase r of the output reads taps (r + pad) % u + j*u, j = 0, 1
    want = np.concatenate([_layout(Cout, 1, [(Cin, 2, lambda g, r, kk, j, ph=ph: w[kk, r, (ph + pad) % u + j * u])]) for ph in range(u)])
    _same("conv_transpose1d", packed, want, query)


# ------------------------------------------------------------------------------------------------------------------ WaveGlow, forward
@pytest.mark.parametrize("nc, n_cond", [(24, 80), (8, 8)])               # two gates, two segments
def test_gated_pack(nc, n_cond):
    L = _L()
    Lt = 8
    w_in, w_cond = _arange(2 * nc, nc, 3), _arange(2 * nc, n_cond) + 100000
    query = L.lib().t2_waveglow_packed_floats(L.WAVEGLOW_GATED, nc, nc, n_cond)
    packed = _buffer(query)
    held = [_zeros(1, nc, Lt), _zeros(1, n_cond, Lt), _dev(w_in), _zeros(2 * nc), _dev(w_cond), _zeros(2 * nc), packed, _zeros(1, nc, Lt)]
    a = L.WaveglowGatedArgs(1, nc, n_cond, Lt, 1, 0, *[L.ptr(v) for v in held])
    L.check(L.lib().t2_waveglow_gated_conv(C.byref(a), L.stream()))
    want = _layout(nc, 2, [(nc, 3, lambda g, r, kk, j: w_in[g * nc + r, kk, j]), (n_cond, 1, lambda g, r, kk, j: w_cond[g * nc + r, kk])])
    _same("gated", packed, want, query)


@pytest.mark.parametrize("last", [0, 1])
def test_res_skip_pack(last):
    L = _L()
    nc, Lt = 24, 8
    rows = nc if last else 2 * nc
    w = _arange(rows, nc)
    query = L.lib().t2_waveglow_packed_floats(L.WAVEGLOW_RES_SKIP, rows, nc, 0)
    packed = _buffer(query)
    held = [_zeros(1, nc, Lt), _dev(w), _zeros(rows), packed, _zeros(1, nc, Lt), _zeros(1, nc, Lt)]
    a = L.WaveglowResSkipArgs(1, nc, Lt, 1, last, *[L.ptr(v) for v in held])
    L.check(L.lib().t2_waveglow_res_skip(C.byref(a), L.stream()))
    _same("res_skip", packed, _layout(rows, 1, [(nc, 1, lambda g, r, kk, j: w[r, kk])]), query)


def test_upsample_pack():
    # row = channel * 256 + phase reads w[ci][channel][phase + 256 * tap]: the row address splits
    L = _L()
    n_mel, T, G = 8, 1, 8
    w = _arange(n_mel, n_mel, 1024)
    query = L.lib().t2_waveglow_packed_floats(L.WAVEGLOW_UPSAMPLE, n_mel, n_mel, 0)
    packed = _buffer(query)
    held = [_zeros(1, n_mel, T), _dev(w), _zeros(n_mel), packed, _zeros(1, n_mel * G, T * 256 // G)]
    a = L.WaveglowUpsampleArgs(1, n_mel, T, G, *[L.ptr(v) for v in held])
    L.check(L.lib().t2_waveglow_upsample(C.byref(a), L.stream()))
    _same("upsample", packed, _layout(n_mel * 256, 1, [(n_mel, 4, lambda g, r, kk, j: w[kk, r // 256, r % 256 + 256 * j])]), query)


# ------------------------------------------------------------------------------------------------------------------ WaveGlow, backward
@pytest.mark.parametrize("last", [0, 1])
def test_gate_backward_pack(last):
    # d_acts = W_rs^T [dx; d_out]: row c, k = r reads w_rs[r][c]; the rows of `out` are a second segment unless the layer is the last
    L = _L()
    nc, Lt = 24, 8
    rows = nc if last else 2 * nc
    w = _arange(rows, nc)
    half = L.lib().t2_waveglow_packed_floats(L.WAVEGLOW_RES_SKIP, nc, nc, 0)
    query = half if last else 2 * half                       # t2amd.h: the entry point takes 2 * half floats and fills what the layer has
    packed = _buffer(query, slack=64 + half)
    held = [None if last else _zeros(1, nc, Lt), _zeros(1, nc, Lt), _dev(w), _zeros(1, nc, Lt), _zeros(1, nc, Lt), packed, _zeros(1, 2 * nc, Lt),
            _zeros(1, nc, Lt)]
    a = L.WaveglowGateBackwardArgs(1, nc, Lt, last, *[L.ptr(v) for v in held])
    L.check(L.lib().t2_waveglow_gate_backward(C.byref(a), L.stream()))
    segs = [(nc, 1, lambda g, r, kk, j: w[kk, r])]
    if not last:
        segs.append((nc, 1, lambda g, r, kk, j: w[nc + kk, r]))
    _same("gate backward", packed, _layout(nc, 1, segs), query)


def test_conv_backward_pack():
    # conv^T: row c, k = r, tap j reads w_in[r][c][2 - j] (flipped taps, a negative tap stride); then W_cond^T: row m, k = r
    L = _L()
    nc, n_cond, Lt, d = 24, 80, 8, 2
    w_in, w_cond = _arange(2 * nc, nc, 3), _arange(2 * nc, n_cond) + 100000
    query = L.lib().t2_waveglow_conv_backward_packed_floats(nc, n_cond)
    packed = _buffer(query)
    held = [_zeros(1, 2 * nc, Lt), _dev(w_in), _dev(w_cond), packed, _zeros(1, nc, Lt), _zeros(1, n_cond, Lt)]
    a = L.WaveglowConvBackwardArgs(1, nc, n_cond, Lt, d, 1, 1, *[L.ptr(v) for v in held])
    L.check(L.lib().t2_waveglow_conv_backward(C.byref(a), L.stream()))
    want = np.concatenate([_layout(nc, 1, [(2 * nc, 3, lambda g, r, kk, j: w_in[kk, r, 2 - j])]),
                           _layout(n_cond, 1, [(2 * nc, 1, lambda g, r, kk, j: w_cond[kk, r])])])
    _same("conv backward", packed, want, query)
