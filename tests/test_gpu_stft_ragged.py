"""GPU checks of the STFT kernels and the vocoder's bias remover on padded batches with per-item counts (csrc/stft.hip,
`lengths=`).

The contract is bit equality with the item run alone through the unchanged equal-length calls, which tests/test_gpu_stft.py
pins to fp64 and to the reference's recording; behind an item's count the outputs are exact zeros and what the inputs hold
there (NaN here) is never read.  The counts probe the full row, the 32-frame tile edge (and one past it, for the synthesis),
the shortest row the reflect padding takes and the one below it.  Against fp64 the bounds are those of
test_analysis_vs_fp64 and test_synthesis_vs_fp64."""
import numpy as np
import pytest
import torch

import stft_ref as R
import test_gpu_stft as TS

pytestmark = pytest.mark.gpu

TILE = TS.TILE
NAN = float("nan")
WANT = ("re", "im", "mag", "phase")


def _S():
    return TS._S()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _wave(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    gain = (1.0 + 0.25 * torch.arange(B, dtype=torch.float64)).view(B, 1)
    return (gain * (0.4 * torch.randn(B, n, generator=g, dtype=torch.float64) + 0.2 * torch.sin(0.05 * t))).float()


def _nan_behind(t, counts):
    t = t.clone()
    for b, n in enumerate(counts):
        t[b, ..., n:] = NAN
    return t


def _sample_counts(N, hop):
    """the full row (two frame tiles), a count whose frames end at the tile edge, the shortest row reflect padding takes, one less"""
    n = 40 * hop + 7
    return n, [n, (TILE - 1) * hop + hop // 3, N // 2 + 1, N // 2]


@pytest.mark.parametrize("name", ["default", "small"])
def test_analysis_same_bits_as_alone(name):
    c = TS._cfg(name)
    N, hop = c["N"], c["hop"]
    n, counts = _sample_counts(N, hop)
    assert 1 + counts[1] // hop == TILE
    x = _wave(4, n, 3)
    xd = _nan_behind(x, counts).cuda()
    *planes, fl = _S().analysis(xd, c["packed"], N, hop, want=WANT, lengths=_i32(counts))
    torch.cuda.synchronize()
    nfs = [1 + m // hop for m in counts[:3]] + [0]
    assert fl.dtype == torch.int32 and fl.tolist() == nfs
    for b, (m, nf) in enumerate(zip(counts, nfs)):
        if nf:
            alone = _S().analysis(x[b:b + 1, :m].contiguous().cuda(), c["packed"], N, hop, want=WANT)
        for i, key in enumerate(WANT):
            got = planes[i]
            assert got.shape == (4, N // 2 + 1, 1 + n // hop)
            if nf:
                assert torch.equal(got[b:b + 1, :, :nf], alone[i]), (name, b, key)
                assert float(alone[0].abs().max()) > 0.1
            assert float(got[b, :, nf:].abs().sum()) == 0.0, (name, b, key)      # zero behind the frames, the whole N/2 row
    # as Python ints: the same bits; the N/2 row raises in the words the analysis uses for a short signal
    as_list = _S().analysis(xd[:3].contiguous(), c["packed"], N, hop, want=WANT, lengths=counts[:3])
    for i in range(4):
        assert torch.equal(as_list[i], planes[i][:3])
    assert as_list[4].tolist() == nfs[:3]
    with pytest.raises(RuntimeError, match=rf"Padding size should be less than.*item 3 of {N // 2} samples"):
        _S().analysis(xd, c["packed"], N, hop, lengths=counts)
    with pytest.raises(RuntimeError, match=rf"lengths\[0\]={n + 1}"):
        _S().analysis(xd, c["packed"], N, hop, lengths=[n + 1] + counts[1:])
    # on the device a count past the row is the row, a negative one is no row
    re_w, fl_w = _S().analysis(x.cuda(), c["packed"], N, hop, want=("re",), lengths=_i32([n + 5, -1, counts[2], counts[3]]))
    assert fl_w.tolist() == [1 + n // hop, 0, nfs[2], 0]
    assert torch.equal(re_w[0], _S().analysis(x[:1].cuda(), c["packed"], N, hop, want=("re",))[0][0]) and float(re_w[1].abs().sum()) == 0.0


def _planes4(bins, nf, mode):
    parts = [TS._planes(1, bins, nf, mode, seed=10 + b) for b in range(4)]
    a = torch.cat([p[0] * (1.0 + 0.25 * b) for b, p in enumerate(parts)])
    b_ = torch.cat([p[1] for p in parts])
    return a, b_, parts[0][2]


@pytest.mark.parametrize("windowed", [True, False], ids=["windowed", "plain"])
@pytest.mark.parametrize("mode", [0, 1], ids=["polar", "denoise"])
@pytest.mark.parametrize("name", ["default", "small"])
def test_synthesis_same_bits_as_alone(name, mode, windowed):
    c = TS._cfg(name)
    N, hop = c["N"], c["hop"]
    bins, nf = N // 2 + 1, TILE + 5
    counts = [nf, TILE + 1, TILE, 1]
    a, b_, bias = _planes4(bins, nf, mode)
    kw = dict(mode=mode, bias=None if bias is None else bias.cuda(), strength=0.9, windowed=windowed)
    ad, bd = _nan_behind(a, counts).cuda(), _nan_behind(b_, counts).cuda()
    y, sl = _S().synthesis(ad, bd, c["packed"], N, hop, lengths=_i32(counts), **kw)
    torch.cuda.synchronize()
    assert y.shape == (4, 1, hop * (nf - 1)) and torch.isfinite(y).all()
    assert sl.dtype == torch.int32 and sl.tolist() == [hop * (m - 1) for m in counts]
    for b, m in enumerate(counts):
        alone = _S().synthesis(a[b:b + 1, :, :m].contiguous().cuda(), b_[b:b + 1, :, :m].contiguous().cuda(), c["packed"], N, hop, **kw)
        assert alone.shape == (1, 1, hop * (m - 1))
        assert torch.equal(y[b:b + 1, :, :hop * (m - 1)], alone), (name, mode, windowed, b)
        assert float(y[b, :, hop * (m - 1):].abs().sum()) == 0.0
        assert m == 1 or float(alone.abs().max()) > 1e-2           # a signal, not rounding noise (the unwindowed sum is small)
    y_list, sl_list = _S().synthesis(ad, bd, c["packed"], N, hop, lengths=counts, **kw)
    assert torch.equal(y_list, y) and torch.equal(sl_list, sl)
    with pytest.raises(RuntimeError, match=r"no frames.*lengths\[3\]=0"):
        _S().synthesis(ad, bd, c["packed"], N, hop, lengths=[nf, TILE + 1, TILE, 0], **kw)
    with pytest.raises(RuntimeError, match=rf"lengths\[1\]={nf + 1}"):
        _S().synthesis(ad, bd, c["packed"], N, hop, lengths=[nf, nf + 1, TILE, 1], **kw)
    # on the device a count below 1 gives an all-zero row of length 0, one past the planes is the planes
    y_w, sl_w = _S().synthesis(_nan_behind(a, [nf, 0, 0, 1]).cuda(), _nan_behind(b_, [nf, 0, 0, 1]).cuda(), c["packed"], N, hop,
                               lengths=_i32([nf + 9, 0, -2, 1]), **kw)
    assert sl_w.tolist() == [hop * (nf - 1), 0, 0, 0] and torch.equal(y_w[0], y[0]) and float(y_w[1:].abs().sum()) == 0.0


def test_bias_remover_same_bits_as_alone():
    from tacotron2_subword_amd.bias_remover import hifiganBiasRemover
    br = hifiganBiasRemover(R.stub_model).cuda()
    N, hop = 1024, 256
    n = 40 * hop + 7
    counts = [n, (TILE - 1) * hop + 100, N // 2 + 1]
    x = _wave(3, n, 5)
    y, sl = br(_nan_behind(x, counts).cuda(), 0.9, lengths=_i32(counts))
    torch.cuda.synchronize()
    assert y.shape == (3, 1, hop * (n // hop)) and torch.isfinite(y).all()
    assert sl.dtype == torch.int32 and sl.tolist() == [hop * (m // hop) for m in counts]
    for b, m in enumerate(counts):
        alone = br(x[b:b + 1, :m].contiguous().cuda(), 0.9)
        assert isinstance(alone, torch.Tensor) and alone.shape == (1, 1, hop * (m // hop))      # without lengths: what it returns today
        assert torch.equal(y[b:b + 1, :, :hop * (m // hop)], alone), b
        assert float(y[b, :, hop * (m // hop):].abs().sum()) == 0.0
        assert float(alone.abs().max()) > 0.1
    y_list, sl_list = br(_nan_behind(x, counts).cuda(), 0.9, lengths=counts)
    assert torch.equal(y_list, y) and torch.equal(sl_list, sl)
    # the vocoder's own output form: the generator's sample counts feed the remover as they are
    assert torch.equal(br(x.cuda(), 0.9, lengths=_i32([n] * 3))[0], br(x.cuda(), 0.9))


def test_ragged_analysis_vs_fp64():
    c = TS._cfg("default")
    N, hop = c["N"], c["hop"]
    n, counts = _sample_counts(N, hop)
    x = _wave(4, n, 7)
    re, im, fl = _S().analysis(_nan_behind(x, counts).cuda(), c["packed"], N, hop, lengths=_i32(counts))
    for b in range(3):
        m, nf = counts[b], 1 + counts[b] // hop
        re64, im64, (sre, sim) = R.analysis64(x[b:b + 1, :m], c["fwd"], N, hop)
        TS._check(f"ragged analysis item {b} n={m} re", re[b:b + 1, :, :nf].cpu(), re64, 1e-6 * sre + 1e-7)
        TS._check(f"ragged analysis item {b} n={m} im", im[b:b + 1, :, :nf].cpu(), im64, 1e-6 * sim + 1e-7)


@pytest.mark.parametrize("mode", [0, 1], ids=["polar", "denoise"])
def test_ragged_synthesis_vs_fp64(mode):
    from tacotron2_subword_amd.audio_processing import window_sumsquare
    c = TS._cfg("default")
    N, hop, win = c["N"], c["hop"], c["win"]
    bins, nf = N // 2 + 1, TILE + 5
    counts = [nf, TILE + 1, TILE, 2]
    a, b_, bias = _planes4(bins, nf, mode)
    y, _ = _S().synthesis(_nan_behind(a, counts).cuda(), _nan_behind(b_, counts).cuda(), c["packed"], N, hop, mode=mode,
                          bias=None if bias is None else bias.cuda(), strength=0.9, lengths=_i32(counts))
    for b, m in enumerate(counts):
        env = window_sumsquare("hann", m, hop_length=hop, win_length=win, n_fft=N, dtype=np.float32)
        X = TS._X64(a[b:b + 1, :, :m], b_[b:b + 1, :, :m], bias, 0.9, mode)
        ref = R.finish64(R.ola64(X, c["inv"], N, hop), env, N, hop)
        S = R.finish64(R.ola64(X.abs(), c["inv"].abs(), N, hop), env, N, hop)
        TS._check(f"ragged synthesis item {b} nf={m} mode={mode}", y[b:b + 1, :, :hop * (m - 1)].cpu(), ref, 2e-6 * S + 1e-7)


def test_surface():
    c = TS._cfg("small")
    N, hop = c["N"], c["hop"]
    x = _wave(2, 10 * hop, 1).cuda()
    out = _S().analysis(x, c["packed"], N, hop)
    assert len(out) == 2 and out[0].shape == (2, N // 2 + 1, 11)                 # without lengths: what it was
    y = _S().synthesis(out[0], out[1], c["packed"], N, hop, mode=1, bias=torch.zeros(N // 2 + 1, device="cuda"))
    assert isinstance(y, torch.Tensor) and y.shape == (2, 1, 10 * hop)
    with pytest.raises(RuntimeError, match="int64"):
        _S().analysis(x, c["packed"], N, hop, lengths=torch.tensor([100, 100], device="cuda"))
    with pytest.raises(RuntimeError, match=r"\(3,\)"):
        _S().analysis(x, c["packed"], N, hop, lengths=_i32([100, 100, 100]))
    with pytest.raises(RuntimeError, match="cpu"):
        _S().synthesis(out[0], out[1], c["packed"], N, hop, lengths=torch.tensor([5, 5], dtype=torch.int32))
