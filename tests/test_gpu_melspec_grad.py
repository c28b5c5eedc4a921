"""GPU checks of the log-mel and STFT-analysis backward (csrc/melspec.hip melspec_grad_kernel, csrc/stft.hip
stft_analysis_backward) against the explicit fp64 backward of melspec_grad_ref.py.

Metric: e = max|dx - dx64| / max|dx64| per item.  Yardstick, measured and not invented: the same quantity for the fp32
torch-op statement of the formula under autograd on the CPU (e32), over every case of test_vs_fp64; the kernels must stay
within 4 x the largest e32.  The margin of 4 is for the summation order: an MFMA chain is a k-ordered fmaf chain whose error
grows linearly in K where torch's blocked sums grow slower (the forward's bound gives the same analysis a margin of 3).
Every comparison prints e_hip, e32 and their ratio.  Every case asserts that no fp64 mel is at the clip and that the
smallest magnitude is positive, so the two rules (clamp mask, zero rule) leave no element unpinned; the silence test is the
one place where they act."""
import pytest
import torch

import melspec_grad_ref as G
import melspec_ref as M

pytestmark = pytest.mark.gpu

TILE = 32
MARGIN = 4.0
_cache = {}


def _S():
    from tacotron2_subword_amd import stft as S
    return S


def _cfg(name):
    if name not in _cache:
        N, hop, win, n_mels = M.CONFIGS[name]
        m = _S().STFT(N, hop, win)
        fwd = m.forward_basis[:, 0, :].clone()
        melb = torch.from_numpy(_S().mel_filterbank(22050, N, n_mels, 0.0, 8000.0))
        _cache[name] = dict(N=N, hop=hop, win=win, n_mels=n_mels, fwd=fwd, melb=melb, stft=m.cuda(), melb_gpu=melb.cuda())
    return _cache[name]


def _conv(c, conv):
    """(pad, mag_eps): TacotronSTFT's convention, or utils.mel_spectrogram's."""
    return (c["N"] // 2, 0.0) if conv == "taco" else ((c["N"] - c["hop"]) // 2, 1e-9)


def _n_for_frames(c, conv, nf):
    """A length that is no multiple of hop and gives nf frames (test_gpu_melspec.py's, restated)."""
    return (nf - 1) * c["hop"] + c["hop"] // 3 if conv == "taco" else nf * c["hop"] + c["hop"] // 3


def _lengths(c, conv):
    return [_conv(c, conv)[0] + 1] + [_n_for_frames(c, conv, nf) for nf in (TILE - 1, TILE, TILE + 1)]


def _grad(c, x, conv, g, melb=None, lengths=None, time_major=False):
    """-> (mel, dx) of the differentiable log_mel on the GPU for the upstream gradient g [B, n_mels, nf]."""
    pad, eps = _conv(c, conv)
    xg = x.cuda().requires_grad_(True)
    mel, _ = _S().log_mel(xg, c["stft"], c["melb_gpu"] if melb is None else melb, lengths=lengths, pad=pad, mag_eps=eps, time_major=time_major,
                          differentiable=True)
    assert mel.grad_fn is not None
    gg = g.cuda()
    mel.backward(gg.transpose(1, 2) if time_major else gg)       # time-major: a non-contiguous upstream gradient
    return mel.detach(), xg.grad


def _reference(c, x, conv, g, melb=None, lengths=None):
    """fp64 explicit backward and the fp32 torch-op statement's error against it, per item."""
    pad, eps = _conv(c, conv)
    melb = c["melb"] if melb is None else melb
    ref = G.backward64(x, c["fwd"], melb, c["N"], c["hop"], pad, g, eps, lengths=lengths)
    e32 = G.rel_err(G.autograd(x, c["fwd"], melb, c["N"], c["hop"], pad, g, eps, lengths=lengths, dtype=torch.float32), ref["dx"])
    return ref, e32


@pytest.fixture(scope="module")
def cases():
    """Every case of test_vs_fp64, computed once and left unchanged: inputs, the fp64 gradient, e32; and the yardstick."""
    out = {}
    for name in M.CONFIGS:
        c = _cfg(name)
        for conv in ("taco", "hifigan"):
            pad, _ = _conv(c, conv)
            for B in (1, 3):
                for n in _lengths(c, conv):
                    x = M.signal(B, n)
                    g = G.upstream(B, c["n_mels"], M.frames(n, c["N"], c["hop"], pad))
                    ref, e32 = _reference(c, x, conv, g)
                    out[(name, conv, B, n)] = dict(x=x, g=g, ref=ref, e32=e32)
    yard = max(max(v["e32"]) for v in out.values())
    print(f"yardstick: largest e32 over {len(out)} cases {yard:.3e}; the kernels are held to {MARGIN:g} x that")
    return out, yard


def _check(tag, dx, ref, e32, yard):
    assert ref["clipped"] == 0 and ref["min_mag"] > 0, tag              # neither rule acts: no element is left unpinned
    assert torch.isfinite(dx).all(), tag
    e = G.rel_err(dx.cpu(), ref["dx"])
    print(f"{tag}: e_hip {max(e):.3e}  e32 {max(e32):.3e}  ratio {max(e) / max(e32):.2f}  e_hip / yardstick {max(e) / yard:.2f}  "
          f"min mel {ref['min_mel']:.2e}  min mag {ref['min_mag']:.2e}")
    assert max(e) <= MARGIN * yard, tag


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", ["small", "short_window", "nonpow2", "default"])
def test_vs_fp64(cases, name, B):
    table, yard = cases
    c = _cfg(name)
    for conv in ("taco", "hifigan"):
        pad, eps = _conv(c, conv)
        for n in _lengths(c, conv):
            k = table[(name, conv, B, n)]
            mel, dx = _grad(c, k["x"], conv, k["g"])
            plain, _ = _S().log_mel(k["x"].cuda(), c["stft"], c["melb_gpu"], pad=pad, mag_eps=eps)
            assert torch.equal(mel, plain)                               # the differentiable forward keeps the forward's bits
            assert dx.shape == k["x"].shape
            _check(f"{name} {conv} B={B} n={n} nf={M.frames(n, c['N'], c['hop'], pad)}", dx, k["ref"], k["e32"], yard)


@pytest.mark.parametrize("n_mels", [33, 128])
@pytest.mark.parametrize("name", ["short_window", "small"])
def test_row_and_bin_edges(cases, name, n_mels):
    _, yard = cases
    c = _cfg(name)
    bins = c["N"] // 2 + 1
    gen = torch.Generator().manual_seed(n_mels)
    melb = (torch.rand(n_mels, bins, generator=gen) * (0.5 + (torch.arange(n_mels) % 7).float()[:, None]) / bins).float()   # dense: every (row, bin) counts
    x = M.signal(2, 35 * c["hop"] + 5)
    for conv in ("taco", "hifigan"):
        pad, _ = _conv(c, conv)
        g = G.upstream(2, n_mels, M.frames(x.shape[1], c["N"], c["hop"], pad))
        ref, e32 = _reference(c, x, conv, g, melb=melb)
        _, dx = _grad(c, x, conv, g, melb=melb.cuda())
        _check(f"edges {name} n_mels={n_mels} {conv}", dx, ref, e32, yard)


@pytest.mark.parametrize("conv", ["taco", "hifigan"])
def test_ragged_bits_and_guards(cases, conv):
    _, yard = cases
    c = _cfg("default")
    N, hop, n_mels = c["N"], c["hop"], c["n_mels"]
    pad, _ = _conv(c, conv)
    n = _n_for_frames(c, conv, TILE + 3)
    lens = [n, n - hop - 7, pad + 1 + hop]
    nfs = [M.frames(v, N, hop, pad) for v in lens]
    assert nfs[0] > nfs[1] > TILE > nfs[2] >= 1                          # two frame tiles, two, one
    x = M.signal(3, n)
    g = G.upstream(3, n_mels, nfs[0])
    _, dx = _grad(c, x, conv, g, lengths=lens)
    _, dx_dev = _grad(c, x, conv, g, lengths=torch.tensor(lens, dtype=torch.int32).cuda())
    assert torch.equal(dx, dx_dev)                                       # ints or a device tensor
    assert torch.equal(_grad(c, x, conv, g, lengths=lens)[1], dx)        # two runs, the same bits
    for b in range(3):
        _, alone = _grad(c, x[b:b + 1, :lens[b]].contiguous(), conv, g[b:b + 1, :, :nfs[b]].contiguous())
        assert torch.equal(dx[b:b + 1, :lens[b]], alone), b              # an item in the batch has the bits of its run alone
        assert bool((dx[b, lens[b]:] == 0).all()) and float(dx[b, :lens[b]].abs().max()) > 0
    xn, gn = x.clone(), g.clone()
    for b in range(3):                                                   # NaN where nothing may be read
        xn[b, lens[b]:] = float("nan")
        gn[b, :, nfs[b]:] = float("nan")
    assert torch.equal(_grad(c, xn, conv, gn, lengths=lens)[1], dx)
    mel_tm, dx_tm = _grad(c, x, conv, g, lengths=lens, time_major=True)
    assert mel_tm.shape == (3, nfs[0], n_mels) and torch.equal(dx_tm, dx)
    ref, e32 = _reference(c, x, conv, g, lengths=lens)
    _check(f"ragged {conv}", dx, ref, e32, yard)


def test_silence_is_finite_and_exactly_zero(cases):
    _, yard = cases
    c = _cfg("small")
    N, hop, n_mels = c["N"], c["hop"], c["n_mels"]
    x = G.silence_signal(N, hop, 160)
    g = G.upstream(1, n_mels, M.frames(160, N, hop, N // 2))
    ref = G.backward64(x, c["fwd"], c["melb"], N, hop, N // 2, g, 0.0)
    assert ref["min_mag"] == 0.0 and ref["clipped"] > 0                  # here the rules act
    _, dx = _grad(c, x, "taco", g)
    assert torch.isfinite(dx).all()
    assert bool((dx[0, :32] == 0).all()) and bool((ref["dx"][0, :32] == 0).all())   # samples that only silent frames reach
    e = max(G.rel_err(dx.cpu(), ref["dx"]))
    print(f"silence: e_hip {e:.3e}  e_hip / yardstick {e / yard:.2f}")
    assert e <= MARGIN * yard


@pytest.mark.parametrize("ragged", [False, True])
def test_analysis_backward(cases, ragged):
    _, yard = cases
    c = _cfg("default")
    N, hop = c["N"], c["hop"]
    bins = N // 2 + 1
    n = (TILE + 1) * hop + hop // 3
    lens = [n, n - hop - 7, N // 2 + 1 + hop] if ragged else None
    x = M.signal(3, n)
    gen = torch.Generator().manual_seed(17)
    d_re, d_im = torch.randn(3, bins, 1 + n // hop, generator=gen), torch.randn(3, bins, 1 + n // hop, generator=gen)
    want = G.analysis_autograd(x, c["fwd"], N, hop, d_re, d_im, lengths=lens)
    e32 = G.rel_err(G.analysis_autograd(x, c["fwd"], N, hop, d_re, d_im, lengths=lens, dtype=torch.float32), want)
    stft = c["stft"]
    xg = x.cuda().requires_grad_(True)
    out = _S().analysis(xg, stft.tables(), N, hop, want=("re", "im"), lengths=lens, differentiable=True, grad_packed=stft.grad_tables())
    re, im = out[0], out[1]
    plain = _S().analysis(x.cuda(), stft.tables(), N, hop, want=("re", "im"), lengths=lens)
    assert re.grad_fn is not None and torch.equal(re, plain[0]) and torch.equal(im, plain[1])
    torch.autograd.backward([re, im], [d_re.cuda(), d_im.cuda()])
    e = G.rel_err(xg.grad.cpu(), want)
    print(f"analysis backward ragged={ragged}: e_hip {max(e):.3e}  e32 {max(e32):.3e}  e_hip / yardstick {max(e) / yard:.2f}")
    assert max(e) <= MARGIN * yard
    if ragged:
        for b in range(3):
            assert bool((xg.grad[b, lens[b]:] == 0).all())
    # one plane alone: the other reads as zeros
    xg2 = x.cuda().requires_grad_(True)
    (only_re,) = _S().analysis(xg2, stft.tables(), N, hop, want=("re",), differentiable=True, grad_packed=stft.grad_tables())
    only_re.backward(d_re.cuda())
    e = G.rel_err(xg2.grad.cpu(), G.analysis_autograd(x, c["fwd"], N, hop, d_re, torch.zeros_like(d_im)))
    assert max(e) <= MARGIN * yard


def test_surface(cases):
    from tacotron2_subword_amd import utils
    from tacotron2_subword_amd.soft_dtw_cuda import SoftDTW
    _, yard = cases
    c = _cfg("default")
    N, hop, n_mels = c["N"], c["hop"], c["n_mels"]
    x = M.signal(2, 33 * hop + 50)
    # TacotronSTFT: opt-in returns self; without it the old refusal stands, word for word
    plain = _S().TacotronSTFT().cuda()
    gpu = _S().TacotronSTFT().cuda()
    assert gpu.differentiable() is gpu
    xg = x.cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match="log_mel is inference only: the input requires grad and grad mode is on; call it under "
                                           r"torch.no_grad\(\) or detach the input"):
        plain.mel_spectrogram(xg)
    with pytest.raises(RuntimeError, match="stft analysis is inference only: the input requires grad and grad mode is on"):
        _S().analysis(xg, c["stft"].tables(), N, hop)
    mel = gpu.mel_spectrogram(xg)
    assert mel.grad_fn is not None and torch.equal(mel, plain.mel_spectrogram(x.cuda()))
    assert not gpu.mel_spectrogram(x.cuda()).requires_grad             # nothing to track: the plain path
    g = G.upstream(2, n_mels, mel.shape[2])
    mel.backward(g.cuda())
    ref, e32 = _reference(c, x, "taco", g)
    _check("TacotronSTFT.cuda().differentiable()", xg.grad, ref, e32, yard)
    # utils.mel_spectrogram_from_audio against the torch.stft formula's autograd in fp64.  The kernel's basis is the fp32 rounding
    # of the basis torch.stft applies in fp64; what that rounding alone moves is the distance e_basis between the two fp64
    # gradients (explicit backward with the rounded basis, autograd through torch.stft), and by the triangle inequality the
    # kernel is held to the yardstick plus that distance
    yg = x.cuda().requires_grad_(True)
    m2 = utils.mel_spectrogram_from_audio(yg, differentiable=True)
    assert m2.grad_fn is not None and m2.shape == (2, n_mels, 33)
    g2 = G.upstream(2, n_mels, 33, seed=1)
    m2.backward(g2.cuda())
    y64 = x.double().requires_grad_(True)
    yp = torch.nn.functional.pad(y64[:, None], (384, 384), mode="reflect")[:, 0]
    spec = torch.stft(yp, N, hop_length=hop, win_length=N, window=torch.hann_window(N, dtype=torch.float64), center=False, return_complex=True)
    out = torch.log(torch.clamp(torch.matmul(c["melb"].double(), torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)), min=1e-5))
    (out * g2.double()).sum().backward()
    rounded = G.backward64(x, c["fwd"], c["melb"], N, hop, 384, g2, 1e-9)
    assert rounded["clipped"] == 0 and rounded["min_mag"] > 0
    e_basis = max(G.rel_err(rounded["dx"], y64.grad.detach()))
    e = max(G.rel_err(yg.grad.cpu(), y64.grad.detach()))
    print(f"mel_spectrogram_from_audio against torch.stft fp64 autograd: e_hip {e:.3e}  e_basis {e_basis:.3e}  bound {MARGIN * yard + e_basis:.3e}")
    assert e_basis < 2e-7 and e <= MARGIN * yard + e_basis
    with torch.no_grad():
        assert torch.equal(utils.mel_spectrogram_from_audio(x.cuda()), m2.detach())
    # SoftDTW on mels of waveforms: a gradient reaches the waveform
    sdtw = SoftDTW(use_cuda=True, gamma=0.1)
    yh = (0.9 * M.signal(2, 33 * hop + 50, seed=5)).cuda().requires_grad_(True)
    loss = sdtw(gpu.mel_spectrogram(yh, time_major=True), gpu.mel_spectrogram(x.cuda(), time_major=True)).sum()
    loss.backward()
    assert torch.isfinite(yh.grad).all() and float(yh.grad.abs().max()) > 0
    # refusals
    for kw in (dict(return_power=True), dict(out=torch.empty(2, n_mels, 34, device="cuda")), dict(scratch=torch.empty(16, device="cuda"))):
        with pytest.raises(RuntimeError, match="differentiable=True does not go with return_power, out= or scratch="):
            _S().log_mel(x.cuda(), gpu.stft_fn, gpu.mel_basis, differentiable=True, **kw)
    for k in ("mag", "phase"):
        with pytest.raises(RuntimeError, match=f'no backward for "{k}"'):
            _S().analysis(xg, c["stft"].tables(), N, hop, want=("re", k), differentiable=True, grad_packed=c["stft"].grad_tables())
    odd = _S().STFT(1024, 300, 1024).cuda()
    with pytest.raises(RuntimeError, match="filter_length=1024 is not a multiple of hop_length=300"):
        _S().log_mel(xg, odd, gpu.mel_basis, differentiable=True)
    assert _S().log_mel(x.cuda(), odd, gpu.mel_basis, differentiable=True)[0].shape[1] == n_mels   # the forward's own limits are unchanged
