"""GPU checks of the log-mel kernel (csrc/melspec.hip) against fp64 torch on the CPU.

The bound is melspec_ref.py's (derived there, not fitted); every comparison prints its worst error / bound.  Inputs are
melspec_ref.signal (test_gpu_stft.py's ramp with seeded signs plus a seeded tone, clamped to [-1, 1]): for it the fp64 mel
never reaches the clip at any configuration below, which every comparison asserts (a share of exactly 0 at the clip), so no
element is left unpinned.  The edge cases use a dense seeded mel table, so that every (row, bin) of the packed table counts."""
import pytest
import torch

import melspec_ref as M

pytestmark = pytest.mark.gpu

TILE = 32
_cache = {}


def _S():
    from tacotron2_subword_amd import stft as S
    return S


def _L():
    from tacotron2_subword_amd import _lib as L
    return L


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
    """A length that is no multiple of hop and gives nf frames."""
    return (nf - 1) * c["hop"] + c["hop"] // 3 if conv == "taco" else nf * c["hop"] + c["hop"] // 3


def _run(c, x, conv, melb=None, **kw):
    pad, eps = _conv(c, conv)
    return _S().log_mel(x.cuda(), c["stft"], c["melb_gpu"] if melb is None else melb, pad=pad, mag_eps=eps, **kw)


def _check(tag, got, ref):
    assert got.shape == ref["logmel"].shape, (tag, got.shape, ref["logmel"].shape)
    assert torch.isfinite(got).all(), tag
    assert float(ref["logmel"].abs().max()) > 0.1, tag
    assert int(ref["clipped"].sum()) == 0, tag                         # share at the clip: exactly 0
    err = (got.double() - ref["logmel"]).abs()
    worst = float((err / ref["log_bound"]).max())
    print(f"{tag}: max err {float(err.max()):.3e}  worst err/bound {worst:.3f}  min mel {float(ref['mel'].min()):.2e}  "
          f"largest bound {float(ref['log_bound'].max()):.2e}")
    assert worst <= 1.0, tag
    return worst


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(M.CONFIGS))
def test_vs_fp64(name, B):
    c = _cfg(name)
    N, hop = c["N"], c["hop"]
    for conv in ("taco", "hifigan"):
        pad, eps = _conv(c, conv)
        for n in [pad + 1] + [_n_for_frames(c, conv, nf) for nf in (TILE - 1, TILE, TILE + 1)]:
            x = M.signal(B, n)
            ref = M.logmel64(x, c["fwd"], c["melb"], N, hop, pad, eps)
            nf = M.frames(n, N, hop, pad)
            assert ref["logmel"].shape == (B, c["n_mels"], nf)
            got, fl = _run(c, x, conv)
            assert fl is None
            _check(f"{name} {conv} B={B} n={n} nf={nf}", got.cpu(), ref)
            tm, _ = _run(c, x, conv, time_major=True)
            assert tm.shape == (B, nf, c["n_mels"]) and torch.equal(tm.transpose(1, 2), got)


@pytest.mark.parametrize("n_mels", [33, 128])
@pytest.mark.parametrize("name", ["short_window", "small"])      # 257 bins: five passes, the last with one live tile; 33 bins: one pass
def test_row_and_bin_edges(name, n_mels):
    c = _cfg(name)
    N, hop = c["N"], c["hop"]
    bins = N // 2 + 1
    assert _L().melspec_plan(N, hop, N // 2, n_mels, 4000).passes == (5 if name == "short_window" else 1)
    g = torch.Generator().manual_seed(n_mels)
    melb = (torch.rand(n_mels, bins, generator=g) * (0.5 + (torch.arange(n_mels) % 7).float()[:, None]) / bins).float()
    x = M.signal(2, 35 * hop + 5)
    for conv in ("taco", "hifigan"):
        pad, eps = _conv(c, conv)
        ref = M.logmel64(x, c["fwd"], melb, N, hop, pad, eps)
        got, _ = _run(c, x, conv, melb=melb.cuda())
        _check(f"edges {name} n_mels={n_mels} {conv}", got.cpu(), ref)
        tm, _ = _run(c, x, conv, melb=melb.cuda(), time_major=True, force_splits=_L().melspec_plan(N, hop, pad, n_mels, x.shape[1]).passes)
        assert torch.equal(tm.transpose(1, 2), got)


def test_exact_integers_bit_for_bit():
    # an integer basis, an integer mel table and an integer signal: with return_power the kernel's output is a sum of products
    # of squared integers, exact in fp32 whatever the order, so it must equal the fp64 result bit for bit
    g = torch.Generator().manual_seed(7)
    N, hop, B, n_mels = 256, 64, 2, 40
    bins = N // 2 + 1
    n = (TILE + 1) * hop + 5
    stft = _S().STFT(N, hop, N).cuda()
    fwd = torch.randint(-1, 2, (2 * bins, N), generator=g).float()
    with torch.no_grad():
        stft.forward_basis.copy_(fwd[:, None, :])                     # the tables follow the buffer
    melb = (torch.rand(n_mels, bins, generator=g) < 0.3).float() * torch.randint(1, 3, (n_mels, bins), generator=g).float()
    x = torch.randint(-1, 2, (B, n), generator=g).float()
    assert _L().melspec_plan(N, hop, N // 2, n_mels, n, B).passes == 3
    re, im, _ = M.analysis64(x, fwd, N, hop, N // 2)
    ref = torch.matmul(melb.double(), re ** 2 + im ** 2)
    assert 0.1 < float(ref.max()) < 2 ** 24
    for splits in (1, 3):
        got, _ = _S().log_mel(x.cuda(), stft, melb.cuda(), return_power=True, force_splits=splits)
        assert torch.equal(got.cpu(), ref.float())
        tm, _ = _S().log_mel(x.cuda(), stft, melb.cuda(), return_power=True, force_splits=splits, time_major=True)
        assert torch.equal(tm.cpu().transpose(1, 2), ref.float())


def test_split_equality_batch_independence_determinism():
    c = _cfg("default")
    passes = _L().melspec_plan(1024, 256, 512, 80, 40 * 256 + 7, 3).passes
    assert passes == 9
    x = M.signal(3, 40 * 256 + 7)
    for conv in ("taco", "hifigan"):
        for tm in (False, True):
            base, _ = _run(c, x, conv, time_major=tm, force_splits=1)
            for s in (0, 3, passes):
                assert torch.equal(_run(c, x, conv, time_major=tm, force_splits=s)[0], base), (conv, tm, s)
            assert torch.equal(_run(c, x, conv, time_major=tm, force_splits=1)[0], base)           # two runs, the same bits
            alone, _ = _run(c, x[1:2].contiguous(), conv, time_major=tm)                             # the plan splits B = 1
            assert torch.equal(base[1:2], alone) and not torch.equal(base[0:1], alone)
    with pytest.raises(RuntimeError, match=r"force_splits=10 outside 0\.\.passes=9"):
        _run(c, x, "taco", force_splits=10)


@pytest.mark.parametrize("conv", ["taco", "hifigan"])
def test_ragged_lengths_padding_and_guards(conv):
    c = _cfg("default")
    N, hop, n_mels = c["N"], c["hop"], c["n_mels"]
    pad, eps = _conv(c, conv)
    n_max = 70 * hop + 11
    lens = [n_max, 37 * hop + 101, pad + 1, pad]
    x = M.signal(4, n_max)
    x[1, lens[1]:] = 0.77                                               # what lies past an item's length must not matter
    x[2, lens[2]:] = -0.5
    nfs = [M.frames(v, N, hop, pad) for v in lens]
    assert nfs[3] == 0 and nfs[2] >= 1 and nfs[1] % TILE != 0
    plan = _L().melspec_plan(N, hop, pad, n_mels, n_max, 4)
    assert plan.nf_max == nfs[0]
    G, SENT, PADV = 64, 12345.0, -7.5
    lengths = torch.tensor(lens, dtype=torch.int32).cuda()
    for tm in (False, True):
        shape = (4, plan.nf_max, n_mels) if tm else (4, n_mels, plan.nf_max)
        numel = 4 * plan.nf_max * n_mels
        for splits in (1, 3):
            obuf = torch.full((numel + 2 * G,), SENT, device="cuda")
            sbuf = torch.full((plan.split_scratch_floats + 2 * G,), SENT, device="cuda")
            out, fl = _run(c, x, conv, lengths=lengths, time_major=tm, pad_value=PADV, force_splits=splits,
                           out=obuf[G:G + numel].view(shape), scratch=sbuf[G:G + plan.split_scratch_floats])
            assert fl.dtype == torch.int32 and fl.tolist() == nfs
            for buf in (obuf, sbuf):
                assert bool((buf[:G] == SENT).all()) and bool((buf[-G:] == SENT).all())
            assert not bool((obuf[G:-G] == SENT).any())                 # every element of out is written
            if splits == 1:
                assert bool((sbuf == SENT).all())                       # one launch, no scratch
            o = out.transpose(1, 2) if tm else out
            for b in range(4):
                assert bool((o[b, :, nfs[b]:] == PADV).all())
                if nfs[b]:
                    alone, _ = _run(c, x[b:b + 1, :lens[b]].contiguous(), conv)
                    assert torch.equal(o[b:b + 1, :, :nfs[b]], alone)
    ref = M.logmel64(x[1:2, :lens[1]], c["fwd"], c["melb"], N, hop, pad, eps)
    _check(f"ragged {conv} item 1", o[1:2, :, :nfs[1]].cpu(), ref)
    # values outside [0, n] are clamped by the kernel; Python ints are checked on the host, in torch's reflect-pad words
    out, fl = _run(c, x[:2], conv, lengths=torch.tensor([n_max + 1000, -5], dtype=torch.int32).cuda())
    assert fl.tolist() == [nfs[0], 0] and bool((out[1] == 0).all()) and torch.equal(out[0], o[0])
    with pytest.raises(RuntimeError, match="Padding size should be less than"):
        _run(c, x, conv, lengths=lens)
    with pytest.raises(RuntimeError, match=r"lengths\[0\]=\d+ exceeds"):
        _run(c, x, conv, lengths=[n_max + 1, 5000, 5000, 5000])
    out2, fl2 = _run(c, x[:3], conv, lengths=lens[:3], pad_value=PADV)
    assert fl2.tolist() == nfs[:3] and torch.equal(out2, o[:3])


def test_second_convention_vs_torch_stft_fp64():
    c = _cfg("default")
    N, hop = c["N"], c["hop"]
    x = M.signal(2, 33 * hop + 50)
    xp = torch.nn.functional.pad(x.double()[:, None], (384, 384), mode="reflect")[:, 0]
    spec = torch.stft(xp, N, hop_length=hop, win_length=N, window=torch.hann_window(N, dtype=torch.float64), center=False, return_complex=True)
    want = torch.log(torch.clamp(torch.matmul(c["melb"].double(), torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)), min=1e-5))
    ref = M.logmel64(x, M.stft_basis64(N, N), c["melb"], N, hop, 384, 1e-9, basis_rounding=2.0 ** -24)
    assert float((ref["logmel"] - want).abs().max()) < 1e-9
    ref["logmel"] = want
    got, _ = _run(c, x, "hifigan")
    _check("second convention vs torch.stft", got.cpu(), ref)


def test_modules(tmp_path):
    from scipy.io.wavfile import write
    from tacotron2_subword_amd import utils
    from tacotron2_subword_amd.Audio import tools
    from tacotron2_subword_amd.soft_dtw_cuda import SoftDTW
    c = _cfg("default")
    cpu, gpu = _S().TacotronSTFT(), _S().TacotronSTFT().cuda()
    x = M.signal(2, 40 * 256 + 9)
    ref = M.logmel64(x, c["fwd"], c["melb"], 1024, 256, 512)
    got = gpu.mel_spectrogram(x.cuda())
    assert not got.requires_grad
    _check("TacotronSTFT.cuda().mel_spectrogram", got.cpu(), ref)
    worst = float(((got.cpu() - cpu.mel_spectrogram(x)).abs().double() / (2 * ref["log_bound"])).max())   # both within the bound of fp64
    print(f"GPU module against CPU module: err / (2 * bound) {worst:.3f}")
    assert worst <= 1.0
    mel, fl = gpu.mel_spectrogram(x.cuda(), lengths=[x.shape[1], 5000], time_major=True)
    assert mel.shape == (2, 41, 80) and fl.tolist() == [41, 20] and torch.equal(mel[0].t(), got[0]) and bool((mel[1, 20:] == 0).all())
    t0 = gpu.stft_fn.mel_tables(gpu.mel_basis)                           # the packed tables follow the buffers
    assert gpu.stft_fn.mel_tables(gpu.mel_basis) is t0
    g2 = gpu.cpu().cuda()
    assert g2.stft_fn._mel_packed is None and torch.equal(g2.mel_spectrogram(x.cuda()), got)
    # surface
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        _S().log_mel(x, gpu.stft_fn, gpu.mel_basis)
    with pytest.raises(RuntimeError, match="float32 signal"):
        _S().log_mel(x.cuda().double(), gpu.stft_fn, gpu.mel_basis)
    with pytest.raises(RuntimeError, match="lengths must be int32"):
        _S().log_mel(x.cuda(), gpu.stft_fn, gpu.mel_basis, lengths=torch.tensor([5000, 5000]).cuda())
    with pytest.raises(RuntimeError, match="Padding size should be less than"):
        _S().log_mel(torch.zeros(1, 512, device="cuda"), gpu.stft_fn, gpu.mel_basis)
    xg = x.cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        _S().log_mel(xg, gpu.stft_fn, gpu.mel_basis)
    # files: utils.mel_spectrogram on the kernel against its CPU path, get_mel, and get_mel_batch into SoftDTW
    paths, lens = [], [33 * 256 + 17, 29 * 256 + 200, 31 * 256, 36 * 256 + 1]
    for i, n in enumerate(lens):
        paths.append(str(tmp_path / f"{i}.wav"))
        write(paths[-1], 22050, (M.signal(1, n, seed=i)[0] * 20000).round().to(torch.int16).numpy())
    a, b = utils.mel_spectrogram(paths[0]), utils.mel_spectrogram(paths[0], device="cpu")
    assert a.is_cuda and a.shape == b.shape == (1, 80, lens[0] // 256)
    y = utils.load_wav_to_torch(paths[0])[0].double() / 32768.0
    y = (y / y.abs().max() * 0.95).float()[None]
    r2 = M.logmel64(y, M.stft_basis64(1024, 1024), c["melb"], 1024, 256, 384, 1e-9, basis_rounding=2.0 ** -24)
    _check("utils.mel_spectrogram on the kernel", a.cpu(), r2)
    _check("utils.mel_spectrogram on the CPU", b, r2)
    singles = [tools.get_mel(p) for p in paths]
    assert all(not s.is_cuda and s.shape == (80, 1 + n // 256) for s, n in zip(singles, lens))
    mel, fl = tools.get_mel_batch(paths)
    assert mel.is_cuda and mel.shape == (4, 1 + max(lens) // 256, 80) and fl.tolist() == [1 + n // 256 for n in lens]
    for i, s in enumerate(singles):
        assert torch.equal(mel[i, :s.shape[1]].cpu(), s.t()) and bool((mel[i, s.shape[1]:] == 0).all())
    sdtw = SoftDTW(use_cuda=True, gamma=0.1)
    batched = sdtw(mel[:2], mel[2:], fl[:2], fl[2:])
    pairs = torch.cat([sdtw(singles[i].t()[None].contiguous().cuda(), singles[i + 2].t()[None].contiguous().cuda()) for i in range(2)])
    print(f"soft-DTW of two pairs: batched {batched.tolist()}  pair by pair {pairs.tolist()}")
    assert torch.isfinite(batched).all() and torch.equal(batched, pairs)
