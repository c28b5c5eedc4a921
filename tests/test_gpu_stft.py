"""GPU checks of the STFT kernels (csrc/stft.hip): analysis and synthesis through the unit entry points against fp64 torch on
the CPU, the modules against the vectors recorded from the reference.

Bounds (derived, not measured; every case prints its worst error / bound):
  analysis re, im:  1e-6 * S + 1e-7 per element, S = the same products over absolute values in fp64.  An fp32 MFMA chain is a
    k-ordered fmaf chain with up to 3.5e-7 * S of error; 1e-6 is that with a margin of 3 (the vocoder tests' form).
  mag, phase:  through mag*cos(phase) and mag*sin(phase) against the fp64 re and im, with 4e-7 * |z| on top (sqrtf, atan2f
    and the fp64 cos/sin of an fp32 phase: a few ulp of |z|).  The phase alone is ill-conditioned where |z| is small.
  synthesis:  2e-6 * S + 1e-7, S = the overlap-add of |X| and |inverse basis| through the same epilogue: the loader's sincosf
    or gain adds a few ulp per operand on top of the chain.
  modules against the recording:  20 x the reference's own fp32-versus-fp64 error, stored per quantity in the recording.
Every comparison also asserts that the fp64 reference exceeds 0.1 somewhere, so that it pins something.

Inputs are a ramp in time times a per-item gain and sign (and a seeded sign per sample, see _signal) plus a seeded tone
(planes: a ramp over frames times a per-bin and per-item factor, seeded phases), so that a shifted frame, swapped planes, a
neighbouring item or a mirrored reflect index cannot pass.  The exact-integer synthesis case compares the overlap-add sum itself: it runs the unit entry point with
windowed = 0 (the reference's STFT(window=None) branch), which skips the envelope division and the N/hop scale."""
import math

import numpy as np
import pytest
import torch

import stft_ref as R

pytestmark = pytest.mark.gpu

TILE = 32
CONFIGS = {"small": (64, 16, 64), "short_window": (512, 128, 400), "default": (1024, 256, 1024), "nonpow2": (800, 200, 800)}
_cache = {}


def _L():
    from tacotron2_subword_amd import _lib as L
    assert L.STFT_FRAME_TILE == TILE
    return L


def _S():
    from tacotron2_subword_amd import stft as S
    return S


def _cfg(name):
    """The module's own bases and squared window, and the kernels' packed tables, once per configuration."""
    if name not in _cache:
        N, hop, win = CONFIGS[name]
        assert _L().stft_plan(N, hop).frame_tile == TILE
        m = _S().STFT(N, hop, win)
        fwd, inv = m.forward_basis[:, 0, :].clone(), m.inverse_basis[:, 0, :].clone()
        wsq = m.window_sq()
        packed = _S().pack_tables(fwd.cuda(), inv.cuda(), torch.from_numpy(wsq).cuda(), N, hop)
        _cache[name] = dict(N=N, hop=hop, win=win, fwd=fwd, inv=inv, wsq=wsq, packed=packed)
    return _cache[name]


def _signal(B, n, seed=0):
    """(0.3 + 0.5 t/n) * sign_t * gain_b + a seeded tone.  sign_t is a seeded +-1 per sample (the same for every item): c = 1e-6
    was derived for chains whose products mix signs (operands uniform in [-1, 1)); under a one-signed ramp the low bins are
    sums of K one-signed products, whose fmaf chain errs by about 0.6 * sqrt(K) * 2^-24 * S (5.7e-7 * S at K = 400),
    a property of that input and not of the kernel."""
    g = torch.Generator().manual_seed(100 + seed)
    t = torch.arange(n, dtype=torch.float64)
    gain = torch.tensor([1.0, -0.75, 0.5])[:B].double().view(B, 1)
    f = (0.01 + 0.2 * torch.rand(B, 1, generator=g, dtype=torch.float64))
    ph = 6.0 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    sign = (torch.randint(0, 2, (n,), generator=torch.Generator().manual_seed(55)) * 2 - 1).double()
    return (gain * sign * (0.3 + 0.5 * t / n) + 0.2 * torch.sin(2 * math.pi * f * t + ph)).float()


def _planes(B, bins, nf, mode, seed=0):
    """polar: (magnitude, phase); denoise: (re, im, bias).  A ramp over frames times per-bin and per-item factors."""
    g = torch.Generator().manual_seed(200 + seed)
    ramp = (1.0 + torch.arange(nf, dtype=torch.float64) / max(nf, 1)).view(1, 1, nf)
    perbin = (1.0 + (torch.arange(bins) % 5).double() / 4).view(1, bins, 1)
    gain = torch.tensor([1.0, 0.75, 0.5])[:B].double().view(B, 1, 1)
    if mode == 0:
        return (gain * ramp * perbin).float(), ((torch.rand(B, bins, nf, generator=g, dtype=torch.float64) * 2 - 1) * math.pi).float(), None
    re = (gain * ramp * perbin * torch.randn(B, bins, nf, generator=g, dtype=torch.float64)).float()
    im = (gain * ramp * perbin * torch.randn(B, bins, nf, generator=g, dtype=torch.float64)).float()
    bias = (0.2 + 1.3 * torch.rand(bins, generator=g, dtype=torch.float64)).float()
    return re, im, bias


def _X64(a, b, bias, strength, mode):
    """The synthesis operand in fp64 from the fp32 inputs; strength is the fp32 value the kernel receives."""
    a, b = a.double(), b.double()
    if mode == 0:
        return torch.cat([a * torch.cos(b), a * torch.sin(b)], dim=1)
    m = torch.sqrt(a * a + b * b)
    sb = (bias.double() * float(np.float32(strength))).float().double().view(1, -1, 1)     # bias * strength is one fp32 product
    gain = torch.where(m > 0, torch.clamp(m - sb, min=0.0) / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(m))
    return torch.cat([gain * a, gain * b], dim=1)


def _check(tag, got, ref, bound):
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert torch.isfinite(got).all(), tag
    assert float(ref.abs().max()) > 0.1, tag
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print(f"{tag}: max err {float(err.max()):.3e}  worst err/bound {worst:.3f}  max |ref| {float(ref.abs().max()):.3e}")
    assert worst <= 1.0, tag
    return worst


def _analysis_lengths(N, hop):
    """The shortest signal reflect padding takes, then frame counts TILE - 1, TILE, TILE + 1 (not at a multiple of hop)."""
    return [N // 2 + 1] + [(nf - 1) * hop + hop // 3 for nf in (TILE - 1, TILE, TILE + 1) if (nf - 1) * hop + hop // 3 > N // 2]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_analysis_vs_fp64(name, B):
    c = _cfg(name)
    N, hop = c["N"], c["hop"]
    for n in _analysis_lengths(N, hop):
        x = _signal(B, n)
        re, im, mag, ph = (t.cpu() for t in _S().analysis(x.cuda(), c["packed"], N, hop, want=("re", "im", "mag", "phase")))
        re64, im64, (sre, sim) = R.analysis64(x, c["fwd"], N, hop)
        assert re.shape == (B, N // 2 + 1, 1 + n // hop)
        tag = f"analysis {name} B={B} n={n} nf={1 + n // hop}"
        _check(tag + " re", re, re64, 1e-6 * sre + 1e-7)
        z = torch.sqrt(re64 ** 2 + im64 ** 2)
        _check(tag + " im", im, im64, 1e-6 * sim + 1e-7)
        _check(tag + " mag*cos", mag.double() * torch.cos(ph.double()), re64, 1e-6 * sre + 1e-7 + 4e-7 * z)
        _check(tag + " mag*sin", mag.double() * torch.sin(ph.double()), im64, 1e-6 * sim + 1e-7 + 4e-7 * z)
        assert (mag >= 0).all() and (ph.abs() <= math.pi + 1e-6).all()


def test_analysis_short_signal_raises():
    c = _cfg("default")
    with pytest.raises(RuntimeError, match="Padding size should be less than"):
        _S().analysis(torch.zeros(1, 512, device="cuda"), c["packed"], 1024, 256)
    with pytest.raises(RuntimeError, match="Padding size should be less than"):      # torch's reflect pad, in the same words
        torch.nn.functional.pad(torch.zeros(1, 1, 512), (512, 512), mode="reflect")
    _S().analysis(torch.zeros(1, 513, device="cuda"), c["packed"], 1024, 256)


def test_analysis_exact_integers_bit_for_bit():
    # small integers, the window forced to ones by giving the unit entry point a basis of integers: every product and sum is
    # exact in fp32, so any summation order must give the fp64 result exactly
    g = torch.Generator().manual_seed(7)
    N, hop, B = 128, 32, 2
    n = (TILE + 1) * hop + 5
    fwd = torch.randint(-3, 4, (N + 2, N), generator=g).float()
    inv = torch.zeros(N + 2, N)
    x = torch.randint(-4, 5, (B, n), generator=g).float()
    packed = _S().pack_tables(fwd.cuda(), inv.cuda(), None, N, hop)
    re, im = (t.cpu() for t in _S().analysis(x.cuda(), packed, N, hop))
    re64, im64, _ = R.analysis64(x, fwd, N, hop)
    assert float(re64.abs().max()) < 2 ** 23 and float(re64.abs().max()) > 0.1
    assert torch.equal(re, re64.float()) and torch.equal(im, im64.float())


@pytest.mark.parametrize("mode", [0, 1], ids=["polar", "denoise"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_synthesis_vs_fp64(name, B, mode):
    from tacotron2_subword_amd.audio_processing import window_sumsquare
    c = _cfg(name)
    N, hop, win = c["N"], c["hop"], c["win"]
    Rr, bins = N // hop, N // 2 + 1
    strength = 0.9
    for nf in (1, 2, Rr - 1, TILE - 1, TILE, TILE + 1, TILE + 2):
        a, b, bias = _planes(B, bins, nf, mode, seed=nf)
        got = _S().synthesis(a.cuda(), b.cuda(), c["packed"], N, hop, mode=mode, bias=None if bias is None else bias.cuda(), strength=strength).cpu()
        assert got.shape == (B, 1, hop * (nf - 1))
        if nf == 1:
            continue
        env = window_sumsquare("hann", nf, hop_length=hop, win_length=win, n_fft=N, dtype=np.float32)
        X = _X64(a, b, bias, strength, mode)
        ref = R.finish64(R.ola64(X, c["inv"], N, hop), env, N, hop)
        S = R.finish64(R.ola64(X.abs(), c["inv"].abs(), N, hop), env, N, hop)
        _check(f"synthesis {name} B={B} nf={nf} mode={mode}", got, ref, 2e-6 * S + 1e-7)


def test_synthesis_exact_integers_bit_for_bit():
    # integer (re, im) through the denoise loader with a zero bias: the gain is |z| / |z| = 1 exactly, the inverse basis holds
    # small integers, windowed = 0 leaves the overlap-add sum as it is: it must equal the fp64 overlap-add bit for bit
    g = torch.Generator().manual_seed(9)
    N, hop, B, nf = 128, 32, 2, TILE + 3
    bins = N // 2 + 1
    inv = torch.randint(-3, 4, (N + 2, N), generator=g).float()
    re = torch.randint(-4, 5, (B, bins, nf), generator=g).float()
    im = torch.randint(-4, 5, (B, bins, nf), generator=g).float()
    packed = _S().pack_tables(torch.zeros(N + 2, N).cuda(), inv.cuda(), None, N, hop)
    got = _S().synthesis(re.cuda(), im.cuda(), packed, N, hop, mode=1, bias=torch.zeros(bins).cuda(), strength=0.9, windowed=False).cpu()
    ref = R.finish64(R.ola64(torch.cat([re, im], 1), inv, N, hop), None, N, hop)
    assert 0.1 < float(ref.abs().max()) < 2 ** 23 and got.shape == ref.shape
    assert torch.equal(got, ref.float())


def test_determinism_and_batch_independence():
    c = _cfg("default")
    N, hop = c["N"], c["hop"]
    x = _signal(3, 40 * hop + 7).cuda()
    o1 = _S().analysis(x, c["packed"], N, hop, want=("re", "im", "mag", "phase"))
    o2 = _S().analysis(x, c["packed"], N, hop, want=("re", "im", "mag", "phase"))
    alone = _S().analysis(x[1:2].contiguous(), c["packed"], N, hop, want=("re", "im", "mag", "phase"))
    for u, v, w in zip(o1, o2, alone):
        assert torch.equal(u, v) and torch.equal(u[1:2], w) and not torch.equal(u[0:1], w)
    for mode in (0, 1):
        a, b, bias = _planes(3, N // 2 + 1, TILE + 5, mode)
        kw = dict(mode=mode, bias=None if bias is None else bias.cuda(), strength=0.9)
        y1 = _S().synthesis(a.cuda(), b.cuda(), c["packed"], N, hop, **kw)
        y2 = _S().synthesis(a.cuda(), b.cuda(), c["packed"], N, hop, **kw)
        ya = _S().synthesis(a[1:2].cuda(), b[1:2].cuda(), c["packed"], N, hop, **kw)
        assert torch.equal(y1, y2) and torch.equal(y1[1:2], ya) and not torch.equal(y1[0:1], ya)


# ---- the modules against the recording ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def G():
    return R.golden()


def _rec(tag, got, G, key, name, scale=20.0):
    rec = torch.from_numpy(G[f"{key}_{name}"]).double()
    bound = scale * float(G[f"err_{key}_{name}"])
    return _check(f"{tag} {key} {name} (bound {bound:.2e})", got.cpu(), rec, torch.full_like(rec, bound))


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_modules_vs_recording(G, name):
    from tacotron2_subword_amd.bias_remover import hifiganBiasRemover
    N, hop, win = R.CONFIGS[name]
    x = R.wave().cuda()
    s = _S().STFT(N, hop, win).cuda()
    inv = s.inverse(*s.transform(x))
    fwd = s.forward(x)
    assert not inv.requires_grad and not fwd.requires_grad
    _rec("STFT", inv, G, "inverse", name)
    _rec("STFT", fwd, G, "forward", name)
    br = hifiganBiasRemover(R.stub_model, filter_length=N, n_overlap=N // hop, win_length=win).cuda()
    first = br.stft.transform(R.stub_model(torch.zeros(1, 80, 88, device="cuda")).squeeze(0))[0][:, :, :1]
    assert tuple(br.bias_spec.shape) == (1, N // 2 + 1, 1)
    assert float((br.bias_spec - first).abs().max()) <= 1e-6 * float(first.abs().max())
    rec_bias = torch.from_numpy(G[f"bias_{name}"]).cuda()
    assert float((br.bias_spec - rec_bias).abs().max()) <= 1e-5 * float(rec_bias.abs().max())
    y09, y01 = br(x, 0.9), br(x, 0.1)
    assert not y09.requires_grad and y09.dim() == 3 and y09.shape[1] == 1
    _rec("remover", y09, G, "br09", name)
    _rec("remover", y01, G, "br01", name)
    diff = float((y09 - fwd).abs().max())
    print(f"bias-removed audio differs from the plain round trip by {diff:.3f}")
    assert diff > 0.1                                        # cannot pass by ignoring the bias
    # strength 0 is the plain round trip, by the other loader
    bound = 20.0 * float(G[f"err_forward_{name}"])
    assert float((br(x, 0.0) - fwd).abs().max()) <= bound


def test_griffin_lim_vs_recording(G):
    from tacotron2_subword_amd.audio_processing import griffin_lim
    s = _S().STFT(1024, 256, 1024).cuda()
    mag, _ = s.transform(R.wave().cuda())
    sig = griffin_lim(mag, s, n_iters=2, angles=G["gl_angles"])          # host-drawn phases move to the magnitudes' device
    assert sig.is_cuda and not sig.requires_grad
    _rec("griffin_lim", sig, G, "gl", "default")


def test_round_trip(G):
    s = _S().STFT(1024, 256, 1024).cuda()
    x = R.wave()
    y = s.forward(x.cuda()).cpu()
    n = y.shape[-1]
    assert n == 256 * (4000 // 256)
    bound = 20.0 * float(G["err_forward_default"])
    err = float((y[:, 0] - x[:, :n]).abs().max())
    print(f"round trip: max err {err:.3e} bound {bound:.3e}")
    assert float(x.abs().max()) > 0.1 and err <= bound


def test_surface():
    s = _S().STFT(1024, 256, 1024).cuda()
    with pytest.raises(RuntimeError, match="one shape"):
        s.inverse(torch.zeros(1, 513, 4, device="cuda"), torch.zeros(1, 513, 5, device="cuda"))
    with pytest.raises(RuntimeError, match="one shape"):
        s.inverse(torch.zeros(1, 512, 4, device="cuda"), torch.zeros(1, 512, 4, device="cuda"))
    bad = _S().STFT(1024, 300, 1024).cuda()
    with pytest.raises(RuntimeError, match=r"1024.*300"):
        bad.inverse(torch.zeros(1, 513, 4, device="cuda"), torch.zeros(1, 513, 4, device="cuda"))
    m = torch.ones(1, 513, 4, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        s.inverse(m, torch.zeros(1, 513, 4, device="cuda"))
    with torch.no_grad():
        assert not s.inverse(m, torch.zeros(1, 513, 4, device="cuda")).requires_grad
    # the packed tables follow the buffers
    t0 = s.tables()
    assert s.tables() is t0
    s2 = s.cpu().cuda()
    assert s2._packed is None and s2.tables() is not t0
