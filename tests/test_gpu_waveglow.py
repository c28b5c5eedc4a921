"""GPU checks of WaveGlow inference (csrc/waveglow.hip): the single kernels through the unit entry points against fp64 torch on
the CPU, the whole model against the vectors recorded from the reference and against the fp64 restatement
(tests/waveglow_ref.py), the bias remover and the module's surface.

Single GEMM kernels are held to 1e-6 * mag + 1e-7 per output element, mag being the same sum over absolute values in fp64
(every term that is added into the element): an fp32 MFMA chain is a k-ordered fmaf chain, 1e-6 is its error with a margin
of about 3 (tests/test_gpu_hifigan.py).  The gate is held to 1e-6 * (magA + magB/4) + 3e-7: tanh is 1-Lipschitz, the sigmoid
1/4-Lipschitz, and 3e-7 covers a few ulp of tanhf / expf on outputs in [-1, 1].  Inputs are a ramp in time times a
per-channel sign (and a per-item gain), so that a shifted tap, a swapped row or a neighbouring item cannot pass.  End to end
the bound is 25 times the reference's own fp32 error on the same inputs, recorded with each case.  No test calls torch's
convolution library on the GPU: every reference is computed on the CPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import waveglow_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 128
DEV = "cuda"


def _L():
    from tacotron2_subword_amd import _lib as L
    assert L.VOCODER_TIME_TILE == TILE
    return L


def _glow():
    from tacotron2_subword_amd.waveglow import glow
    return glow


def _ramp(B, Cch, Lt, integer=False):
    t = torch.arange(Lt, dtype=torch.float64)
    sign = torch.tensor([1.0 if (c * 5 + 1) % 3 else -1.0 for c in range(Cch)], dtype=torch.float64)
    if integer:
        base = (t % 7 + 1).view(1, 1, Lt) + (torch.arange(Cch, dtype=torch.float64) % 3).view(1, Cch, 1)
        return (base * sign.view(1, Cch, 1) + torch.arange(B, dtype=torch.float64).view(B, 1, 1)).float()
    x = (1.0 + t / Lt).view(1, 1, Lt) * sign.view(1, Cch, 1) * (1.0 + 0.25 * torch.arange(B, dtype=torch.float64)).view(B, 1, 1)
    return x.float()


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _check(tag, got, ref, bound):
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print(tag, "max err", float(err.max()), "worst err/bound", worst, "min bound", float(bound.min()))
    assert torch.isfinite(got).all()
    assert worst <= 1.0, tag


# ------------------------------------------------------------------------------------------------------------------ 1. gated conv
def _gated(x, spect, w_in, b_in, w_cond, b_cond, d, raw=False):
    L = _L()
    B, nc, Lt = x.shape
    n_cond = spect.shape[1]
    y = torch.full((B, 2 * nc if raw else nc, Lt), float("nan"), device=DEV)
    packed = torch.empty(L.lib().t2_waveglow_packed_floats(L.WAVEGLOW_GATED, nc, nc, n_cond), device=DEV)
    t = [_d(v) for v in (x, spect, w_in, b_in, w_cond, b_cond)]
    a = L.WaveglowGatedArgs(B, nc, n_cond, Lt, d, int(raw), *[L.ptr(v) for v in t], L.ptr(packed), L.ptr(y))
    L.check(L.lib().t2_waveglow_gated_conv(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    return y.cpu()


def _gated_ref(x, spect, w_in, b_in, w_cond, b_cond, d):
    """(pre-activation u, its sum over absolute values) in fp64."""
    u = F.conv1d(x.double(), w_in.double(), b_in.double(), dilation=d, padding=d) + F.conv1d(spect.double(), w_cond.double()[:, :, None], b_cond.double())
    mag = (F.conv1d(x.double().abs(), w_in.double().abs(), b_in.double().abs(), dilation=d, padding=d)
           + F.conv1d(spect.double().abs(), w_cond.double().abs()[:, :, None], b_cond.double().abs()))
    return u, mag


# (nc, n_cond, L, d, B): every L of {1, 32, 127, 128, 129, 258}, every d of {1, 2, 64, 128} (L shorter than d included),
# every nc of {8, 16, 24, 256}, both conditioning widths, both batch sizes
GATED_CASES = [
    (8, 64, 1, 1, 1),
    (8, 64, 32, 64, 1),              # the whole signal is shorter than the dilation
    (16, 64, 127, 2, 3),
    (24, 64, 128, 128, 1),           # taps at -L and +L: only the centre tap is inside
    (16, 640, 129, 128, 1),
    (8, 64, 258, 128, 3),            # three time tiles, the widest halo
    (24, 64, 258, 64, 1),
    (256, 640, 129, 2, 1),           # the published width: 8 row tiles, 16 + 40 chunks of K
    (256, 64, 32, 128, 1),
    (24, 640, 1, 128, 3),
]


@pytest.mark.parametrize("case", GATED_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gated_conv_vs_fp64(case):
    nc, n_cond, Lt, d, B = case
    g = torch.Generator().manual_seed(nc * 1000 + Lt * 10 + d)
    x, spect = _ramp(B, nc, Lt), _ramp(B, n_cond, Lt) * 0.5
    scale = (3 * nc + n_cond) ** -0.5                       # pre-activations of order 1: the gate is not saturated
    w_in, w_cond = torch.randn(2 * nc, nc, 3, generator=g) * scale, torch.randn(2 * nc, n_cond, generator=g) * scale
    b_in, b_cond = torch.randn(2 * nc, generator=g) * 0.1, torch.randn(2 * nc, generator=g) * 0.1
    got = _gated(x, spect, w_in, b_in, w_cond, b_cond, d)
    u, mag = _gated_ref(x, spect, w_in, b_in, w_cond, b_cond, d)
    ref = torch.tanh(u[:, :nc]) * torch.sigmoid(u[:, nc:])
    print("pre-activation std", float(u.std()), "output std", float(ref.std()))
    assert float(ref.std()) > 0.05
    _check(f"gated {case}", got, ref, 1e-6 * (mag[:, :nc] + mag[:, nc:] / 4) + 3e-7)
    raw = _gated(x, spect, w_in, b_in, w_cond, b_cond, d, raw=True)
    _check(f"gated raw {case}", raw, u, 1e-6 * mag + 1e-7)


def test_gated_conv_exact_integers_bit_for_bit():
    # small integers: every product and sum is exact in fp32, so any order must give the fp64 pre-activation exactly
    g = torch.Generator().manual_seed(5)
    B, nc, n_cond, Lt, d = 2, 24, 72, TILE + 3, 4
    x, spect = _ramp(B, nc, Lt, integer=True), _ramp(B, n_cond, Lt, integer=True)
    w_in, w_cond = torch.randint(-3, 4, (2 * nc, nc, 3), generator=g).float(), torch.randint(-3, 4, (2 * nc, n_cond), generator=g).float()
    b_in, b_cond = torch.randint(-5, 6, (2 * nc,), generator=g).float(), torch.randint(-5, 6, (2 * nc,), generator=g).float()
    u, _ = _gated_ref(x, spect, w_in, b_in, w_cond, b_cond, d)
    assert float(u.abs().max()) < 2 ** 23 and float(u.abs().max()) > 100
    assert torch.equal(_gated(x, spect, w_in, b_in, w_cond, b_cond, d, raw=True), u.float())


def test_gated_conv_refuses_unsupported_shapes():
    L = _L()
    z = torch.zeros(8 * 64 * 64, device=DEV)
    for nc, n_cond, d, needle in ((12, 64, 1, "n_channels=12"), (8, 60, 1, "60 conditioning channels"), (8, 64, 3, "dilation 3"), (8, 64, 256, "dilation 256")):
        a = L.WaveglowGatedArgs(1, nc, n_cond, 8, d, 0, *[L.ptr(z)] * 8)
        assert L.lib().t2_waveglow_gated_conv(C.byref(a), L.stream()) != 0
        assert needle in L.lib().t2_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------ 2. res_skip
@pytest.mark.parametrize("nc, Lt, B, first, last", [(8, 1, 1, 0, 0), (24, TILE + 1, 3, 1, 0), (24, 2 * TILE + 2, 1, 0, 1), (16, 40, 2, 1, 1),
                                                   (256, TILE - 1, 1, 0, 0), (256, 40, 1, 0, 1)])
def test_res_skip_vs_fp64(nc, Lt, B, first, last):
    L = _L()
    g = torch.Generator().manual_seed(nc * 100 + Lt)
    rows = nc if last else 2 * nc
    acts = _ramp(B, nc, Lt) * 0.5
    w, bias = torch.randn(rows, nc, generator=g) * nc ** -0.5, torch.randn(rows, generator=g) * 0.1
    x0, out0 = torch.randn(B, nc, Lt, generator=g), torch.randn(B, nc, Lt, generator=g)
    x, out = _d(x0).clone(), _d(out0).clone()
    if first:
        out.fill_(float("nan"))                             # taken as zero and never read
    packed = torch.empty(L.lib().t2_waveglow_packed_floats(L.WAVEGLOW_RES_SKIP, rows, nc, 0), device=DEV)
    t = [_d(acts), _d(w), _d(bias)]
    a = L.WaveglowResSkipArgs(B, nc, Lt, first, last, *[L.ptr(v) for v in t], L.ptr(packed), L.ptr(x), L.ptr(out))
    L.check(L.lib().t2_waveglow_res_skip(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    rs = F.conv1d(acts.double(), w.double()[:, :, None], bias.double())
    mag = F.conv1d(acts.double().abs(), w.double().abs()[:, :, None], bias.double().abs())
    o_prev = torch.zeros_like(out0.double()) if first else out0.double()
    if last:
        assert torch.equal(x.cpu(), x0)                     # the last layer leaves x alone
        _check("res_skip last: out", out.cpu(), o_prev + rs, 1e-6 * (mag + o_prev.abs()) + 1e-7)
    else:
        _check("res_skip: x", x.cpu(), x0.double() + rs[:, :nc], 1e-6 * (mag[:, :nc] + x0.double().abs()) + 1e-7)
        _check("res_skip: out", out.cpu(), o_prev + rs[:, nc:], 1e-6 * (mag[:, nc:] + o_prev.abs()) + 1e-7)


# ------------------------------------------------------------------------------------------------------------------ 3. upsample
@pytest.mark.parametrize("n_mel, T, G, B", [(8, 1, 8, 1), (8, 2, 8, 2), (8, 5, 8, 3), (80, 1, 8, 1), (80, 2, 8, 1), (80, 5, 8, 2),
                                             (8, TILE + 2, 8, 1), (8, 5, 2, 1), (8, 5, 6, 1)])
def test_upsample_and_regroup_vs_fp64(n_mel, T, G, B):
    L = _L()
    g = torch.Generator().manual_seed(n_mel * 10 + T)
    mel = _ramp(B, n_mel, T) * -2.0
    w, bias = torch.randn(n_mel, n_mel, 1024, generator=g) * (4 * n_mel) ** -0.5, torch.randn(n_mel, generator=g) * 0.1
    Lg = T * 256 // G
    spect = torch.full((B, n_mel * G, Lg), float("nan"), device=DEV)
    packed = torch.empty(L.lib().t2_waveglow_packed_floats(L.WAVEGLOW_UPSAMPLE, n_mel, n_mel, 0), device=DEV)
    t = [_d(mel), _d(w), _d(bias)]
    a = L.WaveglowUpsampleArgs(B, n_mel, T, G, *[L.ptr(v) for v in t], L.ptr(packed), L.ptr(spect))
    L.check(L.lib().t2_waveglow_upsample(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    cfg = dict(n_group=G)
    ref = R.upsample({"upsample.weight": w, "upsample.bias": bias}, cfg, mel)
    mag = R.upsample({"upsample.weight": w.abs(), "upsample.bias": bias.abs()}, cfg, mel.abs())
    assert ref.shape == spect.shape and float(ref.std()) > 0.1
    _check(f"upsample {(n_mel, T, G, B)}", spect.cpu(), ref, 1e-6 * mag + 1e-7)


# ------------------------------------------------------------------------------------------------------------------ 4. coupling
ULP = 2.0 ** -23


@pytest.mark.parametrize("n_half, n_early, nc, Lt, B, identity", [(4, 0, 8, 1, 1, True), (4, 0, 256, 257, 2, False), (3, 0, 24, 300, 1, True),
                                                                   (3, 2, 16, 255, 3, False), (2, 0, 256, 40, 1, False), (2, 2, 8, 513, 2, True)])
def test_coupling_vs_fp64(n_half, n_early, nc, Lt, B, identity):
    """(b, s) = end(out) are chains over nc: e = 1e-6 * mag + 1e-7 each.  a1' = (a1 - b) / exp(s) is held to e_b / exp(s) (that
    bound divided by exp(s)), plus |a1'| * e_s (what the error of s does to exp(-s), to first order), plus 2 ulp of |a1'| for
    the subtraction's and the division's rounding and expf.  With W_inverse = I the mix returns its input exactly, so the
    division is seen directly; otherwise the mix carries those errors through |W_inverse| and adds a chain's 1e-6 * mag + 1e-7."""
    L = _L()
    g = torch.Generator().manual_seed(n_half * 1000 + nc + Lt)
    c = 2 * n_half
    in_scale, sigma = (0.666, 0.666) if identity else (1.0, 0.5)
    out = _ramp(B, nc, Lt) * 0.5
    w_end, b_end = torch.randn(c, nc, generator=g) * 0.5 * nc ** -0.5, torch.randn(c, generator=g) * 0.1
    audio = torch.randn(B, c, Lt, generator=g)
    W = torch.eye(c) if identity else torch.linalg.qr(torch.randn(c, c, generator=g))[0].float().inverse().contiguous()
    z = torch.randn(B, max(n_early, 1), Lt, generator=g)
    dst = torch.full((B, n_early + c, Lt), float("nan"), device=DEV)
    inter = torch.full((B, Lt, c), float("nan"), device=DEV) if n_early == 0 else None
    t = [_d(out), _d(w_end), _d(b_end), _d(audio), _d(W), _d(z)]
    a = L.WaveglowCoupleArgs(B, nc, n_half, Lt, n_early, in_scale, sigma, *[L.ptr(v) for v in t], L.ptr(dst), L.ptr(inter))
    L.check(L.lib().t2_waveglow_couple(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    dst = dst.cpu()
    o = F.conv1d(out.double(), w_end.double()[:, :, None], b_end.double())
    e = 1e-6 * F.conv1d(out.double().abs(), w_end.double().abs()[:, :, None], b_end.double().abs()) + 1e-7
    b, s, e_b, e_s = o[:, :n_half], o[:, n_half:], e[:, :n_half], e[:, n_half:]
    assert 0.1 < float(s.abs().max()) < 3.0
    a_in = (audio * np.float32(in_scale)).double()          # the fp32 product the reference forms (sigma * z), taken as given
    a1 = (a_in[:, n_half:] - b) / torch.exp(s)
    v = torch.cat([a_in[:, :n_half], a1], 1)
    e_v = torch.cat([torch.zeros_like(e_b), e_b / torch.exp(s) + a1.abs() * e_s + 2 * ULP * a1.abs()], 1)
    if identity:
        ref, bound = v, e_v + 1e-30
    else:
        Wd = W.double()
        ref = torch.einsum("rc,bcl->brl", Wd, v)
        bound = torch.einsum("rc,bcl->brl", Wd.abs(), e_v) + 1e-6 * torch.einsum("rc,bcl->brl", Wd.abs(), v.abs()) + 1e-7
    _check(f"coupling {(n_half, n_early, nc, Lt, B)}", dst[:, n_early:], ref, bound)
    if n_early:
        assert torch.equal(dst[:, :n_early], z * np.float32(sigma))          # the prepended plane goes first
    else:
        assert torch.equal(inter.cpu(), dst.permute(0, 2, 1).contiguous())    # the waveform's order


# ------------------------------------------------------------------------------------------------------------------ 5-6. the recording
@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "waveglow.npz"))
    return {k: z[k] for k in z.files}


def _sd(gold, tag):
    return {k: torch.from_numpy(gold[k if k.startswith("upsample.") else f"{tag}/{k}"]) for k in json.loads(str(gold[f"{tag}_keys"]))}


def _case(gold, n):
    return torch.from_numpy(gold[f"mel{n}"]), [torch.from_numpy(gold[f"noise{n}_{j}"]) for j in range(2)]


@pytest.fixture(scope="module")
def models(gold):
    """{tag: (cfg, weight-normed module, module after remove_weightnorm)} on the GPU."""
    glow, out = _glow(), {}
    for tag, cfg in json.loads(str(gold["configs"])).items():
        pair = []
        for removed in (False, True):
            m = glow.WaveGlow(**cfg)
            m.load_state_dict(_sd(gold, tag))
            if removed:
                glow.WaveGlow.remove_weightnorm(m)
            pair.append(m.cuda().eval())
        out[tag] = (cfg, *pair)
    return out


@pytest.mark.parametrize("tag", ["a", "deep"])
def test_end_to_end_vs_reference_recording(gold, models, tag):
    cfg, normed, removed = models[tag]
    worst = 0.0
    with torch.no_grad():
        for n in range(len(gold["cases"])):
            mel, noise = _case(gold, n)
            for si, sigma in enumerate(gold["sigmas"]):
                audio, info = normed.infer_debug(_d(mel), float(sigma), [_d(z) for z in noise], debug=True)
                again = removed.infer(_d(mel), float(sigma), noise=[_d(z) for z in noise])
                assert torch.equal(audio, again)                                 # weight-normed and folded: equal bits
                ref, ref_err = torch.from_numpy(gold[f"{tag}_audio{n}_s{si}"]), float(gold[f"{tag}_ref_fp32_err{n}_s{si}"])
                assert audio.shape == ref.shape and audio.dtype == torch.float32
                err = float((audio.cpu().double() - ref.double()).abs().max())
                serr = float((info["spect"].cpu().double() - torch.from_numpy(gold[f"spect{n}"]).double()).abs().max())
                sref = float(gold[f"spect_ref_fp32_err{n}"])
                worst = max(worst, err / ref_err)
                print(tag, tuple(int(v) for v in gold["cases"][n]), "sigma", float(sigma), "audio err", err, "reference's own", ref_err, "ratio", err / ref_err,
                      "spect err", serr, "reference's own", sref, "ratio", serr / sref)
                assert torch.isfinite(audio).all()
                assert err <= 25 * ref_err
                assert serr <= 25 * sref
                fa = info["flow_audio"]
                assert torch.equal(audio, fa.permute(0, 2, 1).reshape(fa.shape[0], -1))
    print(tag, "worst audio err / reference's own fp32 err", worst)


@pytest.mark.parametrize("tag", ["a", "deep"])
def test_infer_undoes_the_reference_forward(gold, models, tag):
    """The recorded z is the reference's forward of its own audio; as noise (sigma = 1) it must give that audio back."""
    cfg, normed, _ = models[tag]
    with torch.no_grad():
        for n in range(len(gold["cases"])):
            mel, _ = _case(gold, n)
            for si in range(len(gold["sigmas"])):
                planes = R.planes_from_z(cfg, torch.from_numpy(gold[f"{tag}_z{n}_s{si}"]))
                audio = normed.infer(_d(mel), 1.0, noise=[_d(z) for z in planes])
                ref, ref_err = torch.from_numpy(gold[f"{tag}_audio{n}_s{si}"]), float(gold[f"{tag}_ref_fp32_err{n}_s{si}"])
                err = float((audio.cpu().double() - ref.double()).abs().max())
                print(tag, n, si, "audio err", err, "ratio to the reference's own", err / ref_err)
                assert err <= 25 * ref_err


# ------------------------------------------------------------------------------------------------------------------ 7. full width
@pytest.mark.parametrize("nc, B, T", [(256, 1, 2), (64, 1, 9)])
def test_full_width_vs_fp64_restatement(nc, B, T):
    cfg = dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2, WN_config=dict(n_layers=8, n_channels=nc, kernel_size=3))
    sd = R.make_state_dict(cfg, 31 + nc)
    folded, mel = R.fold(sd), R.make_mel(B, T, 41)
    g = torch.Generator().manual_seed(43)
    noise = [torch.randn(s, generator=g) for s in R.noise_shapes(cfg, B, T)]
    ref = R.infer(folded, cfg, mel, noise, 0.666)
    ref32 = R.infer(folded, cfg, mel, noise, 0.666, dtype=torch.float32)
    ref_err = float((ref32.double() - ref).abs().max())
    model = _glow().WaveGlow(**cfg)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    with torch.no_grad():
        audio = model.infer(_d(mel), 0.666, noise=[_d(z) for z in noise])
    err = float((audio.cpu().double() - ref).abs().max())
    print("channels", nc, "audio std", float(ref.std()), "err", err, "fp32 torch on the CPU vs fp64", ref_err, "ratio", err / ref_err)
    assert float(ref.std()) > 0.05
    assert audio.shape == (B, T * 256) and torch.isfinite(audio).all()
    assert err <= 25 * ref_err


# ------------------------------------------------------------------------------------------------------------------ 8. determinism
def test_same_bits_on_rerun_and_alone_vs_in_batch(gold, models):
    cfg, model, _ = models["deep"]
    B, T = 3, 5
    mel = R.make_mel(B, T, 7, n_mel=cfg["n_mel_channels"])
    g = torch.Generator().manual_seed(9)
    noise = [torch.randn(s, generator=g) for s in R.noise_shapes(cfg, B, T)]
    with torch.no_grad():
        a = model.infer(_d(mel), 0.666, noise=[_d(z) for z in noise])
        b = model.infer(_d(mel), 0.666, noise=[_d(z) for z in noise])
        assert torch.equal(a, b)
        for i in range(B):
            alone = model.infer(_d(mel[i:i + 1]), 0.666, noise=[_d(z[i:i + 1]) for z in noise])
            assert torch.equal(alone[0], a[i]), i
    assert float((a[0] - a[1]).abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------------------------ 9. bias remover
def test_waveglow_bias_remover(tmp_path):
    from tacotron2_subword_amd.bias_remover import hifiganBiasRemover, waveglowBiasRemover
    cfg = dict(n_mel_channels=80, n_flows=4, n_group=8, n_early_every=2, n_early_size=2, WN_config=dict(n_layers=2, n_channels=8, kernel_size=3))
    model = _glow().WaveGlow(**cfg)
    model.load_state_dict(R.make_state_dict(cfg, 3, end_std=0.05))
    model = model.cuda().eval()
    remover = waveglowBiasRemover(model)
    with torch.no_grad():
        bias_audio = model.infer(torch.zeros(1, 80, 88, device=DEV), sigma=0.0)
        spec, _ = remover.stft.transform(bias_audio)
    assert bias_audio.shape == (1, 88 * 256) and float(bias_audio.std()) > 1e-3
    assert remover.bias_spec.shape == (1, 513, 1) and torch.equal(remover.bias_spec, spec[:, :, :1])
    path = str(tmp_path / "waveglow.pt")
    torch.save({"model": model}, path)
    from_path = waveglowBiasRemover(model_path=path)
    assert torch.equal(from_path.bias_spec, remover.bias_spec)
    with torch.no_grad():
        other = hifiganBiasRemover(lambda mel: model.infer(mel, sigma=0.0).unsqueeze(0))
        assert torch.equal(other.bias_spec, remover.bias_spec)
        audio = torch.randn(2, 256 * 20 + 17, generator=torch.Generator().manual_seed(1)).to(DEV) * 0.3
        got, want = remover(audio, strength=0.01), other(audio, 0.01)
    assert got.shape == (256 * 20,) and torch.equal(got, want[:, 0][0])
    assert float((got - audio[0, :got.numel()]).abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ 10. surface
def test_surface(gold, models):
    cfg, model, _ = models["a"]
    glow = _glow()
    mel = _d(R.make_mel(2, 3, 1, n_mel=8))
    with torch.no_grad():
        audio = model.infer(mel, sigma=0.666)
    assert audio.shape == (2, 768) and audio.dtype == torch.float32 and audio.is_cuda and not audio.requires_grad
    with pytest.raises(RuntimeError, match="grad mode"):
        model.infer(mel)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            model.infer(mel.cpu())
        with pytest.raises(RuntimeError, match=r"\[B, 8, T\]"):
            model.infer(_d(R.make_mel(1, 3, 1, n_mel=80)))
        with pytest.raises(RuntimeError, match="float32"):
            model.infer(mel.half())
        with pytest.raises(RuntimeError, match="1 noise planes given, the model draws 2"):
            model.infer(mel, noise=[torch.zeros(2, 6, 96, device=DEV)])
        with pytest.raises(RuntimeError, match="a noise plane is"):
            model.infer(mel, noise=[torch.zeros(2, 6, 96, device=DEV), torch.zeros(2, 2, 95, device=DEV)])
        with pytest.raises(RuntimeError, match="inference only"):
            model((mel, audio))
        # the draws consume the generator the same way at sigma = 0 and sigma = 1, in the reference's order
        torch.manual_seed(11)
        a1 = model.infer(mel, sigma=1.0)
        after1 = torch.randn(4, device=DEV)
        torch.manual_seed(11)
        a0 = model.infer(mel, sigma=0.0)
        after0 = torch.randn(4, device=DEV)
        assert torch.equal(after0, after1) and not torch.equal(a0, a1)
        torch.manual_seed(11)
        planes = [torch.empty(s, device=DEV).normal_() for s in R.noise_shapes(cfg, 2, 3)]
        assert torch.equal(model.infer(mel, sigma=1.0, noise=planes), a1)
        assert torch.equal(model.infer(mel, sigma=0.0, noise=[torch.zeros_like(z) for z in planes]), a0)
        # repack() after an edit behind autograd's back
        m = glow.WaveGlow(**cfg)
        m.load_state_dict(_sd(gold, "a"))
        m = m.cuda().eval()
        base = m.infer(mel, sigma=0.0)
        assert torch.equal(base, a0)
        kept = m.WN[0].end.bias.detach().clone()
        m.WN[0].end.bias.data += 0.25
        assert torch.equal(m.infer(mel, sigma=0.0), base)         # .data edits are invisible to the version counters
        changed = m.repack().infer(mel, sigma=0.0)
        assert float((changed - base).abs().max()) > 1e-3
        with torch.no_grad():
            m.WN[0].end.bias.copy_(kept)                          # an edit autograd sees: repacked without being asked
        assert torch.equal(m.infer(mel, sigma=0.0), base)
