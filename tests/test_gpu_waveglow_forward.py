"""GPU checks of WaveGlow's forward direction (csrc/waveglow.hip: audio -> z, log_s, log det W and the negative
log-likelihood): WaveGlow.analyze / nll / WaveGlowLoss against the vectors recorded from the reference's own forward and loss
(tests/golden/waveglow_forward.npz) and against the fp64 restatement (tests/waveglow_fwd_ref.py), the fixed-order fp64 sums, the
tail, head and logdet kernels on their own through the unit entry points, the round trip through infer, determinism and the
surface.

The tolerances are those of tests/test_gpu_waveglow.py: a chain of fmaf over k terms is held to 1e-6 * mag + 1e-7 per element
(mag = the same sum over absolute values in fp64), end to end the bound is 25 times the reference's own fp32 error on the same
inputs, recorded for z and for every flow's log_s of every case.  A sum that the kernels accumulate in fp64 is held to
2^-23 * sum |terms| of the fp64 sum of the kernel's own fp32 outputs: fewer than 2^24 terms cost under 2^-29 * sum |t|, plus
one rounding where the result is stored as fp32.  No test calls torch's convolution library on the GPU: every reference is
computed on the CPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import waveglow_fwd_ref as FR
import waveglow_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
ULP = 2.0 ** -23
CASES = [(1, 1, 8), (2, 4, 1024), (2, 4, 1500), (3, 2, 1027), (1, 5, 1021), (1, 1, 1024)]


def _L():
    from tacotron2_subword_amd import _lib as L
    return L


def _glow():
    from tacotron2_subword_amd.waveglow import glow
    return glow


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _check(tag, got, ref, bound):
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print(tag, "max err", float(err.max()), "worst err/bound", worst, "min bound", float(bound.min()))
    assert torch.isfinite(got).all()
    assert worst <= 1.0, tag


def _ramp(B, Cch, Lt):
    """A ramp in time times a per-channel sign and a per-item gain: a swapped row or a neighbouring item cannot pass."""
    t = torch.arange(Lt, dtype=torch.float64)
    sign = torch.tensor([1.0 if (c * 5 + 1) % 3 else -1.0 for c in range(Cch)], dtype=torch.float64)
    return ((1.0 + t / Lt).view(1, 1, Lt) * sign.view(1, Cch, 1) * (1.0 + 0.25 * torch.arange(B, dtype=torch.float64)).view(B, 1, 1)).float()


# ------------------------------------------------------------------------------------------------------------------ the recording
@pytest.fixture(scope="module")
def gold():
    z, base = np.load(os.path.join(GOLDEN, "waveglow_forward.npz")), np.load(os.path.join(GOLDEN, "waveglow.npz"))
    out = {k: z[k] for k in z.files}
    out["base"], out["configs"] = {k: base[k] for k in base.files}, json.loads(str(base["configs"]))
    assert [tuple(int(v) for v in c) for c in out["cases"]] == CASES
    return out


def _sd(gold, tag):
    base = gold["base"]
    sd = {k: torch.from_numpy(base[k if k.startswith("upsample.") else f"{tag}/{k}"]) for k in json.loads(str(base[f"{tag}_keys"]))}
    return {k: torch.from_numpy(gold[f"{tag}/{k}"]) if k.startswith("convinv.") else v for k, v in sd.items()}


def _inputs(gold, n):
    return torch.from_numpy(gold[f"mel{n}"]), torch.from_numpy(gold[f"audio{n}"])


@pytest.fixture(scope="module")
def models(gold):
    """{tag: (cfg, weight-normed module, module after remove_weightnorm)} on the GPU, with the recording's skewed mixes."""
    glow, out = _glow(), {}
    for tag, cfg in gold["configs"].items():
        pair = []
        for removed in (False, True):
            m = glow.WaveGlow(**cfg)
            m.load_state_dict(_sd(gold, tag))
            if removed:
                glow.WaveGlow.remove_weightnorm(m)
            pair.append(m.cuda().eval())
        out[tag] = (cfg, *pair)
    return out


@pytest.fixture(scope="module")
def refs(gold):
    """{(tag, n): (z, log_s, logdet per matrix)} of the fp64 restatement, computed once and left unchanged."""
    out = {}
    for tag, cfg in gold["configs"].items():
        folded = R.fold(_sd(gold, tag))
        for n in range(len(CASES)):
            out[tag, n] = FR.forward(folded, cfg, *_inputs(gold, n))
    return out


@pytest.mark.parametrize("tag", ["a", "deep"])
def test_analyze_and_nll_vs_reference_recording(gold, models, refs, tag):
    cfg, normed, removed = models[tag]
    glow = _glow()
    with torch.no_grad():
        for n, (B, T, N) in enumerate(CASES):
            mel, audio = (_d(t) for t in _inputs(gold, n))
            z, log_s, logdet = normed.analyze((mel, audio))
            z2, log_s2, logdet2 = removed.analyze((mel, audio))
            L = N // cfg["n_group"]
            assert z.shape == (B, cfg["n_group"], L) and z.dtype == torch.float32 and len(log_s) == len(logdet) == cfg["n_flows"]
            assert [tuple(t.shape) for t in log_s] == [(B, c // 2, L) for c in R.flow_channels(cfg)]
            assert all(t.dim() == 0 and t.dtype == torch.float32 and t.is_cuda for t in logdet)
            assert torch.equal(z, z2) and all(torch.equal(a, b) for a, b in zip(log_s + logdet, log_s2 + logdet2))     # weight-normed and folded
            z64, s64, ld64 = refs[tag, n]
            zerr, zref = float((z.cpu().double() - torch.from_numpy(gold[f"{tag}_z{n}"]).double()).abs().max()), float(gold[f"{tag}_z_err{n}"])
            serr = [float((a.cpu().double() - torch.from_numpy(gold[f"{tag}_log_s{n}_{k}"]).double()).abs().max()) for k, a in enumerate(log_s)]
            sref = [float(v) for v in gold[f"{tag}_log_s_err{n}"]]
            print(tag, (B, T, N), "z err", zerr, "reference's own", zref, "ratio", zerr / zref, "log_s err per flow", serr, "reference's own", sref,
                  "worst ratio", max(e / r for e, r in zip(serr, sref)))
            assert torch.isfinite(z).all() and zerr <= 25 * zref
            assert all(e <= 25 * r for e, r in zip(serr, sref))
            for k in range(cfg["n_flows"]):
                ref = B * L * float(ld64[k])
                print("  log det W", k, float(logdet[k]), "fp64", ref)
                assert abs(float(logdet[k]) - ref) <= 1e-6 * abs(ref) + 1e-7
            for si, sigma in enumerate(float(s) for s in gold["sigmas"]):
                ref = float(FR.loss(z64, s64, ld64, sigma))
                bound = 25 * max(float(gold[f"{tag}_loss_err{n}"][si]), ULP * FR.loss_magnitude(z64, s64, ld64, sigma))
                from_tuple = float(glow.WaveGlowLoss(sigma)((z, log_s, logdet)))
                from_sums = normed.nll(mel, audio, sigma=sigma)
                assert from_sums.dim() == 0 and from_sums.dtype == torch.float32 and from_sums.is_cuda
                print("  sigma", sigma, "loss fp64", ref, "WaveGlowLoss(analyze)", from_tuple, "nll", float(from_sums), "recorded",
                      float(gold[f"{tag}_loss{n}"][si]), "bound", bound)
                assert abs(from_tuple - ref) <= bound and abs(float(from_sums) - ref) <= bound
                assert torch.equal(from_sums, removed.nll(mel, audio, sigma=sigma))


# ------------------------------------------------------------------------------------------------------------------ the sums
@pytest.mark.parametrize("tag, n", [("a", 0), ("deep", 2), ("deep", 3)])
def test_sums_vs_fp64_sums_of_the_kernels_own_outputs(gold, models, tag, n):
    cfg, model, _ = models[tag]
    mel, audio = (_d(t) for t in _inputs(gold, n))
    sigma = 0.7
    with torch.no_grad():
        z, log_s, logdet, info = model.analyze_debug((mel, audio), sigma=sigma)
        items, scalar = model.nll(mel, audio, sigma=sigma, per_item=True), model.nll(mel, audio, sigma=sigma)
    B, G, L = z.shape
    sums = info["sums"].cpu()
    assert sums.shape == (B, cfg["n_flows"] + 1) and sums.dtype == torch.float64
    for k, s in enumerate(log_s):
        s = s.cpu().double().flatten(1)
        _check(f"sum log_s {k}", sums[:, k], s.sum(1), ULP * s.abs().sum(1) + 1e-300)
    z2 = z.cpu().double().flatten(1) ** 2
    _check("sum z^2", sums[:, -1], z2.sum(1), ULP * z2.sum(1) + 1e-300)
    assert float(sums[:, -1].min()) > 0
    # the per-item values and the scalar, from the kernel's own outputs in fp64
    ld = torch.stack(logdet).cpu().double() / (B * L)
    zc, sc = z.cpu(), [t.cpu() for t in log_s]
    ref_items = FR.nll_items(zc, sc, ld, sigma)
    mags = torch.tensor([FR.loss_magnitude(zc[b:b + 1], [t[b:b + 1] for t in sc], ld, sigma) for b in range(B)], dtype=torch.float64)
    assert items.shape == (B,) and items.dtype == torch.float32
    assert torch.equal(items, info["nll_item"]) and torch.equal(scalar, info["loss"])
    _check("nll per item", items.cpu(), ref_items, ULP * mags)
    bound = ULP * float(mags.max())
    print("scalar", float(scalar), "mean of the items", float(items.double().mean()), "fp64", float(ref_items.mean()), "bound", bound)
    assert abs(float(items.double().mean()) - float(scalar)) <= bound
    assert abs(float(scalar) - float(ref_items.mean())) <= bound


# ------------------------------------------------------------------------------------------------------------------ the tail kernel
@pytest.mark.parametrize("n_half, n_peel, nc, Lt, B, identity", [(4, 0, 8, 1, 1, True), (4, 2, 256, 257, 2, False), (3, 0, 24, 300, 1, True),
                                                                 (3, 2, 16, 255, 3, False), (2, None, 256, 40, 1, False), (1, None, 8, 513, 2, False)])
def test_tail_vs_fp64(n_half, n_peel, nc, Lt, B, identity):
    """(b, s) = end(out) are chains over nc: e = 1e-6 * mag + 1e-7 each.  a1' = exp(s) * a1 + b is held to
    e_b + exp(s) * |a1| * (e_s + 2 ulp) + ulp * |a1'|: the error of b, what the error of s does to exp(s) to first order, 2 ulp
    for expf and the product's rounding, one for the sum's.  a0 passes through untouched, so whatever is peeled from it lands in
    z bit for bit.  With W = I the mix returns its input exactly; otherwise it carries those errors through |W| and adds a
    chain's 1e-6 * mag + 1e-7.  n_peel None: the last flow, all of cat(a0, a1') goes to z."""
    L = _L()
    g = torch.Generator().manual_seed(n_half * 1000 + nc + Lt)
    c, G = 2 * n_half, 8
    last = n_peel is None
    n_peel = c if last else n_peel
    cn, zoff = c - n_peel, G - c if last else 2
    out = _ramp(B, nc, Lt) * 0.5
    w_end, b_end = torch.randn(c, nc, generator=g) * 0.5 * nc ** -0.5, torch.randn(c, generator=g) * 0.1
    audio = torch.randn(B, c, Lt, generator=g)
    W = None if last else (torch.eye(cn) if identity else (torch.linalg.qr(torch.randn(cn, cn, generator=g))[0] * (0.5 + 1.5 * torch.rand(cn, generator=g))).contiguous())
    nblk = (Lt + 255) // 256
    dst = None if last else torch.full((B, cn, Lt), float("nan"), device=DEV)
    z = torch.full((B, G, Lt), float("nan"), device=DEV)
    log_s = torch.full((B, n_half, Lt), float("nan"), device=DEV)
    part_s, part_z = (torch.full((B, nblk), float("nan"), device=DEV, dtype=torch.float64) for _ in range(2))
    t = [_d(out), _d(w_end), _d(b_end), _d(audio), _d(W)]
    a = L.WaveglowTailArgs(B, nc, n_half, Lt, n_peel, G, zoff, *[L.ptr(v) for v in t], L.ptr(dst), L.ptr(z), L.ptr(log_s), L.ptr(part_s), L.ptr(part_z))
    L.check(L.lib().t2_waveglow_tail(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    z, log_s = z.cpu(), log_s.cpu()
    o = F.conv1d(out.double(), w_end.double()[:, :, None], b_end.double())
    e = 1e-6 * F.conv1d(out.double().abs(), w_end.double().abs()[:, :, None], b_end.double().abs()) + 1e-7
    b, s, e_b, e_s = o[:, :n_half], o[:, n_half:], e[:, :n_half], e[:, n_half:]
    assert 0.1 < float(s.abs().max()) < 3.0
    a0, a1 = audio[:, :n_half].double(), audio[:, n_half:].double()
    y1 = torch.exp(s) * a1 + b
    v = torch.cat([a0, y1], 1)
    e_v = torch.cat([torch.zeros_like(e_b), e_b + torch.exp(s) * a1.abs() * (e_s + 2 * ULP) + ULP * y1.abs()], 1)
    _check(f"log_s {(n_half, n_peel, nc, Lt, B)}", log_s, s, e_s)
    # z: the peeled channels at their offset, everything else untouched
    touched = torch.zeros(G, dtype=torch.bool)
    touched[zoff:zoff + n_peel] = True
    assert torch.isnan(z[:, ~touched]).all() and torch.isfinite(z[:, touched]).all()
    from_a0 = min(n_peel, n_half)
    assert torch.equal(z[:, zoff:zoff + from_a0], audio[:, :from_a0])                     # bit for bit
    if n_peel > n_half:
        _check("z from a1'", z[:, zoff + n_half:zoff + n_peel], v[:, n_half:n_peel], e_v[:, n_half:n_peel])
    if not last:
        rest, e_rest = v[:, n_peel:], e_v[:, n_peel:]
        if identity:
            ref, bound = rest, e_rest + 1e-30
        else:
            Wd = W.double()
            ref = torch.einsum("rc,bcl->brl", Wd, rest)
            bound = torch.einsum("rc,bcl->brl", Wd.abs(), e_rest) + 1e-6 * torch.einsum("rc,bcl->brl", Wd.abs(), rest.abs()) + 1e-7
        _check(f"tail {(n_half, n_peel, nc, Lt, B)}", dst.cpu(), ref, bound)
    # the partial sums, one per item and block of 256 columns, of the kernel's own outputs
    pad = nblk * 256 - Lt
    blocks = lambda x: F.pad(x.double(), (0, pad)).reshape(B, x.shape[1], nblk, 256).permute(0, 2, 1, 3).flatten(2)
    sb = blocks(log_s)
    _check("partial sums of s", part_s.cpu(), sb.sum(2), ULP * sb.abs().sum(2) + 1e-300)
    zb = blocks(z[:, touched]) ** 2 if n_peel else torch.zeros(B, nblk, 1, dtype=torch.float64)
    _check("partial sums of z^2", part_z.cpu(), zb.sum(2), ULP * zb.sum(2) + 1e-300)


# ------------------------------------------------------------------------------------------------------------------ the head kernel
@pytest.mark.parametrize("G", [2, 8])
@pytest.mark.parametrize("N", ["G", 8 * 256 + 5])
def test_head_regroup_and_mix(G, N):
    L = _L()
    N, B = G if N == "G" else N, 3
    Lt = N // G
    g = torch.Generator().manual_seed(G * 10 + N)
    audio = torch.randn(B, N, generator=g)
    regrouped = audio[:, :Lt * G].reshape(B, Lt, G).permute(0, 2, 1).contiguous()
    for W in (torch.eye(G), torch.randn(G, G, generator=g)):
        dst = torch.full((B, G, Lt), float("nan"), device=DEV)
        t = [_d(audio), _d(W)]
        a = L.WaveglowHeadArgs(B, G, N, L.ptr(t[0]), L.ptr(t[1]), L.ptr(dst))
        L.check(L.lib().t2_waveglow_head(C.byref(a), L.stream()))
        torch.cuda.synchronize()
        if torch.equal(W, torch.eye(G)):
            assert torch.equal(dst.cpu(), regrouped)                                         # exact, bit for bit
        else:
            ref = torch.einsum("rc,bcl->brl", W.double(), regrouped.double())
            _check(f"head {(G, N)}", dst.cpu(), ref, 1e-6 * torch.einsum("rc,bcl->brl", W.double().abs(), regrouped.double().abs()) + 1e-7)
    with pytest.raises(RuntimeError, match=f"n_samples={G - 1}"):
        a = L.WaveglowHeadArgs(B, G, G - 1, L.ptr(t[0]), L.ptr(t[1]), L.ptr(dst))
        L.check(L.lib().t2_waveglow_head(C.byref(a), L.stream()))


# ------------------------------------------------------------------------------------------------------------------ the logdet kernel
@pytest.mark.parametrize("c", [2, 4, 6, 8])
def test_logdet_vs_fp64(c):
    L = _L()
    g = torch.Generator().manual_seed(70 + c)
    mats = []
    for j in range(4):
        Q = torch.linalg.qr(torch.randn(c, c, generator=g))[0]
        if torch.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        mats.append(Q.clone())                                                               # orthonormal: log det = 0
        d = torch.exp((torch.rand(c, generator=g) * 2 - 1) * np.log(10.0))                  # condition <= 100
        mats.append(Q * d.view(1, c))
    negative = mats[1].clone()
    negative[0] = -negative[0]
    mats.append(negative)
    W = torch.stack(mats).contiguous()
    out = torch.full((len(mats),), 7.0, device=DEV)
    L.check(L.lib().t2_waveglow_logdet_matrices(L.ptr(_d(W)), c, len(mats), L.ptr(out), L.stream()))
    torch.cuda.synchronize()
    out = out.cpu()
    ref = torch.logdet(W.double())
    assert torch.isnan(ref[-1]) and torch.isnan(out[-1])                                  # a negative determinant, as torch.logdet
    assert float(torch.linalg.cond(W[:-1].double()).max()) <= 100.0 * (1 + 1e-6) and float(ref[:-1].abs().max()) > 0.5
    _check(f"logdet {c}", out[:-1], ref[:-1], 1e-6 * ref[:-1].abs() + 1e-7)


# ------------------------------------------------------------------------------------------------------------------ full width
@pytest.fixture(scope="module")
def full_width():
    """{nc: (cfg, state dict, module on the GPU)} at 80 mel channels, 12 flows, 8 layers, with skewed mixes; built once."""
    out = {}
    for nc in (256, 64):
        cfg = dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2, WN_config=dict(n_layers=8, n_channels=nc, kernel_size=3))
        sd = FR.skew_mixes(R.make_state_dict(cfg, 31 + nc), cfg, 5)
        model = _glow().WaveGlow(**cfg)
        model.load_state_dict(sd)
        out[nc] = (cfg, sd, model.cuda().eval())
    return out


@pytest.mark.parametrize("nc, B, T, N", [(256, 1, 2, 512), (64, 2, 3, 1003)])
def test_full_width_vs_fp64_restatement(full_width, nc, B, T, N):
    cfg, sd, model = full_width[nc]
    folded, mel = R.fold(sd), R.make_mel(B, T, 41)
    audio = torch.randn(B, N, generator=torch.Generator().manual_seed(47)) * 0.3
    z64, s64, ld64 = FR.forward(folded, cfg, mel, audio)
    z32, s32, ld32 = FR.forward(folded, cfg, mel, audio, dtype=torch.float32)
    sigma = 0.7
    zref, sref = float((z32.double() - z64).abs().max()), max(float((a.double() - b).abs().max()) for a, b in zip(s32, s64))
    loss64 = float(FR.loss(z64, s64, ld64, sigma))
    lref = abs(float(_glow().WaveGlowLoss(sigma)((z32, s32, [B * (N // 8) * t for t in ld32]))) - loss64)
    with torch.no_grad():
        z, log_s, logdet = model.analyze((_d(mel), _d(audio)))
        loss = float(model.nll(_d(mel), _d(audio), sigma=sigma))
        loss_tuple = float(_glow().WaveGlowLoss(sigma)((z, log_s, logdet)))
    zerr = float((z.cpu().double() - z64).abs().max())
    serr = max(float((a.cpu().double() - b).abs().max()) for a, b in zip(log_s, s64))
    print("channels", nc, "z std", float(z64.std()), "max |log_s|", max(float(t.abs().max()) for t in s64), "z err", zerr, "fp32 torch on the CPU vs fp64", zref,
          "log_s err", serr, "vs", sref, "loss", loss, loss_tuple, "fp64", loss64, "err", abs(loss - loss64), abs(loss_tuple - loss64), "vs", lref)
    assert z.shape == (B, 8, N // 8) and torch.isfinite(z).all() and max(float(t.abs().max()) for t in s64) > 0.1
    assert zerr <= 25 * zref and serr <= 25 * sref
    assert abs(loss - loss64) <= 25 * lref and abs(loss_tuple - loss64) <= 25 * lref


# ------------------------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("tag", ["a", "deep"])
def test_infer_undoes_analyze(gold, models, tag):
    """N = T * 256: z as noise at sigma = 1 gives the audio back, within 25 times what fp32 torch on the CPU loses on the same trip."""
    cfg, model, _ = models[tag]
    n = CASES.index((2, 4, 1024))
    mel, audio = _inputs(gold, n)
    folded = R.fold(_sd(gold, tag))
    z32 = FR.forward(folded, cfg, mel, audio, dtype=torch.float32)[0]
    back32 = R.infer(folded, cfg, mel, R.planes_from_z(cfg, z32), 1.0, dtype=torch.float32)
    ref_err = float((back32.double() - audio.double()).abs().max())
    with torch.no_grad():
        z = model.analyze((_d(mel), _d(audio)))[0]
        back = model.infer(_d(mel), 1.0, noise=R.planes_from_z(cfg, z))
    err = float((back.cpu().double() - audio.double()).abs().max())
    print(tag, "round trip err", err, "fp32 torch on the CPU", ref_err, "ratio", err / ref_err)
    assert back.shape == audio.shape and err <= 25 * ref_err


# ------------------------------------------------------------------------------------------------------------------ determinism
def test_same_bits_on_rerun_and_alone_vs_in_batch(gold, models):
    cfg, model, _ = models["deep"]
    B, T, N = 3, 3, 1500
    mel = R.make_mel(B, T, 7, n_mel=cfg["n_mel_channels"])
    audio = torch.randn(B, N, generator=torch.Generator().manual_seed(9)) * 0.3
    with torch.no_grad():
        runs = [model.analyze_debug((_d(mel), _d(audio)), sigma=0.7) for _ in range(2)]
        (z, log_s, logdet, info), (z2, log_s2, logdet2, info2) = runs
        assert torch.equal(z, z2) and all(torch.equal(a, b) for a, b in zip(log_s + logdet, log_s2 + logdet2))
        assert all(torch.equal(info[k], info2[k]) for k in ("loss", "nll_item", "sums"))
        assert torch.equal(model.nll(_d(mel), _d(audio), 0.7, per_item=True), info["nll_item"])
        for i in range(B):
            za, sa, _, ia = model.analyze_debug((_d(mel[i:i + 1]), _d(audio[i:i + 1])), sigma=0.7)
            assert torch.equal(za[0], z[i]) and all(torch.equal(a[0], b[i]) for a, b in zip(sa, log_s)), i
            assert torch.equal(ia["nll_item"][0], info["nll_item"][i]) and torch.equal(ia["sums"][0], info["sums"][i]), i
    assert float((z[0] - z[1]).abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------------------------ surface
def test_surface(gold, models):
    cfg, model, _ = models["a"]
    glow = _glow()
    mel = _d(R.make_mel(2, 3, 1, n_mel=8))
    audio = _d(torch.randn(2, 3 * 256 + 7, generator=torch.Generator().manual_seed(3)) * 0.3)
    with torch.no_grad():
        z, log_s, logdet = model.analyze((mel, audio))
        loss = model.nll(mel, audio)
    assert z.shape == (2, 8, 96) and z.is_cuda and not z.requires_grad and not loss.requires_grad
    with pytest.raises(RuntimeError, match="backward is not built"):
        model.analyze((mel, audio))
    with pytest.raises(RuntimeError, match="backward is not built"):
        model.nll(mel, audio)
    with torch.no_grad():
        assert torch.equal(z, model.analyze((mel, audio[:, :768].contiguous()))[0])           # a tail of N % n_group samples is dropped
        with pytest.raises(RuntimeError, match="backward is not built"):
            with torch.enable_grad():
                model.analyze((mel, audio.clone().requires_grad_()))
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            model.analyze((mel.cpu(), audio))
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            model.nll(mel, audio.cpu())
        with pytest.raises(RuntimeError, match=r"\[B, 8, T\]"):
            model.analyze((_d(R.make_mel(2, 3, 1, n_mel=80)), audio))
        with pytest.raises(RuntimeError, match=r"\[B, N\] with B = 2"):
            model.analyze((mel, audio[:1]))
        with pytest.raises(RuntimeError, match="float32"):
            model.analyze((mel.half(), audio))
        with pytest.raises(RuntimeError, match="float32"):
            model.analyze((mel, audio.double()))
        with pytest.raises(RuntimeError, match="n_samples=7 is shorter than one group of n_group=8"):
            model.analyze((mel, audio[:, :7].contiguous()))
        with pytest.raises(RuntimeError, match="n_samples=1537.*1536"):
            model.nll(mel, _d(torch.zeros(2, 2 * 256 + 1025)))
        with pytest.raises(RuntimeError, match="sigma=0"):
            model.nll(mel, audio, sigma=0)
        model.analyze((mel, _d(torch.zeros(2, 2 * 256 + 1024))))                                # the longest audio three frames take
        with pytest.raises(RuntimeError, match="inference only"):
            model((mel, audio))
        # an in-place edit that autograd sees is picked up; one behind its back needs repack()
        m = glow.WaveGlow(**cfg)
        m.load_state_dict(_sd(gold, "a"))
        m = m.cuda().eval()
        base = m.nll(mel, audio)
        assert torch.equal(base, loss)
        m.convinv[1].conv.weight.mul_(1.25)
        scaled = m.nll(mel, audio)
        assert not torch.equal(scaled, base)
        ld = m.analyze((mel, audio))[2][1]
        assert abs(float(ld) - (float(logdet[1]) + 2 * 96 * 8 * np.log(1.25))) <= 1e-6 * abs(float(ld)) + 1e-4
        m.WN[0].end.bias.data.add_(0.01)
        assert torch.equal(m.nll(mel, audio), scaled)
        m.repack()
        assert not torch.equal(m.nll(mel, audio), scaled)
        # both directions keep their own buffer, and a pickle carries neither
        m.infer(mel, sigma=0.0)
        assert m._packed is not m._packed_fwd and m._packed.shape == m._packed_fwd.shape and not torch.equal(m._packed, m._packed_fwd)
        assert not any(k in m.__getstate__() for k in glow._CACHES)
