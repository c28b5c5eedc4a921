"""GPU checks of the HiFi-GAN multi-period discriminator (``DiscriminatorP`` / ``MultiPeriodDiscriminator``, csrc/vocoder_disc.hip)
and the three GAN losses, at the reference's full widths: feature maps, scores and the gradient of every parameter and of both
audios against the recording of the reference's own MultiPeriodDiscriminator under torch's autograd on the CPU
(tests/golden/hifigan_disc.npz) and against fp64 autograd over tests/hifigan_disc_ref.py, at every edge length of
hifigan_disc_ref.edge_lengths; the two real recipes, batching, determinism, three SGD steps, the surface, and the whole GAN step's
plumbing behind ``Generator.trainable()``.

Every tensor, forward or gradient, is held to 25 * max(the fp32 CPU run's own max deviation from fp64 on that tensor,
2^-23 * max |x64|), the bound test_gpu_hifigan_train.py and test_gpu_waveglow_backward.py state, and max |g64| > 0 is asserted
for every gradient tensor.  The upstream of the gradient tests is a seeded random weight on every feature map and on the score.
No test calls torch's convolution library on the GPU: every reference is computed on the CPU.

The tile-edge lengths: no period divides 127, only 2 divides 128 and only 3 divides 129, so per period conv 1's N = H * p takes
the nearest multiples of p on both sides of the 128-column tile (and 128, 129 themselves at p = 2, 3): edge_lengths says which, the
plan test pins them.  Audio comes from make_clean_audio: seeds whose fp64 run keeps every pre-activation 2e-6 clear of zero, where
lrelu' jumps and a gradient is decided by rounding (the reasoning stands there)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hifigan_disc_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP = 2.0 ** -23
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "hifigan_disc.npz"))
    out = {k: z[k] for k in z.files}
    out["seeds"], out["keys"] = json.loads(str(z["seeds"])), json.loads(str(z["keys"]))
    return out


_CACHE = {}


def _sd(gold):
    if "sd" not in _CACHE:
        _CACHE["sd"] = R.make_state_dict(gold["seeds"]["weights"])
    return _CACHE["sd"]


def _mpd(gold):
    """One MultiPeriodDiscriminator on the GPU with the recording's weights; tests that step the parameters make their own."""
    if "mpd" not in _CACHE:
        _CACHE["mpd"] = _fresh_mpd(_sd(gold))
    for p in _CACHE["mpd"].parameters():
        p.requires_grad_(True)
    _CACHE["mpd"].zero_grad(set_to_none=True)
    return _CACHE["mpd"]


def _fresh_mpd(sd):
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import MultiPeriodDiscriminator
    mpd = MultiPeriodDiscriminator()
    mpd.load_state_dict(sd, strict=True)
    return mpd.cuda()


def _case(gold, n):
    """Case n of the recording, its fp64 gradients and forward computed once."""
    if ("case", n) not in _CACHE:
        B, T = (int(v) for v in gold["cases"][n])
        y, y_hat, ups = R.mpd_inputs(_sd(gold), gold["seeds"], n, B, T)
        g64, _, o64 = R.autograd(_sd(gold), y, y_hat, F64, lambda o: R.mpd_total(o, ups))
        _CACHE["case", n] = (y, y_hat, ups, g64, o64)
    return _CACHE["case", n]


def _held(tag, name, got, ref, dev, sub=None):
    """max |got - ref| of a finite tensor of ref's shape; sub: ref is the flattened tensor at that stride.  _ratio puts it over the bound."""
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), (tag, name)
    if sub is not None:
        got = got.flatten()[::sub]
    assert got.shape == ref.shape, (tag, name, got.shape, ref.shape)
    return float((got - ref.double()).abs().max())


def _ratio(err, dev, mag):
    return err / (25 * max(dev, ULP * mag))


def _cuda_ups(ups):
    return [u.cuda() for u in ups]


# ----------------------------------------------------------------------------------------------------------------------
# 1, 2: the recording and fp64
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1])
def test_forward_vs_recording_and_fp64(gold, n):
    """The four returned lists, every shape, and every feature map and score against fp64 and against the reference's own fp32 values."""
    y, y_hat, _, _, o64 = _case(gold, n)
    B = y.shape[0]
    with torch.no_grad():
        outs = _mpd(gold)(y.cuda(), y_hat.cuda())
    assert len(outs) == 4 and all(isinstance(o, list) and len(o) == len(R.PERIODS) for o in outs)
    keep, worst, i = int(gold["fmap_keep"]), [0.0, 0.0], 0
    for d, p in enumerate(R.PERIODS):
        for side, score, fmap, s64, f64 in (("r", outs[0][d], outs[2][d], o64[0][d], o64[2][d]), ("g", outs[1][d], outs[3][d], o64[1][d], o64[3][d])):
            assert len(fmap) == R.N_LAYERS and score.shape == s64.shape == (B, R.rows(p, y.shape[2])[6] * p)
            assert torch.equal(score, torch.flatten(fmap[-1], 1, -1)) and score.grad_fn is None
            for l, (a, b) in enumerate(zip(fmap, f64)):
                dev, mag = float(gold[f"fdev{n}"][i]), float(gold[f"fmag{n}"][i])
                assert a.shape == b.shape and abs(float(b.abs().max()) - mag) <= 1e-6 * mag      # the same weights and audio as the recording
                rec = torch.from_numpy(gold[f"f{n}/{d}/{side}/{l}"])
                sub = 1 if l == 5 else max(1, -(-a.numel() // keep))
                r64, rrec = _ratio(_held("fmap", (d, side, l), a, b, dev), dev, mag), _ratio(_held("fmap", (d, side, l), a, rec, dev, sub), dev, mag)
                worst = [max(worst[0], r64), max(worst[1], rrec)]
                assert r64 <= 1.0 and rrec <= 1.0, (d, side, l, r64, rrec)
                i += 1
    print(f"forward case {n}: worst err/bound vs fp64 {worst[0]:.3f}, vs the recording {worst[1]:.3f}")


@pytest.mark.parametrize("n", [0, 1])
def test_gradients_vs_recording_and_fp64(gold, n):
    """All 90 parameters and both audios through MultiPeriodDiscriminator(y, y_hat), a random weight on every feature map and score."""
    y, y_hat, ups, g64, _ = _case(gold, n)
    mpd = _mpd(gold)
    yc, hc = y.cuda().requires_grad_(True), y_hat.cuda().requires_grad_(True)
    R.mpd_total(mpd(yc, hc), [(_cuda_ups(a), _cuda_ups(b)) for a, b in ups]).backward()
    got = {k: p.grad for k, p in mpd.named_parameters()}
    got["y"], got["y_hat"] = yc.grad, hc.grad
    assert list(got) == gold["keys"] and sorted(got) == sorted(g64)
    stride, worst = int(gold["grad_stride"]), [0.0, 0.0]
    for i, k in enumerate(gold["keys"]):
        dev, mag = float(gold[f"dev{n}"][i]), float(gold[f"mag{n}"][i])
        assert mag > 0 and abs(float(g64[k].abs().max()) - mag) <= 1e-6 * mag, k     # the weights are the recording's, and nothing passes by being zero
        r64 = _ratio(_held("grad", k, got[k], g64[k], dev), dev, mag)
        rrec = _ratio(_held("grad", k, got[k], torch.from_numpy(gold[f"g{n}/{k}"]), dev, stride), dev, mag)
        worst = [max(worst[0], r64), max(worst[1], rrec)]
        assert r64 <= 1.0 and rrec <= 1.0, (k, r64, rrec)
    print(f"gradients case {n}: {len(got)} tensors, worst err/bound vs fp64 {worst[0]:.3f}, vs the recording {worst[1]:.3f}")


def _disc_step(disc, x, ups):
    """One forward + backward of weighted_sum through one DiscriminatorP: ({short key: grad}, score, fmap)."""
    disc.zero_grad(set_to_none=True)
    xc = x.cuda().requires_grad_(True)
    score, fmap = disc(xc)
    assert score.grad_fn is not None
    R.weighted_sum(score, fmap, _cuda_ups(ups)).backward()
    got = {k: p.grad.detach().clone() for k, p in disc.named_parameters()}
    got["x"] = xc.grad.detach().clone()
    return got, score.detach(), [f.detach() for f in fmap]


EDGES = [(d, what) for d, p in enumerate(R.PERIODS) for what in R.edge_lengths(p)]


@pytest.mark.parametrize("d,what", EDGES, ids=[f"p{R.PERIODS[d]}-{w}" for d, w in EDGES])
def test_edge_lengths_forward_and_gradients_vs_fp64(gold, d, what):
    """One DiscriminatorP over 2B items at each length that can break a mechanism (reflect pad, stride phases, tile edges, several
    tiles, one- and two-row tails): every feature map, the score, the 18 parameter gradients and the audio's against fp64."""
    p = R.PERIODS[d]
    B, T = R.edge_lengths(p)[what]
    sd, seed = _sd(gold), 7000 + 100 * d + sorted(R.edge_lengths(p)).index(what)
    x = R.make_clean_audio(sd, [d], 2 * B, T, seed)
    ups = R.make_upstream(p, 2 * B, T, seed + 50)
    g64, s64, f64 = R.disc_grads(sd, d, p, x, ups, F64)
    g32, s32, f32 = R.disc_grads(sd, d, p, x, ups, F32)
    got, score, fmap = _disc_step(_mpd(gold).discriminators[d], x, ups)
    prefix = f"discriminators.{d}."
    assert sorted(prefix + k if k != "x" else k for k in got) == sorted(g64)
    assert [tuple(f.shape) for f in fmap] == [tuple(f.shape) for f in f64] and torch.equal(score, torch.flatten(fmap[-1], 1, -1))
    wf = wg = 0.0
    for l, (a, b, c) in enumerate(zip(fmap, f64, f32)):
        dev, mag = float((c.double() - b).abs().max()), float(b.abs().max())
        r = _ratio(_held(what, l, a, b, dev), dev, mag)
        wf = max(wf, r)
        assert r <= 1.0, ("fmap", l, r)
    for k, ref in g64.items():
        dev, mag = float((g32[k].double() - ref).abs().max()), float(ref.abs().max())
        assert mag > 0, k
        r = _ratio(_held(what, k, got[k[len(prefix):] if k != "x" else k], ref, dev), dev, mag)
        wg = max(wg, r)
        assert r <= 1.0, (k, r)
    print(f"edge p={p} {what} 2B={2 * B} T={T} rows {R.rows(p, T)}: worst err/bound forward {wf:.3f}, gradients {wg:.3f}")


# ----------------------------------------------------------------------------------------------------------------------
# 3: the two real recipes
# ----------------------------------------------------------------------------------------------------------------------
def _loss_held(got, l64, l32):
    """A scalar against fp64 within 25 * max(the fp32 CPU run's deviation, 2^-23 * |fp64|)."""
    assert abs(got - l64) <= 25 * max(abs(l32 - l64), ULP * abs(l64)), (got, l64, l32)


def _real_term(scores, d):
    return float(((1 - scores[d]) ** 2).mean())


def _generated_term(scores, d):
    return float((scores[d] ** 2).mean())


def test_discriminator_step_with_y_hat_detached(gold):
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import discriminator_loss
    y, y_hat, _, _, _ = _case(gold, 1)
    sd, mpd = _sd(gold), _mpd(gold)
    g64, l64, o64 = R.autograd(sd, y, y_hat, F64, R.discriminator_side_loss)
    g32, l32, o32 = R.autograd(sd, y, y_hat, F32, R.discriminator_side_loss)
    hc = y_hat.cuda().requires_grad_(True)
    y_d_rs, y_d_gs, _, _ = mpd(y.cuda(), hc.detach())
    loss, r_losses, g_losses = discriminator_loss(y_d_rs, y_d_gs)
    loss.backward()
    assert hc.grad is None
    _loss_held(float(loss.detach()), l64, l32)
    assert len(r_losses) == len(g_losses) == 5 and all(isinstance(v, float) for v in r_losses + g_losses)
    for d in range(5):                                         # every entry of the returned lists, by the rule of the total
        _loss_held(r_losses[d], _real_term(o64[0], d), _real_term(o32[0], d))
        _loss_held(g_losses[d], _generated_term(o64[1], d), _generated_term(o32[1], d))
    worst = 0.0
    for k, p in mpd.named_parameters():
        dev, mag = float((g32[k].double() - g64[k]).abs().max()), float(g64[k].abs().max())
        assert mag > 0, k
        worst = max(worst, _ratio(_held("d-step", k, p.grad, g64[k], dev), dev, mag))
    print(f"discriminator step: loss {float(loss.detach())} (fp64 {l64}), worst gradient err/bound {worst:.3f}")
    assert worst <= 1.0


def test_generator_step_gradient_to_y_hat_only(gold):
    """feature_loss + generator_loss: the loss against the CPU reference, no parameter gradient where none is asked for, and d y_hat
    with the bits of the full backward.  d y_hat's values are not held against fp64 here: |r - g| has a kink wherever a real and a
    generated feature-map value coincide, these maps hold about ten pairs nearer than 2e-6 at any length (the compressed negative
    side of the leaky ReLU), and there sign(r - g) * 2 / numel is decided by rounding.  The data gradients' values are held by the
    weighted-sum tests above, whose upstream has no kink."""
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import feature_loss, generator_loss
    y, y_hat, _, _, _ = _case(gold, 1)
    sd, mpd = _sd(gold), _mpd(gold)
    g64, l64, o64 = R.autograd(sd, y, y_hat, F64, R.generator_side_loss, wrt_params=False)
    g32, l32, o32 = R.autograd(sd, y, y_hat, F32, R.generator_side_loss, wrt_params=False)

    def run():
        hc = y_hat.cuda().requires_grad_(True)
        _, y_d_gs, fmap_rs, fmap_gs = mpd(y.cuda(), hc)
        loss_gen, gen_losses = generator_loss(y_d_gs)
        assert len(gen_losses) == 5 and all(torch.is_tensor(v) for v in gen_losses)
        for d in range(5):                                     # every entry of the returned list, by the rule of the total
            _loss_held(float(gen_losses[d].detach()), _real_term(o64[1], d), _real_term(o32[1], d))
        loss = feature_loss(fmap_rs, fmap_gs) + loss_gen
        loss.backward()
        return float(loss.detach()), hc.grad

    full_loss, full = run()                                    # as the reference's loop runs it: the parameters get gradients too
    assert all(p.grad is not None for p in mpd.parameters())
    mpd.zero_grad(set_to_none=True)
    for p in mpd.parameters():
        p.requires_grad_(False)
    only_loss, only = run()
    assert all(p.grad is None for p in mpd.parameters())
    assert torch.equal(only, full) and only_loss == full_loss
    _loss_held(only_loss, l64, l32)
    assert float(g64["y_hat"].abs().max()) > 0 and float(only.abs().max()) > 0 and torch.isfinite(only).all()
    print(f"generator step: loss {only_loss} (fp64 {l64}, fp32 CPU {l32})")


# ----------------------------------------------------------------------------------------------------------------------
# 4, 5: batching and determinism
# ----------------------------------------------------------------------------------------------------------------------
def test_an_item_has_the_bits_of_its_run_alone(gold):
    sd, mpd = _sd(gold), _mpd(gold)
    y, y_hat = R.make_audio(3, 1000, 61).cuda(), R.make_audio(3, 1000, 62).cuda()
    with torch.no_grad():
        _, _, fmap_rs, fmap_gs = mpd(y, y_hat)
        for d, disc in enumerate(mpd.discriminators):
            for x, maps in ((y, fmap_rs[d]), (y_hat, fmap_gs[d])):
                score, alone = disc(x)
                assert all(torch.equal(a, b) for a, b in zip(alone, maps)) and torch.equal(score, torch.flatten(maps[-1], 1, -1))
                for b in range(3):
                    _, item = disc(x[b:b + 1])
                    assert all(torch.equal(a[0], m[b]) for a, m in zip(item, maps)), (d, b)


def test_an_item_has_the_gradient_bits_of_its_run_alone(gold):
    """The backward per item: conv_post's and the GEMM data gradients and the audio's gather never mix items, so the audio gradient
    of item b inside a batch of three has the bits of the item run alone under its own slice of the upstream."""
    mpd = _mpd(gold)
    x = R.make_audio(3, 1000, 63)
    for d, disc in enumerate(mpd.discriminators):
        ups = R.make_upstream(disc.period, 3, 1000, 640 + d)
        batch, _, _ = _disc_step(disc, x, ups)
        assert float(batch["x"].abs().max()) > 0
        for b in range(3):
            item, _, _ = _disc_step(disc, x[b:b + 1], [u[b:b + 1] for u in ups])
            assert torch.equal(item["x"][0], batch["x"][b]), (d, b)


def test_two_runs_give_the_same_bits(gold):
    y, y_hat, ups, _, _ = _case(gold, 1)
    mpd = _mpd(gold)
    cu = [(_cuda_ups(a), _cuda_ups(b)) for a, b in ups]

    def run():
        mpd.zero_grad(set_to_none=True)
        yc, hc = y.cuda().requires_grad_(True), y_hat.cuda().requires_grad_(True)
        outs = mpd(yc, hc)
        R.mpd_total(outs, cu).backward()
        return [f.detach() for part in outs[2:] for maps in part for f in maps] + [p.grad.clone() for p in mpd.parameters()] + [yc.grad, hc.grad]

    a, b = run(), run()
    assert len(a) == 60 + 90 + 2 and all(torch.equal(u, v) for u, v in zip(a, b))


# ----------------------------------------------------------------------------------------------------------------------
# 6: three SGD steps
# ----------------------------------------------------------------------------------------------------------------------
SGD_LR = 1e-3


def test_three_sgd_steps_of_the_discriminator_loss_follow_the_fp64_run(gold):
    """p -= lr * grad of discriminator_loss, three times, on the weight-normed parameters: every forward packs the parameters as they
    are, so stale packed weights cannot pass.  The loss before every step and after the last and every parameter at the end stay
    within 25 times the fp32 CPU run's deviation from the fp64 run of the same steps, floored at 2^-23 * the loss and 2^-23 * max |p64|."""
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import discriminator_loss
    sd = _sd(gold)
    y, y_hat = R.make_audio(1, 300, 71), R.make_audio(1, 300, 72)
    l64, p64 = R.sgd_steps(sd, y, y_hat, F64, SGD_LR, 3)
    l32, p32 = R.sgd_steps(sd, y, y_hat, F32, SGD_LR, 3)
    assert l64[3] < l64[2] < l64[1] < l64[0] and l64[0] - l64[3] > 0.01 * l64[0]
    mpd, got = _fresh_mpd(sd), []
    for _ in range(3):
        mpd.zero_grad(set_to_none=True)
        loss = discriminator_loss(*mpd(y.cuda(), y_hat.cuda())[:2])[0]
        loss.backward()
        got.append(float(loss.detach()))
        with torch.no_grad():
            for p in mpd.parameters():
                p -= SGD_LR * p.grad
    with torch.no_grad():
        got.append(float(discriminator_loss(*mpd(y.cuda(), y_hat.cuda())[:2])[0]))
    print("loss fp64", l64, "fp32 CPU", l32, "GPU", got)
    assert got[3] < got[2] < got[1] < got[0]
    for a, b, c in zip(got, l64, l32):
        assert abs(a - b) <= 25 * max(abs(c - b), ULP * abs(b))
    worst = 0.0
    for k, p in mpd.state_dict().items():
        bound = 25 * max(float((p32[k].double() - p64[k]).abs().max()), ULP * float(p64[k].abs().max()))
        worst = max(worst, float((p.cpu().double() - p64[k]).abs().max()) / bound)
    print("parameters after three steps, worst err/bound", worst)
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# 7, 8: the surface and the GAN step's plumbing
# ----------------------------------------------------------------------------------------------------------------------
def test_surface(gold):
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import DiscriminatorP, MultiPeriodDiscriminator
    sd = _sd(gold)
    mpd = MultiPeriodDiscriminator()
    assert list(mpd.state_dict()) == list(sd) and [tuple(v.shape) for v in mpd.state_dict().values()] == [tuple(v.shape) for v in sd.values()]
    mpd.load_state_dict(sd, strict=True)
    assert [d.period for d in mpd.discriminators] == list(R.PERIODS)
    with pytest.raises(NotImplementedError, match="multi-scale discriminator"):
        DiscriminatorP(2, use_spectral_norm=True)
    with pytest.raises(NotImplementedError, match="multi-scale discriminator"):
        DiscriminatorP(2, kernel_size=3)
    with pytest.raises(NotImplementedError, match="multi-scale discriminator"):
        DiscriminatorP(2, stride=2)
    y = R.make_audio(2, 257, 81)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        mpd.cuda()(y, y)
    with pytest.raises(RuntimeError, match="too short for period"):
        mpd.discriminators[4](R.make_audio(1, 5, 82).cuda())
    with torch.no_grad():                                      # the no-grad path keeps nothing
        outs = mpd(y.cuda(), y.cuda())
    assert all(f.grad_fn is None and not f.requires_grad for part in outs[2:] for maps in part for f in maps)
    for p in mpd.parameters():
        p.requires_grad_(False)
    score, fmap = mpd.discriminators[0](y.cuda())             # nothing asks for a gradient
    assert score.grad_fn is None and tuple(score.shape) == (2, R.rows(2, 257)[6] * 2)
    assert all(torch.equal(a, b) for a, b in zip(fmap, [m[:2] for m in outs[2][0]]))


def test_gan_step_end_to_end_has_the_bits_of_the_two_graph_version(gold):
    """Plumbing only: Generator.trainable() -> y_hat -> MultiPeriodDiscriminator -> generator_loss + feature_loss + 45 * L1(mel), one
    backward; every generator parameter gets a finite non-zero gradient with the bits of the two-graph version cut at y_hat."""
    import hifigan_ref as HR
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import Generator, feature_loss, generator_loss
    from tacotron2_subword_amd.utils import mel_spectrogram_from_audio
    cfg = json.loads(str(np.load(os.path.join(GOLDEN, "hifigan.npz"))["configs"]))["rb2"]
    h = HR.H(cfg)
    gen = Generator(h)
    gen.load_state_dict(HR.calibrate(HR.make_state_dict(h, 3101), h, HR.make_mel(2, 16, 3201)))
    gen = gen.cuda().trainable()
    mpd = _mpd(gold)
    mel = HR.make_mel(2, 33, 91).cuda()
    y = R.make_audio(2, 33 * 32, 92).cuda()
    with torch.no_grad():
        target = mel_spectrogram_from_audio(y.squeeze(1))

    def loss_of(y_hat):
        _, y_d_gs, fmap_rs, fmap_gs = mpd(y, y_hat)
        mel_term = F.l1_loss(mel_spectrogram_from_audio(y_hat.squeeze(1), differentiable=True), target) * 45
        return generator_loss(y_d_gs)[0] + feature_loss(fmap_rs, fmap_gs) + mel_term

    gen.zero_grad(set_to_none=True)
    loss_of(gen(mel)).backward()
    one = {k: p.grad.clone() for k, p in gen.named_parameters()}
    gen.zero_grad(set_to_none=True)
    y_hat = gen(mel)
    cut = y_hat.detach().requires_grad_(True)
    loss_of(cut).backward()
    y_hat.backward(cut.grad)
    assert float(cut.grad.abs().max()) > 0
    for k, p in gen.named_parameters():
        assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 and torch.equal(p.grad, one[k]), k
