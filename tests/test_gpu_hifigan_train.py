"""GPU checks of HiFi-GAN generator training end to end (``Generator.trainable()``, csrc/vocoder_bwd.hip): ``.grad`` of every
parameter and of the mel against the gradients recorded from the reference's own Generator under torch's autograd on the CPU
(tests/golden/hifigan_grad.npz) and against an fp64 autograd pass over tests/hifigan_ref._walk (tests/hifigan_grad_ref.py);
weight-normed and folded, a general upstream gradient, config_v1 at full width, three SGD steps, the mel-L1 recipe's plumbing,
determinism and the surface with and without the opt-in.

A gradient tensor is held to 25 * max(the fp32 CPU autograd's own max deviation from fp64 on that tensor, 2^-23 * max |g64|), the
bound test_gpu_waveglow_backward.py states, and max |g64| > 0 is asserted for every tensor.  No test calls torch's convolution
library on the GPU: every reference is computed on the CPU."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hifigan_grad_ref as GR
import hifigan_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "hifigan_grad.npz"))
    out = {k: z[k] for k in z.files}
    out["configs"] = json.loads(str(np.load(os.path.join(GOLDEN, "hifigan.npz"))["configs"]))
    out["seeds"] = json.loads(str(z["seeds"]))
    return out


_SD = {}


def _setup(gold, tag):
    """(h, the weight-normed state dict) of generator `tag`, made again from the recording's seeds."""
    if tag not in _SD:
        gi, seeds = list(gold["configs"]).index(tag), gold["seeds"]
        h = R.H(gold["configs"][tag])
        _SD[tag] = (h, R.calibrate(R.make_state_dict(h, seeds["weights"] + gi), h, R.make_mel(2, 16, seeds["calibrate_mel"] + gi)))
    return _SD[tag]


def _inputs(gold, tag, n):
    gi, seeds = list(gold["configs"]).index(tag), gold["seeds"]
    B, T = (int(v) for v in gold["cases"][n])
    h = _setup(gold, tag)[0]
    mel = R.make_mel(B, T, seeds["mel"] + 10 * gi + n)
    return mel, GR.upstream(B, T * int(np.prod(h["upsample_rates"])), seeds["upstream"] + 10 * gi + n)


def _generator(h, sd, folded=False):
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import Generator
    gen = Generator(h)
    gen.load_state_dict(sd)
    if folded:
        gen.remove_weight_norm()
    return gen.cuda().trainable()


def _step(gen, mel, gy):
    """One forward + backward of sum(audio * gy): ({name: grad on the CPU, 'mel': the mel's}, the audio)."""
    gen.zero_grad(set_to_none=True)
    m = mel.cuda().requires_grad_(True)
    audio = gen(m)
    assert audio.grad_fn is not None and audio.shape == gy.shape
    (audio * gy.cuda()).sum().backward()
    grads = {k: p.grad.detach().cpu() for k, p in gen.named_parameters()}
    grads["mel"] = m.grad.detach().cpu()
    return grads, audio.detach()


def _ref(sd, h, mel, gy, dtype=torch.float64):
    g, m, _ = GR.grads(sd, h, mel, gy, dtype)
    return dict(g, mel=m)


def _cpu_dev(sd, h, mel, gy, g64):
    g32 = _ref(sd, h, mel, gy, torch.float32)
    return {k: float((g32[k].double() - g64[k]).abs().max()) for k in g64}


def _compare(tag, grads, g64, dev):
    """Every tensor against fp64 within 25 * max(dev[key], 2^-23 * max |g64|); returns the worst err / bound."""
    assert sorted(grads) == sorted(g64)
    worst = 0.0
    for k, ref in g64.items():
        mag = float(ref.abs().max())
        assert mag > 0, k                                     # nothing passes by being zero
        assert grads[k].shape == ref.shape and torch.isfinite(grads[k]).all(), k
        bound = 25 * max(dev[k], ULP * mag)
        ratio = float((grads[k].double() - ref).abs().max()) / bound
        worst = max(worst, ratio)
        assert ratio <= 1.0, (tag, k, ratio)
    print(tag, len(g64), "tensors, worst err/bound", worst)
    return worst


@pytest.mark.parametrize("tag", ["rb1", "rb2"])
def test_gradients_vs_reference_recording_and_fp64(gold, tag):
    """Both generators on both cases: every parameter's and the mel's gradient against the reference's recorded gradients and
    against fp64, within the recorded fp32 deviation of the reference's own gradients on that run; and folded, after
    remove_weight_norm(), against fp64."""
    h, sd = _setup(gold, tag)
    keys = json.loads(str(gold[f"{tag}_keys"]))
    assert keys == list(sd) + ["mel"]
    normed, folded_gen = _generator(h, sd), _generator(h, sd, folded=True)
    folded = R.fold(sd)
    for n in range(len(gold["cases"])):
        mel, gy = _inputs(gold, tag, n)
        g64 = _ref(sd, h, mel, gy)
        dev = dict(zip(keys, (float(v) for v in gold[f"{tag}_dev{n}"])))
        for k, v in zip(keys, gold[f"{tag}_mag{n}"]):          # the weights are the recording's: fp64 agrees with what it saw
            assert abs(float(g64[k].abs().max()) - float(v)) <= 1e-9 * float(v), k
        grads, audio = _step(normed, mel, gy)
        _compare(f"{tag} case {n} weight-normed vs fp64", grads, g64, dev)
        with torch.no_grad():
            assert torch.equal(audio, normed(mel.cuda()))      # the kept-activation forward has the bits of inference
        worst = 0.0                                            # the reference's own fp32 gradients
        for k in keys:
            rec = torch.from_numpy(gold[f"{tag}_g{n}/{k}"])
            ratio = float((grads[k].double() - rec.double()).abs().max()) / (25 * max(dev[k], ULP * float(g64[k].abs().max())))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (tag, n, k, ratio)
        print(tag, "case", n, "vs the recording, worst err/bound", worst)
        f64 = _ref(folded, h, mel, gy)
        grads_f, _ = _step(folded_gen, mel, gy)
        assert "conv_pre.weight" in grads_f
        _compare(f"{tag} case {n} folded vs fp64", grads_f, f64, _cpu_dev(folded, h, mel, gy, f64))


def test_general_upstream_gradient_through_the_tanh_and_zero_rows(gold):
    """An upstream gradient that is zero on one whole item and on a stretch of the other: those samples must add nothing."""
    h, sd = _setup(gold, "rb1")
    mel, gy = _inputs(gold, "rb1", 1)
    gy = gy.clone()
    gy[0] = 0.0
    gy[1, :, 100:300] = 0.0
    g64 = _ref(sd, h, mel, gy)
    grads, _ = _step(_generator(h, sd), mel, gy)
    assert float(grads["mel"][0].abs().max()) == 0.0
    _compare("rb1 sparse upstream", grads, g64, _cpu_dev(sd, h, mel, gy, g64))


def test_full_width_config_v1_vs_fp64():
    h = R.load_config(os.path.join(GOLDEN, "hifigan_config_v1.json"))
    sd = R.calibrate(R.make_state_dict(h, 411), h, R.make_mel(1, 4, 412))
    mel = R.make_mel(1, 2, 413)
    gy = GR.upstream(1, 2 * 256, 414)
    g64 = _ref(sd, h, mel, gy)
    grads, _ = _step(_generator(h, sd), mel, gy)
    _compare("config_v1 B=1 T=2", grads, g64, _cpu_dev(sd, h, mel, gy, g64))


SGD_LR = 1e-7


def test_three_sgd_steps_follow_the_fp64_run_and_repack_by_themselves(gold):
    """p -= lr * grad of 0.5 * sum((audio - target)^2), three times, on the weight-normed parameters: every training forward packs
    the parameters as they are, and the inference call at the end packs again by itself (the training path drops the cache).
    The loss before every step and after the last and every parameter at the end stay within 25 times the fp32 CPU run's
    deviation from the fp64 run of the same steps, floored at 2^-23 * the loss (a sum of squares) and 2^-23 * max |p64|."""
    h, sd = _setup(gold, "rb2")
    mel = R.make_mel(2, 5, 77)
    target = torch.tanh(torch.randn(2, 1, 5 * 32, generator=torch.Generator().manual_seed(5))) * 0.5
    l64, p64 = GR.sgd_steps(sd, h, mel, target, torch.float64, SGD_LR, 3)
    l32, p32 = GR.sgd_steps(sd, h, mel, target, torch.float32, SGD_LR, 3)
    assert l64[3] < l64[2] < l64[1] < l64[0] and l64[0] - l64[3] > 0.01 * l64[0]
    gen, got = _generator(h, sd), []
    for _ in range(3):
        gen.zero_grad(set_to_none=True)
        loss = 0.5 * ((gen(mel.cuda()) - target.cuda()) ** 2).sum()
        loss.backward()
        got.append(float(loss.detach()))
        assert gen._packed is None                             # the inference cache is dropped, not left stale
        with torch.no_grad():
            for p in gen.parameters():
                p -= SGD_LR * p.grad
    with torch.no_grad():
        got.append(float(0.5 * ((gen(mel.cuda()) - target.cuda()) ** 2).sum()))
    assert gen._packed is not None
    print("loss fp64", l64, "fp32 CPU", l32, "GPU", got)
    assert got[3] < got[2] < got[1] < got[0]
    for a, b, c in zip(got, l64, l32):
        assert abs(a - b) <= 25 * max(abs(c - b), ULP * abs(b))
    worst = 0.0
    for k, p in gen.state_dict().items():
        bound = 25 * max(float((p32[k].double() - p64[k]).abs().max()), ULP * float(p64[k].abs().max()))
        worst = max(worst, float((p.cpu().double() - p64[k]).abs().max()) / bound)
    print("parameters after three steps, worst err/bound", worst)
    assert worst <= 1.0


ADAM_LR = 1e-4


def test_three_fused_adam_steps_follow_the_fp64_adam_loop(gold):
    """optim.FusedAdam writes the parameters through raw pointers and bumps no version, so nothing but packing on every training
    forward makes the next forward see the step.  Three steps on the weight-normed parameters: the audio and the loss before every
    step and after the last (the last through the inference path, which must pack again too) stay within 25 times the fp32 CPU
    loop's deviation from the fp64 loop, floored at 2^-23 (the audio is of order 1) and 2^-23 * the loss; the audio moves by
    thousands of times that bound from step to step, so stale packed weights cannot pass."""
    from tacotron2_subword_amd.optim import FusedAdam
    h, sd = _setup(gold, "rb2")
    mel = R.make_mel(2, 5, 77)
    target = torch.tanh(torch.randn(2, 1, 5 * 32, generator=torch.Generator().manual_seed(5))) * 0.5
    l64, a64, _ = GR.adam_steps(sd, h, mel, target, torch.float64, ADAM_LR, 3)
    l32, a32, _ = GR.adam_steps(sd, h, mel, target, torch.float32, ADAM_LR, 3)
    assert l64[3] < l64[2] < l64[1] < l64[0]
    gen = _generator(h, sd)
    versions = [p._version for p in gen.parameters()]
    opt = FusedAdam(gen.parameters(), lr=ADAM_LR)
    losses, audios = [], []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        audio = gen(mel.cuda())
        loss = 0.5 * ((audio - target.cuda()) ** 2).sum()
        loss.backward()
        losses.append(float(loss.detach()))
        audios.append(audio.detach().cpu())
        opt.step()
    with torch.no_grad():
        audio = gen(mel.cuda())
        audios.append(audio.cpu())
        losses.append(float(0.5 * ((audio - target.cuda()) ** 2).sum()))
    print("loss fp64", l64, "fp32 CPU", l32, "GPU", losses, "versions bumped:", versions != [p._version for p in gen.parameters()])
    for n in range(4):
        bound = 25 * max(float((a32[n].double() - a64[n]).abs().max()), ULP)
        err = float((audios[n].double() - a64[n]).abs().max())
        print("step", n, "audio err", err, "bound", bound, "moved since the step before", float((a64[n] - a64[max(n - 1, 0)]).abs().max()))
        assert err <= bound, n
        assert n == 0 or float((a64[n] - a64[n - 1]).abs().max()) > 1000 * bound
        assert abs(losses[n] - l64[n]) <= 25 * max(abs(l32[n] - l64[n]), ULP * l64[n]), n


def test_only_the_mel_asks_for_a_gradient(gold):
    """No parameter requires grad: the weight gradients are not launched and the mel's gradient is the one of the full backward."""
    h, sd = _setup(gold, "rb1")
    mel, gy = _inputs(gold, "rb1", 0)
    gen = _generator(h, sd)
    full, _ = _step(gen, mel, gy)
    gen.zero_grad(set_to_none=True)
    for p in gen.parameters():
        p.requires_grad_(False)
    m = mel.cuda().requires_grad_(True)
    (gen(m) * gy.cuda()).sum().backward()
    assert torch.equal(m.grad.cpu(), full["mel"]) and all(p.grad is None for p in gen.parameters())


def test_mel_l1_recipe_has_the_bits_of_feeding_backward_the_log_mel_gradient(gold):
    """Plumbing only: 45 * L1(mel(y_hat), mel_target) through one graph gives the parameter gradients of two graphs cut at y_hat."""
    from tacotron2_subword_amd.utils import mel_spectrogram_from_audio
    h, sd = _setup(gold, "rb2")
    mel = R.make_mel(2, 33, 91).cuda()
    gen = _generator(h, sd)
    with torch.no_grad():
        y = torch.tanh(torch.randn(2, 33 * 32, generator=torch.Generator().manual_seed(92))).cuda() * 0.5
        target = mel_spectrogram_from_audio(y)
    gen.zero_grad(set_to_none=True)
    y_hat = gen(mel)
    (F.l1_loss(mel_spectrogram_from_audio(y_hat.squeeze(1), differentiable=True), target) * 45).backward()
    one = {k: p.grad.clone() for k, p in gen.named_parameters()}
    gen.zero_grad(set_to_none=True)
    y_hat = gen(mel)
    cut = y_hat.detach().squeeze(1).requires_grad_(True)
    (F.l1_loss(mel_spectrogram_from_audio(cut, differentiable=True), target) * 45).backward()
    y_hat.backward(cut.grad.unsqueeze(1))
    assert float(cut.grad.abs().max()) > 0
    for k, p in gen.named_parameters():
        assert float(p.grad.abs().max()) > 0 and torch.equal(p.grad, one[k]), k


def test_two_runs_give_the_same_bits(gold):
    h, sd = _setup(gold, "rb1")
    mel, gy = _inputs(gold, "rb1", 1)
    gen = _generator(h, sd)
    a, _ = _step(gen, mel, gy)
    b, _ = _step(gen, mel, gy)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_surface_with_and_without_the_opt_in(gold):
    from tacotron2_subword_amd.hifigan_infer.hifigan_model import Generator
    h, sd = _setup(gold, "rb2")
    mel = R.make_mel(2, 9, 95).cuda()
    never = Generator(h)
    never.load_state_dict(sd)
    never = never.cuda()
    gen = _generator(h, sd)
    with torch.no_grad():
        want = never(mel)
    # never opted in, or opted out again: the refusal by name, the silent no-grad result, the bits
    for g in (never, gen.trainable(False)):
        with pytest.raises(RuntimeError, match="inference only"):
            g(mel.clone().requires_grad_(True))
        out = g(mel)
        assert not out.requires_grad and out.grad_fn is None and torch.equal(out, want)
        a, lens = g(mel, lengths=[9, 4])
        assert not a.requires_grad and lens.tolist() == [9 * 32, 4 * 32]
    gen.trainable()
    # opted in: grad mode off or nothing requiring grad runs the inference path; otherwise one node, the same bits
    with torch.no_grad():
        assert torch.equal(gen(mel), want) and gen(mel).grad_fn is None
        a, _ = gen(mel, lengths=[9, 4])
    out = gen(mel)
    assert out.grad_fn is not None and torch.equal(out.detach(), want)
    with pytest.raises(RuntimeError, match="lengths= together with a gradient"):
        gen(mel, lengths=[9, 4])
    with pytest.raises(RuntimeError, match="return_pre_tanh"):
        gen(mel, return_pre_tanh=True)
    for p in gen.parameters():
        p.requires_grad_(False)
    assert gen(mel).grad_fn is None                            # nothing asks for a gradient
    m = mel.clone().requires_grad_(True)
    gen(m).sum().backward()                                    # the mel alone does: conv_pre's data gradient
    assert m.grad is not None and float(m.grad.abs().max()) > 0 and all(p.grad is None for p in gen.parameters())
