"""CPU-only: the synthesis side of stft.py, window_sumsquare, griffin_lim and the bias remover against the vectors recorded
from the reference (tests/golden/make_golden_stft_inverse.py), and t2_stft_plan's sizes and refusals (a pure host call).

The torch formulas of the CPU path are held to 20 x the reference's own fp32-versus-fp64 error, which the recording stores
per quantity (err_*): the bound the GPU tests use for the kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

import stft_ref as R

NAMES = list(R.CONFIGS)


@pytest.fixture(scope="module")
def G():
    return R.golden()


def _stft(name):
    from tacotron2_subword_amd.stft import STFT
    return STFT(*R.CONFIGS[name])


def _close(got, G, key, name):
    err = float(np.abs(np.asarray(got) - G[f"{key}_{name}"]).max())
    bound = 20 * float(G[f"err_{key}_{name}"])
    print(key, name, "max err", err, "bound", bound)
    assert got.shape == G[f"{key}_{name}"].shape
    assert np.abs(G[f"{key}_{name}"]).max() > 0.1
    assert err <= bound


@pytest.mark.parametrize("name", NAMES)
def test_inverse_basis_and_state_dict(G, name):
    s = _stft(name)
    assert list(s.state_dict().keys()) == ["forward_basis", "inverse_basis"]
    fl = R.CONFIGS[name][0]
    assert tuple(s.inverse_basis.shape) == (fl + 2, 1, fl) and s.inverse_basis.dtype == torch.float32
    rows = G[f"basis_rows_{name}"]
    got = s.inverse_basis[rows, 0, :].numpy()
    assert np.abs(got - G[f"basis_{name}"]).max() <= 1e-6 * float(G[f"basis_max_{name}"])     # pinv goes through LAPACK
    assert abs(float(s.inverse_basis.abs().max()) - float(G[f"basis_max_{name}"])) <= 1e-6 * float(G[f"basis_max_{name}"])


@pytest.mark.parametrize("name", NAMES)
def test_window_sumsquare_bit_for_bit(G, name):
    from tacotron2_subword_amd.audio_processing import window_sumsquare
    fl, hop, win = R.CONFIGS[name]
    nf = 1 + 4000 // hop
    env = window_sumsquare("hann", nf, hop_length=hop, win_length=win, n_fft=fl, dtype=np.float32)
    assert env.dtype == np.float32 and np.array_equal(env, G[f"env_{name}"])
    if name == "short_window":
        assert int((env == 0).sum()) == 113
    with pytest.raises(ValueError):
        window_sumsquare("hann", nf, hop_length=hop, win_length=win, n_fft=fl, norm=2)


@pytest.mark.parametrize("name", NAMES)
def test_inverse_and_forward_cpu(G, name):
    s, x = _stft(name), R.wave()
    _close(s.inverse(*s.transform(x)).numpy(), G, "inverse", name)
    _close(s.forward(x).numpy(), G, "forward", name)
    with pytest.raises(RuntimeError):
        s.inverse(torch.zeros(1, R.CONFIGS[name][0] // 2 + 1, 4), torch.zeros(1, R.CONFIGS[name][0] // 2 + 1, 5))


@pytest.mark.parametrize("name", NAMES)
def test_bias_remover_cpu(G, name):
    from tacotron2_subword_amd.bias_remover import hifiganBiasRemover
    fl, hop, win = R.CONFIGS[name]
    br = hifiganBiasRemover(R.stub_model, filter_length=fl, n_overlap=fl // hop, win_length=win, device="cpu")
    assert tuple(br.bias_spec.shape) == (1, fl // 2 + 1, 1) and "bias_spec" in br.state_dict()
    rec = G[f"bias_{name}"]
    assert np.abs(br.bias_spec.numpy() - rec).max() <= 1e-5 * np.abs(rec).max()
    x = R.wave()
    _close(br(x, 0.9).numpy(), G, "br09", name)
    _close(br(x, 0.1).numpy(), G, "br01", name)
    assert np.abs(G[f"br09_{name}"] - G[f"forward_{name}"]).max() > 0.1          # the bias matters on these inputs
    with pytest.raises(Exception):
        hifiganBiasRemover(R.stub_model, mode="ones", device="cpu")


def test_griffin_lim_cpu(G):
    from tacotron2_subword_amd.audio_processing import griffin_lim
    s = _stft("default")
    mag, _ = s.transform(R.wave())
    _close(griffin_lim(mag, s, n_iters=2, angles=G["gl_angles"]).numpy(), G, "gl", "default")
    torch.manual_seed(0)
    assert tuple(griffin_lim(mag, s, n_iters=0).shape) == (2, 3840)                # draws its own start phases


def test_plan_sizes_without_device():
    from tacotron2_subword_amd import _lib as L
    p = L.stft_plan(1024, 256, 16)
    assert (p.bins, p.overlap, p.frame_tile, p.bin_tile, p.out_len) == (513, 4, L.STFT_FRAME_TILE, 16, 256 * 15)
    assert p.fwd_floats == 33 * 32 * 1024                  # 33 tiles of 16 bins (the last holds one), 32 chunks of 32 k
    assert p.inv_floats == 8 * 33 * 4 * 1024               # 8 column tiles of 32 samples, 33 bin chunks, 4 overlaps
    assert p.wsq_floats == 2048 and p.packed_bytes == 4 * (p.fwd_floats + p.inv_floats + p.wsq_floats)
    p = L.stft_plan(800, 200, 1)
    assert (p.bins, p.overlap, p.out_len) == (401, 4, 0) and p.fwd_floats == 26 * 25 * 1024 and p.inv_floats == 7 * 26 * 4 * 1024
    for n in (64, 128, 256, 512, 2048):
        assert L.stft_plan(n, n // 4).bins == n // 2 + 1


@pytest.mark.parametrize("args,words", [((1023, 341, 4), ("1023", "odd")), ((1024, 300, 4), ("1024", "300")), ((8192, 2048, 4), ("8192",)),
                                        ((1024, 8, 4), ("128",)), ((1024, 256, 0), ("0 frames",))])
def test_plan_refusals_without_device(args, words):
    from tacotron2_subword_amd import _lib as L
    info = L.StftPlanInfo()
    assert L.lib().t2_stft_plan(*args, C.byref(info)) != 0
    msg = L.lib().t2_last_error().decode()
    assert all(w in msg for w in words), msg
    with pytest.raises(RuntimeError):
        L.stft_plan(*args)
