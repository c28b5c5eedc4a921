"""CPU-only checks of the log-mel front end: the pure host plan of csrc/melspec.hip, the derived bound of melspec_ref.py
against an fp32 evaluation, and the Python surface that needs no GPU (utils.mel_spectrogram's CPU path, the Audio package)."""
import math
import sys

import numpy as np
import pytest
import torch

import melspec_ref as M


@pytest.fixture(scope="module")
def L():
    from tacotron2_subword_amd import build
    from tacotron2_subword_amd import _lib
    build.build()
    return _lib


def _wav(path, n, sr=22050, seed=0):
    from scipy.io.wavfile import write
    x = M.signal(1, n, seed)[0]
    write(str(path), sr, (x * 20000).round().to(torch.int16).numpy())
    return path


@pytest.mark.parametrize("n_mels", [8, 33, 80, 128])
@pytest.mark.parametrize("conv", ["taco", "hifigan"])
@pytest.mark.parametrize("N,hop", [(64, 16), (512, 128), (800, 200), (1024, 256)])
def test_plan_values(L, N, hop, conv, n_mels):
    pad = N // 2 if conv == "taco" else (N - hop) // 2
    n, B = 40 * hop + 7, 3
    p = L.melspec_plan(N, hop, pad, n_mels, n, B)
    bins = N // 2 + 1
    assert p.bins == bins and p.frame_tile == 32 == L.STFT_FRAME_TILE
    assert p.passes == -(-bins // 64) and p.row_tiles == -(-n_mels // 32)
    assert p.nf_max == (n + 2 * pad - N) // hop + 1 == M.frames(n, N, hop, pad)
    assert p.nf_max == (1 + n // hop if conv == "taco" else n // hop)
    assert p.frame_tiles == -(-p.nf_max // 32)
    assert p.fwd_floats == -(-bins // 16) * -(-N // 32) * 1024 == L.stft_plan(N, hop).fwd_floats
    assert p.mel_floats == p.row_tiles * p.passes * 2048
    assert p.packed_bytes == 4 * (p.fwd_floats + p.mel_floats)
    assert p.split_scratch_floats == p.passes * B * p.nf_max * n_mels
    assert 1 <= p.splits <= p.passes
    assert p.scratch_floats == (p.split_scratch_floats if p.splits > 1 else 0)


@pytest.mark.parametrize("args,words", [
    ((1023, 256, 511, 80, 4000, 1), r"filter_length=1023 is odd"),
    ((4098, 256, 512, 80, 40000, 1), r"filter_length=4098 outside"),
    ((1024, 256, 512, 0, 4000, 1), r"n_mels=0 outside 1\.\.128"),
    ((1024, 256, 512, 129, 4000, 1), r"n_mels=129 outside 1\.\.128"),
    ((1024, 256, -1, 80, 4000, 1), r"pad=-1 outside 0\.\.filter_length/2=512"),
    ((1024, 256, 513, 80, 4000, 1), r"pad=513 outside 0\.\.filter_length/2=512"),
    ((1024, 256, 384, 80, 255, 1), r"n=255 samples with pad=384"),
    ((1024, 0, 512, 80, 4000, 1), r"hop_length=0 outside"),
    ((1024, 256, 512, 80, 4000, 0), r"B=0 outside"),
])
def test_plan_refusals(L, args, words):
    with pytest.raises(RuntimeError, match=words):
        L.melspec_plan(*args)


def test_plan_accepts_the_edges(L):
    assert L.melspec_plan(1024, 256, 384, 80, 256, 1).nf_max == 1       # n + 2*pad == N: one frame
    assert L.melspec_plan(4096, 1024, 2048, 128, 4096, 1).bins == 2049
    assert L.melspec_plan(2, 1, 0, 1, 2, 1).nf_max == 1


def test_plan_splits_single_utterance_not_batch(L):
    n = 9 * 22050                                                        # 9 s at 22.05 kHz: 776 frames, 25 frame tiles
    one, batch = L.melspec_plan(1024, 256, 512, 80, n, 1), L.melspec_plan(1024, 256, 512, 80, n, 64)
    assert one.frame_tiles == 25 and one.passes == 9
    assert 1 < one.splits <= one.passes and one.scratch_floats == one.split_scratch_floats == 9 * one.nf_max * 80
    assert batch.splits == 1 and batch.scratch_floats == 0


@pytest.mark.parametrize("conv", ["taco", "hifigan"])
@pytest.mark.parametrize("name", list(M.CONFIGS))
def test_bound_holds_for_fp32_and_rejects_a_shifted_frame(name, conv):
    from tacotron2_subword_amd.stft import STFT, mel_filterbank
    N, hop, win, n_mels = M.CONFIGS[name]
    pad, eps = (N // 2, 0.0) if conv == "taco" else ((N - hop) // 2, 1e-9)
    fwd = STFT(N, hop, win).forward_basis[:, 0, :]
    melb = torch.from_numpy(mel_filterbank(22050, N, n_mels, 0.0, 8000.0))
    x = M.signal(3, 33 * hop + hop // 3)
    ref = M.logmel64(x, fwd, melb, N, hop, pad, eps)
    got = M.logmel32(x, fwd, melb, N, hop, pad, eps).double()
    assert got.shape == ref["logmel"].shape and got.shape[-1] == M.frames(x.shape[1], N, hop, pad)
    assert int(ref["clipped"].sum()) == 0                               # every element is pinned
    worst = float(((got - ref["logmel"]).abs() / ref["log_bound"]).max())
    shifted = float(((got[:, :, 1:] - ref["logmel"][:, :, :-1]).abs() / ref["log_bound"][:, :, :-1]).max())
    print(f"{name} {conv}: fp32 err/bound {worst:.3f}, shifted by one frame {shifted:.1f}, min mel {float(ref['mel'].min()):.2e}, "
          f"largest log bound {float(ref['log_bound'].max()):.2e}")
    assert worst <= 1.0 and shifted > 1.0


def test_utils_mel_spectrogram_cpu_vs_torch_stft_fp64(tmp_path):
    from tacotron2_subword_amd import utils
    from tacotron2_subword_amd.stft import mel_filterbank
    n = 20 * 256 + 77
    path = _wav(tmp_path / "a.wav", n)
    got = utils.mel_spectrogram(str(path), device="cpu")
    assert got.shape == (1, 80, n // 256) and got.dtype == torch.float32
    from scipy.io.wavfile import read
    _, data = read(str(path))
    a = data / 32768.0
    y = torch.from_numpy(a / np.abs(a).max() * 0.95).float()[None]      # the fp32 signal the function forms
    assert float(y.abs().max()) == pytest.approx(0.95, rel=1e-6)
    yp = torch.nn.functional.pad(y.double()[:, None], (384, 384), mode="reflect")[:, 0]
    spec = torch.stft(yp, 1024, hop_length=256, win_length=1024, window=torch.hann_window(1024, dtype=torch.float64), center=False, return_complex=True)
    melb = torch.from_numpy(mel_filterbank(22050, 1024, 80, 0.0, 8000.0))
    ref = torch.log(torch.clamp(torch.matmul(melb.double(), torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)), min=1e-5))
    # the fp64 formulas of melspec_ref are torch.stft's
    mine = M.logmel64(y, M.stft_basis64(1024, 1024), melb, 1024, 256, 384, 1e-9, basis_rounding=2.0 ** -24)
    assert float((mine["logmel"] - ref).abs().max()) < 1e-9
    worst = float(((got.double() - ref).abs() / mine["log_bound"]).max())
    print(f"utils.mel_spectrogram cpu: err/bound {worst:.3f}")
    assert worst <= 1.0
    # flags the reference ignores are accepted
    assert torch.equal(utils.mel_spectrogram(str(path), stftTaco=True, stftCUDA=True, device="cpu"), got)


def test_utils_helpers(tmp_path):
    from tacotron2_subword_amd import utils
    path = _wav(tmp_path / "a.wav", 3000)
    t, sr = utils.load_wav_to_torch(str(path))
    d, sr2 = utils.load_wav(str(path))
    assert sr == sr2 == 22050 and t.dtype == torch.float32 and d.dtype == np.int16 and torch.equal(t, torch.from_numpy(d.astype(np.float32)))
    (tmp_path / "list.txt").write_text("a.wav|xin chào\nb.wav|hai\n", encoding="utf-8")
    assert utils.load_filepaths_and_text(str(tmp_path / "list.txt")) == [["a.wav", "xin chào"], ["b.wav", "hai"]]
    x = torch.tensor([1e-7, 0.5, 2.0])
    c = utils.spectral_normalize_torch(x)
    assert torch.equal(c, torch.log(torch.clamp(x, min=1e-5))) and torch.equal(utils.dynamic_range_compression_torch(x, C=2), torch.log(torch.clamp(x, min=1e-5) * 2))
    assert torch.allclose(utils.spectral_de_normalize_torch(c)[1:], x[1:]) and torch.equal(utils.dynamic_range_decompression_torch(c, C=2), torch.exp(c) / 2)


def test_import_model_stays_light():
    import subprocess
    code = "import sys; import tacotron2_subword_amd.model, tacotron2_subword_amd.utils; assert 'scipy' not in sys.modules and 'matplotlib' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(__import__("pathlib").Path(__file__).resolve().parents[1]))


def test_audio_tools_get_mel_and_inv_mel_spec(tmp_path):
    from tacotron2_subword_amd.Audio import tools, hparams
    n = 12 * 256 + 100
    path = _wav(tmp_path / "a.wav", n)
    audio, sr = tools.load_wav_to_torch(str(path))
    assert sr == hparams.sampling_rate and audio.shape == (n,)
    mel = tools.get_mel(str(path))
    assert mel.shape == (hparams.n_mel_channels, 1 + n // hparams.hop_length) and mel.dtype == torch.float32 and not mel.is_cuda
    assert torch.isfinite(mel).all() and float(mel.min()) >= math.log(1e-5) - 1e-6
    assert tools._stft.sampling_rate == 22050 and tools._stft.stft_fn.filter_length == 1024
    with pytest.raises(ValueError, match="16000 SR doesn't match target 22050 SR"):
        tools.get_mel(str(_wav(tmp_path / "b.wav", n, sr=16000)))
    out = tmp_path / "inv.wav"
    tools.inv_mel_spec(mel, str(out), griffin_iters=1)
    y, sr = tools.load_wav_to_torch(str(out))
    assert sr == 22050 and y.shape == (256 * (mel.shape[1] - 2),) and torch.isfinite(y).all() and float(y.abs().max()) > 0


def test_audio_alias_resolves_what_the_scoring_scripts_use(monkeypatch):
    import tacotron2_subword_amd.Audio as A
    monkeypatch.setitem(sys.modules, "Audio", A)
    for k in ("hparams", "tools", "stft", "audio_processing"):
        monkeypatch.setitem(sys.modules, "Audio." + k, getattr(A, k))
    import Audio                                                        # softdtw.py:19, best_checkpoint.py:39
    import Audio.stft as stft                                           # Audio/tools.py:6-8
    import Audio.hparams as hparams
    from Audio.audio_processing import griffin_lim
    assert callable(Audio.tools.get_mel) and callable(Audio.tools.inv_mel_spec) and callable(Audio.tools.load_wav_to_torch) and callable(griffin_lim)
    assert callable(Audio.tools.get_mel_batch)
    assert hparams.max_wav_value == 32768.0 and (hparams.filter_length, hparams.hop_length, hparams.win_length) == (1024, 256, 1024)
    assert (hparams.n_mel_channels, hparams.sampling_rate, hparams.mel_fmin, hparams.mel_fmax) == (80, 22050, 0.0, 8000.0)
    assert stft.TacotronSTFT is __import__("tacotron2_subword_amd.stft", fromlist=["x"]).TacotronSTFT and hasattr(stft, "STFT")


def test_log_mel_refuses_cpu_tensors_and_abi_version_is_unchanged(L):
    from tacotron2_subword_amd.stft import TacotronSTFT, log_mel
    t = TacotronSTFT()
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        log_mel(torch.zeros(1, 4000), t.stft_fn, t.mel_basis)
    with pytest.raises(RuntimeError, match="float32 signal"):
        log_mel(torch.zeros(1, 4000, dtype=torch.float64), t.stft_fn, t.mel_basis)
    with pytest.raises(RuntimeError, match="per-item lengths need the HIP kernel"):
        t.mel_spectrogram(torch.zeros(1, 4000), lengths=[4000])
    assert t.mel_spectrogram(torch.zeros(1, 4000), time_major=True).shape == (1, 16, 80)
    assert L.ABI_VERSION == 4 and L.lib().t2_version() == 4
    for name in ("t2_melspec_plan", "t2_melspec_pack", "t2_melspec"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
