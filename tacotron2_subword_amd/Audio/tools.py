"""Audio/tools.py of the reference: get_mel (:30-42), inv_mel_spec (:45-61) and load_wav_to_torch (:25-27), plus
get_mel_batch, an addition: the mels of many files from one ragged launch, on the device, ready for SoftDTW.

The front end module (the reference's module-level `_stft`) is built on first use and lives on the GPU when there is one:
get_mel then computes on the GPU and returns a CPU tensor, as the reference does (Audio/stft.py:66-70)."""
import numpy as np
import torch

from . import hparams
from . import stft
from .audio_processing import griffin_lim
from ..utils import load_wav_to_torch  # noqa: F401  (Audio.tools.load_wav_to_torch)

_front = None


def _get_stft():
    global _front
    if _front is None:
        _front = stft.TacotronSTFT(hparams.filter_length, hparams.hop_length, hparams.win_length, hparams.n_mel_channels,
                                   hparams.sampling_rate, hparams.mel_fmin, hparams.mel_fmax)
        if torch.cuda.is_available():
            _front = _front.cuda()
    return _front


def __getattr__(name):
    if name == "_stft":                                  # the reference's module attribute
        return _get_stft()
    raise AttributeError(name)


def _load_norm(filename, front):
    audio, sampling_rate = load_wav_to_torch(filename)
    if sampling_rate != front.sampling_rate:
        raise ValueError("{}: {} SR doesn't match target {} SR".format(filename, sampling_rate, front.sampling_rate))
    return audio / hparams.max_wav_value


def get_mel(filename):
    """wav file -> log-mel [n_mel_channels, frames] on the CPU."""
    front = _get_stft()
    audio_norm = _load_norm(filename, front).unsqueeze(0)
    with torch.no_grad():
        melspec = front.mel_spectrogram(audio_norm.to(front.mel_basis.device))
    return torch.squeeze(melspec, 0).cpu()


def get_mel_batch(filenames, time_major=True):
    """wav files -> (mel, frame_lengths) on the GPU from one launch: mel [B, frames_max, n_mel_channels] (or
    [B, n_mel_channels, frames_max] with time_major=False), zero past each item's own frames; frame_lengths int32 [B].
    Every item has the bits get_mel gives for it alone.  SoftDTW(...)(X, Y, x_lengths, y_lengths) takes both as they are."""
    front = _get_stft()
    if not front.mel_basis.is_cuda:
        raise RuntimeError("Audio.tools.get_mel_batch: the ragged launch is a HIP kernel and needs a GPU (get_mel works file by file on the CPU)")
    audios = [_load_norm(f, front) for f in filenames]
    if not audios:
        raise ValueError("Audio.tools.get_mel_batch: no files")
    lengths = [int(a.numel()) for a in audios]
    x = torch.zeros(len(audios), max(lengths))
    for i, a in enumerate(audios):
        x[i, :lengths[i]] = a
    with torch.no_grad():
        return front.mel_spectrogram(x.to(front.mel_basis.device), lengths=lengths, time_major=time_major)


def inv_mel_spec(mel, out_filename, griffin_iters=60):
    """log-mel [n_mel_channels, frames] -> a wav file through the mel basis (transposed, not inverted, and scaled by 1000, as
    the reference does) and Griffin-Lim."""
    from scipy.io.wavfile import write
    front = _get_stft()
    dev = front.mel_basis.device
    with torch.no_grad():
        mel_decompress = front.spectral_de_normalize(torch.stack([mel]).to(dev)).transpose(1, 2)
        spec_from_mel = torch.mm(mel_decompress[0], front.mel_basis).transpose(0, 1).unsqueeze(0) * 1000
        audio = griffin_lim(spec_from_mel[:, :, :-1].contiguous(), front.stft_fn, griffin_iters)
    write(out_filename, hparams.sampling_rate, audio.squeeze().cpu().numpy())
