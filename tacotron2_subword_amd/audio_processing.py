"""audio_processing.py of the reference: window_sumsquare (:7-56), griffin_lim (:59-75) and the log dynamic-range
compression of mel magnitudes (:78-93)."""
import numpy as np
import torch
from scipy.signal import get_window


def _pad_center(data, size):
    n = data.shape[-1]
    lpad = (size - n) // 2
    return np.pad(data, (lpad, size - n - lpad), mode="constant")


def window_sumsquare(window, n_frames, hop_length=200, win_length=800, n_fft=800, dtype=np.float32, norm=None):
    """Sum-square envelope of a window at a given hop, shape [n_fft + hop_length * (n_frames - 1)] (librosa 0.6's, as the
    reference restates it, without librosa: norm=None is the identity, anything else is refused).  Frames are added in
    ascending order, each as numpy's in-place add of the fp64 squared window onto the `dtype` envelope; csrc/stft.hip's
    epilogue sums in the same order and the same way."""
    if norm is not None:
        raise ValueError(f"window_sumsquare: norm={norm!r} is not supported (librosa.util.normalize is not restated here); use norm=None")
    win_length = n_fft if win_length is None else win_length
    total = n_fft + hop_length * (n_frames - 1)
    win_sq = _pad_center(get_window(window, win_length, fftbins=True) ** 2, n_fft)      # fp64
    x = np.zeros(total, dtype=dtype)
    for frame in range(n_frames):
        lo = frame * hop_length
        hi = min(total, lo + n_fft)
        x[lo:hi] += win_sq[:hi - lo]
    return x


def griffin_lim(magnitudes, stft_fn, n_iters=30, angles=None):
    """magnitudes [B, N/2+1, frames], stft_fn an STFT -> signal [B, hop*(frames-1)].  `angles` (an addition): the start
    phases, which the reference draws with np.random.rand on the host; numpy arrays and tensors are moved to the
    magnitudes' device."""
    if angles is None:
        angles = np.angle(np.exp(2j * np.pi * np.random.rand(*magnitudes.size()))).astype(np.float32)
    if isinstance(angles, np.ndarray):
        angles = torch.from_numpy(angles)
    angles = angles.to(device=magnitudes.device, dtype=torch.float32)
    signal = stft_fn.inverse(magnitudes, angles).squeeze(1)
    for _ in range(n_iters):
        _, angles = stft_fn.transform(signal)
        signal = stft_fn.inverse(magnitudes, angles).squeeze(1)
    return signal


def dynamic_range_compression(x, C=1, clip_val=1e-5):
    return torch.log(torch.clamp(x, min=clip_val) * C)


def dynamic_range_decompression(x, C=1):
    return torch.exp(x) / C
