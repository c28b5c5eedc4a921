"""utils.py of the reference: the mask and device helpers (:10-14, :28-33), device-agnostic; the wav, filelist and
range-compression helpers (:17-25, :38-54); mel_spectrogram(filename, ...) (:55-80) on the log-mel kernel; the alignment
generator (:92-117).  scipy is imported inside the functions that read wav files, so importing the model stays light."""
import os

import torch


def cpu_quota():
    """CPUs this process may actually use: the smaller of its affinity mask and its cgroup CPU quota (cpu.max of cgroup v2,
    cpu.cfs_quota_us / cpu.cfs_period_us of v1).  A container often SEES every core of the host (os.cpu_count() = 256 on the
    MI355X boxes) while its quota is 16."""
    n = float(len(os.sched_getaffinity(0))) if hasattr(os, "sched_getaffinity") else float(os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, float(q) / float(p))
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, q / p)
        except (OSError, ValueError):
            pass
    return max(1.0, n)


def fit_cpu_threads(reserve=2):
    """Size torch's intra-op thread pool to the CPU quota (never raises it).  Why it matters for the GPU loop: with the default
    pool (one thread per VISIBLE core) every parallel CPU tensor op wakes hundreds of OpenMP workers that spin for a while
    afterwards; under a CFS quota they burn the whole period's budget in a few milliseconds and the kernel then freezes the
    process — the thread that enqueues GPU work included — until the next 100 ms period.  Measured (round 3, scripts/fed_loop.py):
    a training loop that collates on the host stalled 65-85 ms every third step that way; with the pool sized to the quota
    it runs at the resident-batch speed.  Returns the thread count in effect."""
    # several ranks of one job share the container's quota (torchrun exports LOCAL_WORLD_SIZE; bench.py's own launcher WORLD_SIZE)
    ranks = max(1, int(os.environ.get("LOCAL_WORLD_SIZE") or os.environ.get("WORLD_SIZE") or 1))
    want = max(1, int(cpu_quota() / ranks) - reserve)
    if torch.get_num_threads() > want:
        torch.set_num_threads(want)
    return torch.get_num_threads()


def get_mask_from_lengths(lengths, max_len=None):
    """True where index < length.  (The reference allocates a torch.cuda.LongTensor and syncs
    on .item(); max_len can be passed to avoid the sync.)"""
    if max_len is None:
        max_len = int(torch.max(lengths).item())
    ids = torch.arange(0, max_len, device=lengths.device, dtype=lengths.dtype)
    return ids < lengths.unsqueeze(1)


def to_gpu(x):
    x = x.contiguous()
    if torch.cuda.is_available():
        x = x.cuda(non_blocking=True)
    return x


def load_wav_to_torch(full_path):
    """utils.py:17-19: (samples as a float32 tensor, in the file's own scale; sampling rate)."""
    import numpy as np
    from scipy.io.wavfile import read                    # lazy: importing the model does not pull in scipy
    sampling_rate, data = read(full_path)
    return torch.FloatTensor(data.astype(np.float32)), sampling_rate


def load_wav(full_path):
    """utils.py:38-40: (samples as the numpy array the file holds, sampling rate)."""
    from scipy.io.wavfile import read
    sampling_rate, data = read(full_path)
    return data, sampling_rate


def load_filepaths_and_text(filename, split="|"):
    """utils.py:22-25: one list of fields per line of a filelist."""
    with open(filename, encoding="utf-8") as f:
        return [line.strip().split(split) for line in f]


def dynamic_range_compression_torch(x, C=1, clip_val=1e-5):
    return torch.log(torch.clamp(x, min=clip_val) * C)


def dynamic_range_decompression_torch(x, C=1):
    return torch.exp(x) / C


def spectral_normalize_torch(magnitudes):
    return dynamic_range_compression_torch(magnitudes)


def spectral_de_normalize_torch(magnitudes):
    return dynamic_range_decompression_torch(magnitudes)


_mel_front = {}     # (n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, device) -> (STFT module, mel basis)


def _front(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, device):
    key = (n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, str(device))
    if key not in _mel_front:
        from .stft import STFT, mel_filterbank             # lazy: scipy.signal
        basis = torch.from_numpy(mel_filterbank(sampling_rate, n_fft, num_mels, fmin, fmax)).float().to(device)
        _mel_front[key] = ((STFT(n_fft, hop_size, win_size).to(device) if device.type == "cuda" else None), basis)
    return _mel_front[key]


def mel_spectrogram_from_audio(y, n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0.0, fmax=8000.0,
                               lengths=None, differentiable=False):
    """The tensor-in form of `mel_spectrogram` (utils.py:73-79, HiFi-GAN's meldataset convention): y [B, T] float32 in
    [-1, 1] -> log-mel [B, num_mels, frames], or (mel, frame_lengths) with per-item `lengths` (see stft.log_mel).  No file, no
    normalisation.  On the GPU it is one launch of the log-mel kernel, and with differentiable=True a y that requires grad gets
    its gradient from the HIP backward: the spectral term 45 * L1(mel(y), mel(y_hat)) of a vocoder recipe is
        F.l1_loss(mel_spectrogram_from_audio(y_hat, differentiable=True), mel_spectrogram_from_audio(y)) * 45
    On the CPU it is the torch.stft formula (lengths are then refused)."""
    if y.dim() != 2:
        raise RuntimeError(f"mel_spectrogram_from_audio: expected audio [B, T], got {tuple(y.shape)}")
    device = y.device
    pad = int((n_fft - hop_size) / 2)
    front, basis = _front(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, device)
    if device.type == "cuda":
        from .stft import log_mel
        mel, frame_lengths = log_mel(y, front, basis, lengths=lengths, pad=pad, mag_eps=1e-9, differentiable=differentiable)
        return mel if lengths is None else (mel, frame_lengths)
    if lengths is not None:
        raise RuntimeError("mel_spectrogram_from_audio: per-item lengths need the HIP kernel (CUDA tensors)")
    y = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(y, n_fft, hop_length=hop_size, win_length=win_size, window=torch.hann_window(win_size), center=False,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    spec = torch.sqrt(spec.real.pow(2) + spec.imag.pow(2) + 1e-9)
    return spectral_normalize_torch(torch.matmul(basis, spec))


def mel_spectrogram(filename, n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0.0, fmax=8000.0,
                    center=False, stftTaco=False, stftCUDA=False, device=None):
    """utils.py:55-80, the HiFi-GAN convention: wav / 32768, peak-normalised to 0.95 (librosa.util.normalize restated as
    x / max|x|), reflect-padded by (n_fft - hop_size)/2 per side, torch.stft(center=False) with a periodic Hann window,
    sqrt(re^2 + im^2 + 1e-9), mel filterbank, log(clamp(., 1e-5)) -> [1, num_mels, frames] on `device`.
    device=None (an addition) is the GPU when there is one: the whole formula is then one launch of the log-mel kernel
    (stft.log_mel with pad=(n_fft - hop_size)/2, mag_eps=1e-9); on the CPU it is torch.stft.  As in the reference the file's
    own sampling rate replaces `sampling_rate`, and stftTaco / stftCUDA are accepted and ignored."""
    import numpy as np
    audio, sampling_rate = load_wav(filename)
    audio = audio / 32768.0
    peak = np.max(np.abs(audio)) if audio.size else 0.0
    audio = audio / (peak if peak >= np.finfo(audio.dtype).tiny else 1.0) * 0.95
    y = torch.FloatTensor(audio).unsqueeze(0)
    if torch.min(y) < -1.:
        print('min value is ', torch.min(y))
    if torch.max(y) > 1.:
        print('max value is ', torch.max(y))
    device = torch.device(("cuda" if torch.cuda.is_available() else "cpu") if device is None else device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    pad = int((n_fft - hop_size) / 2)
    front, basis = _front(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, device)
    if device.type == "cuda":
        if center:
            raise NotImplementedError("mel_spectrogram: center=True pads twice (the reference never passes it); the log-mel kernel takes one reflect "
                                      "padding of at most n_fft/2: use device='cpu'")
        from .stft import log_mel
        return log_mel(y.to(device), front, basis, pad=pad, mag_eps=1e-9)[0]
    y = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(y, n_fft, hop_length=hop_size, win_length=win_size, window=torch.hann_window(win_size), center=center,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    spec = torch.sqrt(spec.real.pow(2) + spec.imag.pow(2) + 1e-9)
    return spectral_normalize_torch(torch.matmul(basis, spec))


def create_alignment(base_mat, duration_predictor_output):
    """utils.py:108-117: base_mat[i, frames of phone j, j] = 1 where phone j of item i lasts duration[i, j] frames
    (frames laid end to end).  Same result as the reference's triple Python loop, built from a cumulative sum."""
    dur = duration_predictor_output.long()
    end = torch.cumsum(dur, dim=1)                       # [B, n_phones]
    start = end - dur
    t = torch.arange(base_mat.size(1), device=dur.device)[None, :, None]
    hit = (t >= start[:, None, :]) & (t < end[:, None, :])
    base_mat[hit.to(base_mat.device)] = 1
    return base_mat


class Alignment_Generator(torch.nn.Module):
    """utils.py:92-106: durations [B, n_phones] -> hard alignment [B, max total frames, n_phones] (on the CPU, like
    the reference's torch.zeros)."""

    def LR(self, duration_predictor_output):
        frame_lens = torch.sum(duration_predictor_output, -1)
        expand_max_frame_len = int(torch.max(frame_lens, -1)[0])
        alignment = torch.zeros(duration_predictor_output.size(0), expand_max_frame_len, duration_predictor_output.size(1))
        return create_alignment(alignment, duration_predictor_output)

    def forward(self, duration_predictor_output):
        return self.LR(duration_predictor_output)
