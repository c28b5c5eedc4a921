"""Drop-in for the reference's ``bias_remover.hifiganBiasRemover`` (bias_remover.py:6-36) and ``waveglowBiasRemover``
(bias_remover.py:38-74): subtracts the spectrum of what the vocoder emits for an all-zero mel from the magnitudes of its
output, as inference.py:199-202 does before writing the wav.

``forward`` is two launches of csrc/stft.hip: the analysis kernel writes (re, im), and the synthesis kernel applies
``clamp(|z| - strength * bias, 0)`` as a gain on (re, im) in its loader, so no magnitude, phase or denoised-magnitude
tensor exists in between.  ``waveglowBiasRemover`` takes its bias spectrum from ``WaveGlow.infer(zeros, sigma=0)``
(waveglow/glow.py on csrc/waveglow.hip) and runs the same two launches."""
import torch

from . import stft as _stft
from .stft import STFT


class hifiganBiasRemover(torch.nn.Module):
    """Removes model bias from audio produced with HiFi-GAN.  `model`: any callable mel [1, 80, 88] -> audio [1, 1, T].
    `device` (an addition; the reference hard-codes .cuda()): "cpu" runs the torch formula, for comparison with the
    reference on a box without a GPU."""

    def __init__(self, model, filter_length=1024, n_overlap=4, win_length=1024, mode='zeros', device="cuda"):
        super().__init__()
        if mode not in ("zeros", "normal"):
            raise ValueError(f"hifiganBiasRemover: mode {mode!r} is neither 'zeros' nor 'normal'")
        hop = int(filter_length / n_overlap)
        self.stft = STFT(filter_length=filter_length, hop_length=hop, win_length=win_length).to(device)
        mel = (torch.zeros if mode == "zeros" else torch.randn)(1, 80, 88).to(device)
        with torch.no_grad():
            spec, _ = self.stft.transform(model(mel).float().squeeze(0))    # what the vocoder emits for that mel: [1, 1, T] -> [1, N/2+1, frames]
        self.register_buffer("bias_spec", spec[:, :, :1].clone())            # the first frame, [1, N/2+1, 1]

    def forward(self, audio, strength=0.1, lengths=None):
        """audio [B, T] -> [B, 1, hop * (T // hop)].  lengths (an addition): per-item sample counts of a padded batch, in the
        convention of stft.log_mel (Python ints or an int32 device tensor, e.g. what Generator.forward(mel, lengths=...) returns).
        Item b is then denoised as audio[b, :lengths[b]] alone would be, bit for bit, the result is zero behind its
        hop * (lengths[b] // hop) samples, and (audio, lengths) is returned with those counts as an int32 device tensor."""
        audio = audio.to(self.bias_spec.device).float()
        if not audio.is_cuda:
            if lengths is not None:
                raise RuntimeError("hifiganBiasRemover: per-item lengths need the HIP kernels (CUDA tensors)")
            spec, angles = self.stft.transform(audio)
            return self.stft.inverse(torch.clamp(spec - self.bias_spec * strength, 0.0), angles)
        s = self.stft
        if lengths is None:
            re, im = _stft.analysis(audio, s.tables(), s.filter_length, s.hop_length, want=("re", "im"))
            return _stft.synthesis(re, im, s.tables(), s.filter_length, s.hop_length, mode=1, bias=self.bias_spec, strength=strength,
                                   windowed=s.window is not None)
        re, im, frames = _stft.analysis(audio, s.tables(), s.filter_length, s.hop_length, want=("re", "im"), lengths=lengths)
        return _stft.synthesis(re, im, s.tables(), s.filter_length, s.hop_length, mode=1, bias=self.bias_spec, strength=strength,
                               windowed=s.window is not None, lengths=frames)


class waveglowBiasRemover(torch.nn.Module):
    """Removes model bias from audio produced with WaveGlow (bias_remover.py:38-74).  `model_path`: the checkpoint the reference
    loads, ``torch.load(model_path)['model']`` being the module (its classes must be importable: see INTEGRATION.md for the
    ``glow`` alias); an addition: an already-built WaveGlow module is taken as it is.  GPU only, like the reference."""

    def __init__(self, model_path='Outdir/waveglow_256channels.pt', filter_length=1024, n_overlap=4, win_length=1024, mode='zeros'):
        super().__init__()
        if mode not in ("zeros", "normal"):
            raise Exception("Mode {} if not supported".format(mode))
        self.stft = STFT(filter_length=filter_length, hop_length=int(filter_length / n_overlap), win_length=win_length).cuda()
        if isinstance(model_path, torch.nn.Module):
            waveglow = model_path.cuda().eval()
        else:
            waveglow = torch.load(model_path, weights_only=False)['model'].cuda().eval()
        w = waveglow.upsample.weight
        mel_input = (torch.zeros if mode == 'zeros' else torch.randn)((1, 80, 88), dtype=w.dtype, device=w.device)
        with torch.no_grad():
            bias_audio = waveglow.infer(mel_input, sigma=0.0).float()           # [1, 88 * 256]
            bias_spec, _ = self.stft.transform(bias_audio)
        self.register_buffer('bias_spec', bias_spec[:, :, 0][:, :, None].clone())

    def forward(self, audio, strength=0.1):
        """audio [B, T] -> the first item, denoised: [hop * (T // hop)], as the reference's ``audio_denoised[:, 0][0]``."""
        s = self.stft
        audio = audio.cuda().float()
        re, im = _stft.analysis(audio, s.tables(), s.filter_length, s.hop_length, want=("re", "im"))
        audio_denoised = _stft.synthesis(re, im, s.tables(), s.filter_length, s.hop_length, mode=1, bias=self.bias_spec, strength=strength,
                                         windowed=s.window is not None)
        return audio_denoised[:, 0][0]
