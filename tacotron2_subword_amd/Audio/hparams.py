"""Audio/hparams.py of the reference: the front end's settings as module attributes (max_wav_value, sampling_rate,
filter_length, hop_length, win_length, n_mel_channels, mel_fmin, mel_fmax).  The reference keeps a second copy of the values
of its hparams.py there; here they are read from this package's hparams, so the two cannot drift apart."""
from ..hparams import create_hparams as _create_hparams

_NAMES = ("max_wav_value", "sampling_rate", "filter_length", "hop_length", "win_length", "n_mel_channels", "mel_fmin", "mel_fmax")
globals().update({k: getattr(_create_hparams(), k) for k in _NAMES})
