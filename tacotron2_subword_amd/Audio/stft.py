"""Audio/stft.py of the reference: STFT and TacotronSTFT, which are tacotron2_subword_amd.stft's here.  Where the reference
moves the framing conv1d to the GPU and back (Audio/stft.py:66-70), TacotronSTFT.mel_spectrogram runs the whole log-mel
formula in one kernel when its input is a CUDA tensor."""
from ..stft import STFT, TacotronSTFT, log_mel, mel_filterbank  # noqa: F401
