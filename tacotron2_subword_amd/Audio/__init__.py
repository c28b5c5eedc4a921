"""The reference's `Audio` package under its own names (Audio/hparams.py, stft.py, audio_processing.py, tools.py): the mel
front end its scoring scripts call as `Audio.tools.get_mel` (softdtw.py:78-79, best_checkpoint.py:426-427).  The modules
are the project's own (tacotron2_subword_amd.stft, .audio_processing); on a GPU the mel comes from one launch of the log-mel
kernel (csrc/melspec.hip).  INTEGRATION.md shows the `sys.modules["Audio"]` alias with which those scripts run as written."""
from . import hparams, audio_processing, stft, tools  # noqa: F401
