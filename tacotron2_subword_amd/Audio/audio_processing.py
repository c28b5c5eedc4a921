"""Audio/audio_processing.py of the reference: the names of tacotron2_subword_amd.audio_processing."""
from ..audio_processing import dynamic_range_compression, dynamic_range_decompression, griffin_lim, window_sumsquare  # noqa: F401
