"""WaveGlow on the MI355X: the module name the reference's checkpoints and scripts use (``glow``), on the HIP kernels of
csrc/waveglow.hip.  Inference only, fp32, no CPU path."""
from .glow import WN, Invertible1x1Conv, WaveGlow  # noqa: F401
