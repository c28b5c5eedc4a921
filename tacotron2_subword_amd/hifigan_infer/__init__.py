"""HiFi-GAN generator on the MI355X: the module names the reference's scripts import (``hifigan_infer.hifigan_model``,
``hifigan_infer.hifigan_utils``), on the HIP kernels of csrc/vocoder.hip.  Inference only, fp32, no CPU path."""
from .hifigan_model import Generator, ResBlock1, ResBlock2  # noqa: F401
from .hifigan_utils import AttrDict, get_padding, load_checkpoint  # noqa: F401
