"""What the reference's scripts take from hifigan_infer/hifigan_utils.py and from their own copies of AttrDict
(inference.py, best_checkpoint.py, streamlitNews.py, logger.py each define one).  No plotting, no matplotlib."""
import os

import torch


class AttrDict(dict):
    """A dict whose keys are also attributes: ``h = AttrDict(json.loads(text))``, then ``h.upsample_rates``."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


def get_padding(kernel_size, dilation=1):
    return int((kernel_size * dilation - dilation) / 2)


def load_checkpoint(filepath, device):
    assert os.path.isfile(filepath)
    return torch.load(filepath, map_location=device)
