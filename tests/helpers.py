"""Shared helpers for the GPU parity tests (oracle side on CPU, HIP side through the C ABI)."""
import os

import numpy as np
import torch

from oracle import recipe
from oracle import tacotron2_oracle as O

SMA, LSA, FA2, GMM, DCA = "StepwiseMonotonicAttention", "LSA", "ForwardAttentionV2", "GMMAttention", "DynamicConvolutionAttention"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def hp_for(att=SMA, **over):
    hp = O.default_hparams()
    hp["attention"] = att
    hp.update(over)
    return hp


def tiny_hp(att=SMA):
    """Smallest dims the kernels accept (multiples of 64 for the LSTM segments)."""
    return hp_for(att, n_mel_channels=8, symbols_embedding_dim=64, encoder_embedding_dim=64, BERT_embedding_dim=24,
                  decoder_rnn_dim=64, prenet_dim=64, attention_rnn_dim=128, attention_dim=16,
                  attention_location_n_filters=4, attention_location_kernel_size=5, postnet_embedding_dim=64,
                  n_symbols=20, sub_n_symbols=30)


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def to_dev(P, device="cuda"):
    return {k: v.detach().to(device).contiguous() for k, v in P.items()}


def maxabs(a, b):
    a = a.detach().cpu().double() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a)).double()
    b = b.detach().cpu().double() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max())


def oracle_memories(P, hp, x, training=False, rnd=None):
    """CPU oracle encoder side: memory, memory_sub (what Decoder.forward receives)."""
    text, tl, bl, mels, _, ol, sub_ids, pcls, bcls = x
    with torch.no_grad():
        mem = O.front_end(P, hp, text, tl, pcls, "phone", training, rnd)
        mem_sub = O.front_end(P, hp, sub_ids, bl, bcls, "sub", training, rnd)
    return mem, mem_sub


def _partition(M):
    """The row partition of the fixed-order column reductions (csrc/common.h, col_slabs): (slabs, rows per slab)."""
    slabs = 64 if M >= 64 * 64 else (M // 64 if M >= 64 else 1)
    return slabs, (M + slabs - 1) // slabs


def ordered_colsum(X):
    """X: [M, N] float32 on the CPU -> the column sums in the documented order, float32."""
    assert X.dtype == torch.float32 and X.device.type == "cpu"
    M, N = X.shape
    slabs, rows = _partition(M)
    steps = (rows + 3) // 4
    pad = torch.zeros(slabs * steps * 4 + rows * slabs, N)          # row index m0 + 4*k + p may run past the slab: masked below
    pad[:M] = X
    s = torch.arange(slabs).view(slabs, 1)
    p = torch.arange(4).view(1, 4)
    acc = torch.zeros(slabs, 4, N)
    for k in range(steps):
        r = 4 * k + p                                               # row inside the slab, [1, 4]
        m = s * rows + r                                            # [slabs, 4]
        valid = (r < rows) & (m < M)
        acc = torch.where(valid.unsqueeze(-1), acc + pad[m], acc)
    slab = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    out = torch.zeros(N)
    for i in range(slabs):
        out = out + slab[i]
    return out
