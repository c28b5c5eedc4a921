"""Batched high-precision reference of the autoregressive decode loop (Decoder.inference, model.py:430-492), assembled
from the oracle's own pieces: O.DecState, O.prenet, O.decode_step, O.get_mask_from_lengths.  It carries no arithmetic of
its own.  The oracle's decoder_inference handles B == 1 without lengths; this one takes any batch, optional valid lengths
(masks made exactly as O.decoder_forward makes them) and optional prenet keep masks (applied as O.prenet applies them), runs
a fixed number of frames with no stop rule (the stop frame is derived from the returned gate) and also returns the prenet
activations, which the HIP loop leaves in its workspace."""
from collections import namedtuple

import torch

from oracle import tacotron2_oracle as O

DecodeRef = namedtuple("DecodeRef", "mel gate align align_sub p1 p2 p1s p2s")
KEEP_SITES = ("PRENET1", "PRENET2", "PRENET1_SUB", "PRENET2_SUB")      # order of `keep`


def cast_weights(P, dtype):
    return {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in P.items()}


def decode_ref(memory, memory_sub, P, hp, steps, mem_lengths=None, sub_lengths=None, keep=None, dtype=torch.float64):
    """memory [B,Tin,E], memory_sub [B,Tsub,E]; keep: None or four [steps,B,P] 0/1 tensors in KEEP_SITES order (row t is
    applied to the prenets that feed step t).  Returns DecodeRef(mel [B,steps,M], gate [B,steps], align [B,steps,Tin],
    align_sub [B,steps,Tsub], p1, p2, p1s, p2s [steps,B,P]: layer 1 / layer 2 of the phone and the sub-word prenet)."""
    P = cast_weights(P, dtype)
    memory, memory_sub = memory.detach().to(dtype), memory_sub.detach().to(dtype)
    B, Tin, Tsub = memory.shape[0], memory.shape[1], memory_sub.shape[1]
    mask = None if mem_lengths is None else ~O.get_mask_from_lengths(torch.as_tensor(mem_lengths, dtype=torch.long), Tin)
    mask_sub = None if sub_lengths is None else ~O.get_mask_from_lengths(torch.as_tensor(sub_lengths, dtype=torch.long), Tsub)
    w = [P[f"decoder.{n}.layers.{i}.linear_layer.weight"] for n in ("prenet", "prenet_bert") for i in (0, 1)]
    eye = torch.eye(hp["prenet_dim"], dtype=dtype)                  # relu(h1 @ I) == h1 exactly (h1 >= 0): layer 1 through O.prenet
    out = [[] for _ in DecodeRef._fields]
    with torch.no_grad():
        st = O.DecState(memory, memory_sub, mask, mask_sub, P, hp)
        x = memory.new_zeros(B, hp["n_mel_channels"])               # go frame
        for t in range(steps):
            k = [None] * 4 if keep is None else [m[t].to(dtype) for m in keep]
            xp, xb = O.prenet(x, w[0], w[1], k[0], k[1]), O.prenet(x, w[2], w[3], k[2], k[3])
            p1, p1s = O.prenet(x, w[0], eye, k[0], None), O.prenet(x, w[2], eye, k[2], None)
            m, g, a, ab = O.decode_step(st, xp, xb, P, hp)
            for o, v in zip(out, (m, g.squeeze(1), a, ab, p1, xp, p1s, xb)):
                o.append(v)
            x = m
    bt = lambda seq: torch.stack(seq).transpose(0, 1).contiguous()
    return DecodeRef(bt(out[0]), bt(out[1]), bt(out[2]), bt(out[3]), *(torch.stack(o) for o in out[4:]))


def first_crossing(gate, thr):
    """[B,steps] gate logits -> per item the first frame with sigmoid(gate) > thr, -1 if none (model.py:461,480)."""
    above = torch.sigmoid(gate) > thr
    return torch.where(above.any(1), above.float().argmax(1), torch.full((gate.shape[0],), -1))
