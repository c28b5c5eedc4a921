"""BERT sentence encoder on the GPU: token ids -> last hidden state / [CLS] vector (csrc/bert.hip, include/t2amd.h).

What the reference computes on the CPU in data_utils.py:28-46 (get_embedding_cls), one sentence at a time, for every
sentence it speaks or scores.  Here a ragged batch of sentences runs packed (no padding, no mask) in exact fp32:

    enc = BertEncoder.from_model(bert_model)          # or .from_state_dict(sd, config_dict)
    cls = enc.cls([ids_0, ids_1, ...])                # [B, H] on the GPU
    hid = enc.hidden([ids_0, ids_1, ...])             # list of [len_b, H]

The semantics are BertModel(input_ids, attention_mask = the sentence's own tokens, token_type_ids = 0), last hidden
state: full attention within a sentence (INTEGRATION.md has the paragraph on why).  Inference only: no gradient.

Ids come from a host tokenizer, as lists or CPU tensors, and are validated on the host before anything is uploaded
(0 <= id < vocab, 1 <= len <= min(512, max_pos)): the kernels index the tables without checks.  `transformers` is never
imported here; from_model only reads `.config` and `.state_dict()` of what it is given."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L

MAX_LEN = 512
_LAYER_KEYS = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense", "attention.output.LayerNorm",
               "intermediate.dense", "output.dense", "output.LayerNorm")


def state_dict_keys(layers: int):
    """The state-dict names t2_bert_pack takes, in its order (no `bert.` prefix; the pooler is not part of the encoder)."""
    keys = ["embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight",
            "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
    for i in range(layers):
        for k in _LAYER_KEYS:
            keys += [f"encoder.layer.{i}.{k}.weight", f"encoder.layer.{i}.{k}.bias"]
    return keys


def validate_ids(ids_per_sentence, vocab: int, max_pos: int):
    """Host check of a batch of id sequences; returns (ids int32 [total], cu_seqlens int32 [B+1], max_len) as numpy arrays.
    Raises ValueError for an empty batch, an empty or over-long sentence or an id outside the vocabulary."""
    limit = min(MAX_LEN, int(max_pos))
    seqs = []
    for b, s in enumerate(ids_per_sentence):
        a = s.detach().cpu().numpy() if torch.is_tensor(s) else np.asarray(s)
        if a.ndim != 1 or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
            raise ValueError(f"bert: sentence {b} must be a 1-D sequence of integer ids, got shape {tuple(a.shape)} dtype {a.dtype}")
        if not 1 <= a.size <= limit:
            raise ValueError(f"bert: sentence {b} has {a.size} tokens, the encoder takes 1..{limit}")
        a = a.astype(np.int64)
        if a.min() < 0 or a.max() >= vocab:
            raise ValueError(f"bert: sentence {b} holds id {int(a.min() if a.min() < 0 else a.max())}, outside the vocabulary 0..{vocab - 1}")
        seqs.append(a)
    if not seqs:
        raise ValueError("bert: an empty batch")
    cu = np.zeros(len(seqs) + 1, dtype=np.int32)
    np.cumsum([len(a) for a in seqs], out=cu[1:])
    return np.concatenate(seqs).astype(np.int32), cu, max(len(a) for a in seqs)


class BertEncoder:
    """Packed weights of one BERT encoder on one GPU.  The weights go up on first use; workspaces are kept per batch shape
    class and grow as needed."""

    def __init__(self, tensors, config: L.BertConfig, device="cuda"):
        self.config = config
        self.device = torch.device(device)
        self._host = tensors            # fp32 CPU tensors in pack order, dropped once packed
        self._packed = None
        self._ws = None
        L.bert_plan(config, 1, 1, 1, True)           # refuses an unsupported configuration by name, without a device

    @classmethod
    def from_state_dict(cls, sd, config, device="cuda"):
        """sd: a BertModel / BertFor* state dict (keys with or without a `bert.` prefix; pooler and heads are ignored).
        config: a dict (or object) with hidden_size, num_hidden_layers, num_attention_heads, intermediate_size, vocab_size,
        max_position_embeddings, type_vocab_size, layer_norm_eps."""
        cfg = L.bert_config(config)
        pre = "" if "embeddings.word_embeddings.weight" in sd else "bert."
        tensors = []
        for k in state_dict_keys(cfg.layers):
            if pre + k not in sd:
                raise KeyError(f"bert: the state dict has no '{pre + k}'")
            tensors.append(sd[pre + k].detach().to("cpu", torch.float32).contiguous())
        H, I = cfg.hidden, cfg.intermediate
        want = [(cfg.vocab, H), (cfg.max_pos, H), (cfg.type_vocab, H), (H,), (H,)]
        for _ in range(cfg.layers):
            want += [(H, H), (H,)] * 4 + [(H,), (H,), (I, H), (I,), (H, I), (H,), (H,), (H,)]
        for k, t, w in zip(state_dict_keys(cfg.layers), tensors, want):
            if tuple(t.shape) != w:
                raise ValueError(f"bert: '{k}' has shape {tuple(t.shape)}, the configuration says {w}")
        return cls(tensors, cfg, device)

    @classmethod
    def from_model(cls, bert_model, device=None):
        """A transformers BertModel (or anything with .config and .state_dict() in its naming).  device: default the model's
        own when it is on a GPU, else cuda."""
        if device is None:
            p = next(bert_model.parameters())
            device = p.device if p.is_cuda else "cuda"
        return cls.from_state_dict(bert_model.state_dict(), bert_model.config, device)

    # ------------------------------------------------------------------------------------------------------------
    def _ensure_packed(self):
        if self._packed is None:
            with torch.cuda.device(self.device):
                info = L.bert_plan(self.config, 1, 1, 1, True)
                dev = [t.to(self.device) for t in self._host]
                packed = torch.empty(info.packed_floats, dtype=torch.float32, device=self.device)
                ptrs = (C.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
                L.check(L.lib().t2_bert_pack(C.byref(self.config), ptrs, len(dev), L.ptr(packed), L.stream()))
                torch.cuda.current_stream().synchronize()          # the copies read `dev`, which goes away here
            self._packed, self._host = packed, None
        return self._packed

    def _run(self, ids_per_sentence, want_hidden: bool):
        ids, cu, max_len = validate_ids(ids_per_sentence, self.config.vocab, self.config.max_pos)       # before any device call
        B, total, H = len(cu) - 1, int(ids.size), self.config.hidden
        info = L.bert_plan(self.config, B, total, max_len, not want_hidden)
        packed = self._ensure_packed()
        with torch.cuda.device(self.device), torch.no_grad():
            up = torch.from_numpy(np.concatenate([ids, cu])).to(self.device, non_blocking=True)
            if self._ws is None or self._ws.numel() * 4 < info.workspace_bytes:
                self._ws = torch.empty((info.workspace_bytes + 3) // 4, dtype=torch.float32, device=self.device)
            out_cls = torch.empty(B, H, dtype=torch.float32, device=self.device)
            out_hidden = torch.empty(total, H, dtype=torch.float32, device=self.device) if want_hidden else None
            args = L.BertFwdArgs(B, total, max_len, L.ptr(packed), up.data_ptr(), up.data_ptr() + 4 * total, L.ptr(out_hidden), L.ptr(out_cls),
                                 L.ptr(self._ws), self._ws.numel() * 4)
            L.check(L.lib().t2_bert_forward(C.byref(self.config), C.byref(args), L.stream()))
        return out_cls, out_hidden, cu

    def cls(self, ids_per_sentence) -> torch.Tensor:
        """[B, H]: the last hidden state of every sentence's first token.  The last layer runs for those rows only."""
        return self._run(ids_per_sentence, False)[0]

    def hidden(self, ids_per_sentence):
        """The last hidden state of every sentence: a list of [len_b, H] views of one packed tensor."""
        _, hid, cu = self._run(ids_per_sentence, True)
        return [hid[int(cu[b]):int(cu[b + 1])] for b in range(len(cu) - 1)]
