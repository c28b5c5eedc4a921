"""Plain-torch restatement of the BERT encoder (embeddings, post-LayerNorm transformer layers, last hidden state), one
sentence at a time with full attention inside it, in any dtype: the truth (fp64) and the fp32 yardstick of the BERT
tests.  Also the seeded weights and tokens the tests share; nothing here needs transformers."""
import math

import torch

SMALL = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=100,
             max_position_embeddings=520, type_vocab_size=2, layer_norm_eps=1e-12)
BASE = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, vocab_size=128,
            max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12)
_LINEARS = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense", "intermediate.dense", "output.dense")


def make_weights(cfg, seed=0):
    """A state dict with the checkpoint's key names (no `bert.` prefix, no pooler), fp32, from a seeded CPU generator.
    Activations stay O(1) and attention scores reach a few units; LayerNorm weights and biases are perturbed."""
    g = torch.Generator().manual_seed(seed)
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {"embeddings.word_embeddings.weight": rn(cfg["vocab_size"], H), "embeddings.position_embeddings.weight": 0.5 * rn(cfg["max_position_embeddings"], H),
          "embeddings.token_type_embeddings.weight": 0.5 * rn(cfg["type_vocab_size"], H)}
    def ln(name):
        sd[name + ".weight"] = 1.0 + 0.1 * rn(H)
        sd[name + ".bias"] = 0.1 * rn(H)
    ln("embeddings.LayerNorm")
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        for name in _LINEARS:
            out, inp = (I, H) if name == "intermediate.dense" else (H, I) if name == "output.dense" else (H, H)
            scale = 1.5 if name in _LINEARS[:2] else 1.0
            sd[p + name + ".weight"] = scale / math.sqrt(inp) * rn(out, inp)
            sd[p + name + ".bias"] = 0.1 * rn(out)
        ln(p + "attention.output.LayerNorm")
        ln(p + "output.LayerNorm")
    return sd


def tokens(lengths, seed=0, vocab=100):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (int(n),), generator=g).tolist() for n in lengths]


def layer_norm(x, w, b, eps):
    d = x - x.mean(-1, keepdim=True)
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(q, k, v, heads):
    """softmax(q k^T / sqrt(d)) v per head; q [n, H], k and v [L, H]."""
    n, H = q.shape
    d = H // heads
    qh, kh, vh = (t.reshape(-1, heads, d).transpose(0, 1) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(1, 2) / math.sqrt(d), dim=-1)
    return (p @ vh).transpose(0, 1).reshape(n, H)


def encode(sd, cfg, ids, dtype=torch.float64):
    """Last hidden state [len, H] of one sentence."""
    W = lambda k: sd[k].to(dtype)
    eps, heads = cfg["layer_norm_eps"], cfg["num_attention_heads"]
    ids = torch.as_tensor(ids, dtype=torch.long)
    x = W("embeddings.word_embeddings.weight")[ids] + W("embeddings.token_type_embeddings.weight")[0] + W("embeddings.position_embeddings.weight")[:len(ids)]
    x = layer_norm(x, W("embeddings.LayerNorm.weight"), W("embeddings.LayerNorm.bias"), eps)
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        lin = lambda t, name: t @ W(p + name + ".weight").T + W(p + name + ".bias")
        ctx = attention(lin(x, "attention.self.query"), lin(x, "attention.self.key"), lin(x, "attention.self.value"), heads)
        x = layer_norm(lin(ctx, "attention.output.dense") + x, W(p + "attention.output.LayerNorm.weight"), W(p + "attention.output.LayerNorm.bias"), eps)
        y = lin(gelu(lin(x, "intermediate.dense")), "output.dense")
        x = layer_norm(y + x, W(p + "output.LayerNorm.weight"), W(p + "output.LayerNorm.bias"), eps)
    return x


def encode_batch(sd, cfg, ids_per_sentence, dtype=torch.float64):
    return [encode(sd, cfg, ids, dtype) for ids in ids_per_sentence]


def truth_and_dev(sd, cfg, ids_per_sentence):
    """(fp64 hidden states per sentence, dev_ref = max |fp32 - fp64| of this statement over all of them)."""
    with torch.no_grad():
        t64 = encode_batch(sd, cfg, ids_per_sentence, torch.float64)
        t32 = encode_batch(sd, cfg, ids_per_sentence, torch.float32)
    return t64, max(float((a.double() - b).abs().max()) for a, b in zip(t32, t64))
