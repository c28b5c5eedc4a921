"""Dev tool: the BERT sentence encoder on the GPU, HIP path against the torch-op statement, in one process.

  python scripts/time_bert.py [--rounds 5] [--warmup 1] [--timed 10] [--seed 3]

Cases, both at base size (12 layers, hidden 768, 12 heads, intermediate 3072; seeded random weights, vocabulary 128):
B = 1 at 40 tokens, and B = 64 ragged at 20..100 tokens.  One call = ids on the host -> [B, 768] CLS vectors on the GPU.
"hip" is tacotron2_subword_amd.bert.BertEncoder.cls (csrc/bert.hip: packed rows, CLS-only last layer); "torch" is the
same computation in torch ops on the same GPU in fp32, padded to the longest sentence and masked: transformers'
BertModel when it imports, else the padded restatement below on tests/bert_ref.py's weights.  The two alternate: per
round --warmup calls, then --timed calls each between its own pair of events (5 warm-up and 50 timed calls per path by
default); reported: the median of all timed calls and their min-to-max spread.  The HIP path counts as faster when its
median lies below the other's by more than the larger of the two spreads.  Then the kernels alone at the B = 64 shape,
the same way: the four products of a layer through t2_gemm_ex and the kernels of csrc/bert.hip, with the share of the
157 TFLOP/s fp32-matrix peak for the products.  A run without a GPU fails."""
import argparse, ctypes as C, math, os, statistics, sys
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--timed", type=int, default=10)
ap.add_argument("--seed", type=int, default=3)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import torch.nn.functional as F
import bert_ref as R
from tacotron2_subword_amd import _lib as L
from tacotron2_subword_amd.bert import BertEncoder

assert torch.cuda.is_available(), "time_bert.py measures on the GPU: none found"
PEAK = 157e12
cfg = R.BASE
H, I, NL, NH = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"]
sd = R.make_weights(cfg, 4)
enc = BertEncoder.from_state_dict(sd, cfg)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(work):
    times = {name: [] for name, _ in work}
    for _ in range(a.rounds):
        for name, fn in work:
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            times[name] += [event_ms(fn) for _ in range(a.timed)]
    return times


def report(times, extra=None):
    stats = {}
    for name, v in times.items():
        med, spread = statistics.median(v), max(v) - min(v)
        stats[name] = (med, spread)
        print(f"{name:52s} {len(v):3d} calls  median {med:9.4f} ms  min {min(v):9.4f}  max {max(v):9.4f}  spread {spread:.4f} ms"
              + (f"  {extra[name]}" if extra and name in extra else ""), flush=True)
    return stats


try:
    from transformers import BertConfig, BertModel
    hf = BertModel(BertConfig(**cfg), add_pooling_layer=False)
    hf.load_state_dict(sd, strict=False)
    hf = hf.cuda().eval()
    torch_name = "torch (transformers BertModel, padded + masked)"

    def torch_hidden(tok, mask):
        return hf(input_ids=tok, attention_mask=mask, token_type_ids=torch.zeros_like(tok))[0]
except ImportError:
    dsd = {k: v.cuda() for k, v in sd.items()}
    torch_name = "torch (padded restatement of bert_ref, masked)"

    def torch_hidden(tok, mask):
        n = tok.shape[1]
        x = dsd["embeddings.word_embeddings.weight"][tok] + dsd["embeddings.token_type_embeddings.weight"][0] + dsd["embeddings.position_embeddings.weight"][:n]
        x = F.layer_norm(x, (H,), dsd["embeddings.LayerNorm.weight"], dsd["embeddings.LayerNorm.bias"], cfg["layer_norm_eps"])
        bias = (1.0 - mask[:, None, None, :].float()) * torch.finfo(torch.float32).min
        for i in range(NL):
            p = f"encoder.layer.{i}."
            lin = lambda t, name: F.linear(t, dsd[p + name + ".weight"], dsd[p + name + ".bias"])
            heads = lambda t: t.view(t.shape[0], n, NH, 64).transpose(1, 2)
            q, k, v = (heads(lin(x, "attention.self." + w)) for w in ("query", "key", "value"))
            ctx = (torch.softmax(q @ k.transpose(2, 3) / 8.0 + bias, -1) @ v).transpose(1, 2).reshape(-1, n, H)
            x = F.layer_norm(lin(ctx, "attention.output.dense") + x, (H,), dsd[p + "attention.output.LayerNorm.weight"], dsd[p + "attention.output.LayerNorm.bias"], cfg["layer_norm_eps"])
            y = lin(F.gelu(lin(x, "intermediate.dense")), "output.dense")
            x = F.layer_norm(y + x, (H,), dsd[p + "output.LayerNorm.weight"], dsd[p + "output.LayerNorm.bias"], cfg["layer_norm_eps"])
        return x


def torch_cls(ids):
    n = max(len(s) for s in ids)
    tok = torch.zeros(len(ids), n, dtype=torch.long)
    mask = torch.zeros(len(ids), n, dtype=torch.long)
    for b, s in enumerate(ids):
        tok[b, :len(s)] = torch.tensor(s)
        mask[b, :len(s)] = 1
    with torch.no_grad():
        return torch_hidden(tok.cuda(), mask.cuda())[:, 0]


g = torch.Generator().manual_seed(a.seed)
cases = [("B=1, 40 tokens", [40]), ("B=64 ragged, 20..100 tokens", torch.randint(20, 101, (64,), generator=g).tolist())]
for label, lengths in cases:
    ids = R.tokens(lengths, seed=a.seed, vocab=cfg["vocab_size"])
    total = sum(lengths)
    ours, theirs = enc.cls(ids), torch_cls(ids)
    flop = 2.0 * total * NL * (4 * H * H + 2 * H * I) + sum(4.0 * n * n * H for n in lengths) * NL
    print(f"--- {label}: {total} tokens (padded: {len(lengths) * max(lengths)}), {flop / 1e9:.1f} GFLOP unpadded; max |hip - torch| {float((ours - theirs).abs().max()):.3e} "
          f"(max |cls| {float(theirs.abs().max()):.2f})", flush=True)
    st = report(alternate([("hip  BertEncoder.cls", lambda: enc.cls(ids)), (torch_name, lambda: torch_cls(ids))]))
    (mh, sh), (mt, stt) = st["hip  BertEncoder.cls"], st[torch_name]
    margin = max(sh, stt)
    print(f"ratio torch / hip = {mt / mh:.2f}; hip median below torch median by {mt - mh:.4f} ms, larger spread {margin:.4f} ms: "
          f"{'FASTER (passes)' if mt - mh > margin else 'FAILS the condition'}; hip at {flop / (mh * 1e-3) / PEAK * 100:.1f} % of the fp32-matrix peak", flush=True)

# the kernels alone, at the B = 64 shape
lengths = cases[1][1]
B, T, max_len = len(lengths), sum(lengths), max(lengths)
dev = "cuda"
cu = torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32, device=dev)
idsd = torch.randint(0, cfg["vocab_size"], (T,), dtype=torch.int32, device=dev)
x, qkv, ctx, ffn = (torch.randn(T, n, device=dev) for n in (H, 3 * H, H, I))
wqkv, wo, w1, w2 = (torch.randn(n, k, device=dev) / math.sqrt(k) for n, k in ((3 * H, H), (H, H), (I, H), (H, I)))
bias = torch.randn(I, device=dev)
word, pos, typ, lw, lb = (sd[k].cuda() for k in ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
                                                  "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"))


def product(A, W, Cm, M, N, K, act, beta):
    args = L.GemmArgs(L.ptr(A), L.ptr(W), L.ptr(Cm), M, N, K, K, 1, K, 1, N, 1, 0, 0, 0, 1.0, beta, L.ptr(bias), act, 0, 0, None, 0, 0)
    return lambda: L.check(L.lib().t2_gemm_ex(C.byref(args), L.stream()))


def attention(first):
    q = x if first else qkv
    out = ctx
    args = L.BertAttentionArgs(B, NH, T, max_len, int(first), q.data_ptr(), qkv.data_ptr() + 4 * H, qkv.data_ptr() + 8 * H, H if first else 3 * H, 3 * H, 3 * H,
                               L.ptr(cu), L.ptr(out), H)
    return lambda: L.check(L.lib().t2_bert_attention(C.byref(args), L.stream()))


ln_args = L.BertLayernormArgs(T, H, 1e-12, L.ptr(x), L.ptr(lw), L.ptr(lb), L.ptr(ctx))
em_args = L.BertEmbedLnArgs(B, T, max_len, H, 1e-12, L.ptr(idsd), L.ptr(cu), L.ptr(word), L.ptr(pos), L.ptr(typ), L.ptr(lw), L.ptr(lb), L.ptr(ctx))
attn_flop = sum(4.0 * n * n * H for n in lengths)
work = [("product QKV      [T,768] x [2304,768]^T", product(x, wqkv, qkv, T, 3 * H, H, 0, 0.0), 2.0 * T * 3 * H * H, NL),
        ("product out      [T,768] x [768,768]^T + x", product(ctx, wo, x, T, H, H, 0, 1.0), 2.0 * T * H * H, NL),
        ("product FFN in   [T,768] x [3072,768]^T, GELU", product(x, w1, ffn, T, I, H, 3, 0.0), 2.0 * T * I * H, NL),
        ("product FFN out  [T,3072] x [768,3072]^T + x", product(ffn, w2, x, T, H, I, 0, 1.0), 2.0 * T * H * I, NL),
        ("t2_bert_attention, all query rows", attention(False), attn_flop, NL - 1),
        ("t2_bert_attention, first query only", attention(True), attn_flop / max_len, 1),
        ("t2_bert_layernorm [T,768]", lambda: L.check(L.lib().t2_bert_layernorm(C.byref(ln_args), L.stream())), 0.0, 2 * NL),
        ("t2_bert_embed_ln  [T,768]", lambda: L.check(L.lib().t2_bert_embed_ln(C.byref(em_args), L.stream())), 0.0, 1)]
print(f"--- kernels alone at B={B}, T={T} tokens, longest {max_len}", flush=True)
times = alternate([(n, f) for n, f, _, _ in work])
report(times, {n: (f"x{k} per call; " + (f"{fl / (statistics.median(times[n]) * 1e-3) / PEAK * 100:.1f} % of peak" if fl else "memory-bound")) for n, _, fl, k in work})
gemm_ms = sum(statistics.median(times[n]) * k for n, _, _, k in work[:4])
own_ms = sum(statistics.median(times[n]) * k for n, _, _, k in work[4:])
print(f"sum over a call (full layers): products {gemm_ms:.3f} ms, the kernels of bert.hip {own_ms:.3f} ms", flush=True)
info = L.bert_plan(enc.config, B, T, max_len, True)
print(f"plan: {info.launches} launches, workspace {info.workspace_bytes / 1e6:.1f} MB, packed weights {info.packed_floats * 4 / 1e6:.1f} MB", flush=True)
