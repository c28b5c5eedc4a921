"""GPU tests of the BERT sentence encoder (csrc/bert.hip, tacotron2_subword_amd/bert.py) and of the GELU epilogue of the
GEMM layer, against fp64 truth from tests/bert_ref.py.  No transformers, nothing from the reference.

Bound of every check: 4 * max(dev_ref, 2^-23 * max|truth|).  dev_ref is the deviation of the same torch-op statement in
fp32 from itself in fp64 on that case (computed here on the CPU; for the recorded cases the `dev` of
tests/golden/bert.npz); the floor is one fp32 rounding of the output.  The factor 4: a second fp32 summation order (a
consistent permutation of the hidden units, small and base configurations, lengths 2..512) lay at 0.66 - 1.71 x dev_ref
from fp64, so 2 would be marginal and 4 leaves about 2.3 x over the worst seen.  Every check prints err / bound."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import bert_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert.npz")
DEV = "cuda"
WORST = {}
RAGGED = [2, 65, 33, 7, 64, 512, 1]
ATTN_LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 129, 512]


def LIB():
    from tacotron2_subword_amd import _lib
    return _lib


def check(group, what, got, truth, dev):
    truth = torch.as_tensor(truth, dtype=torch.float64)
    got = got.detach().double().cpu()
    assert got.shape == truth.shape, (group, what, got.shape, truth.shape)
    err = float((got - truth).abs().max())
    bound = 4.0 * max(float(dev), 2.0 ** -23 * float(truth.abs().max()))
    share = err / bound
    WORST[group] = max(WORST.get(group, 0.0), share)
    print(f"[{group}] {what}: err {err:.3e} bound {bound:.3e} err/bound {share:.3f} (worst of group {WORST[group]:.3f})")
    assert err <= bound, (group, what, err, bound)


def dev_of(f):
    """(truth, dev_ref) of a statement f(dtype)."""
    with torch.no_grad():
        t64, t32 = f(torch.float64), f(torch.float32)
    return t64, float((t32.double() - t64).abs().max())


def cu_of(lengths):
    return torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------
# GELU epilogue
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 63, 130])
def test_gemm_gelu(M):
    L = LIB()
    N, K = 256, 128
    g = torch.Generator().manual_seed(M)
    x, w, b = torch.randn(M, K, generator=g), 2.0 / K ** 0.5 * torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    truth, dev = dev_of(lambda dt: R.gelu(x.to(dt) @ w.to(dt).T + b.to(dt)))
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    out = torch.full((M, N), float("nan"), device=DEV)
    a = L.GemmArgs(L.ptr(xd), L.ptr(wd), L.ptr(out), M, N, K, K, 1, K, 1, N, 1, 0, 0, 0, 1.0, 0.0, L.ptr(bd), 3, 0, 0, None, 0, 0)
    L.check(L.lib().t2_gemm_ex(C.byref(a), L.stream()))
    check("gemm_gelu", f"M={M}", out, truth, dev)
    assert float(truth.min()) < -0.1 and float(truth.max()) > 3.0          # both branches of the curve are exercised


# ---------------------------------------------------------------------------------------------------------------
# attention alone
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attention_case():
    heads, H = 2, 128
    total = sum(ATTN_LENGTHS)
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(total, 3 * H, generator=g)
    qkv[:, :2 * H] *= 2.6                                                 # scores q.k / 8 have a deviation of 6.8: the largest reach about 30
    cu = cu_of(ATTN_LENGTHS)
    def f(dt):
        rows = []
        for b in range(len(ATTN_LENGTHS)):
            s = qkv[int(cu[b]):int(cu[b + 1])].to(dt)
            rows.append(R.attention(s[:, :H], s[:, H:2 * H], s[:, 2 * H:], heads))
        return torch.cat(rows)
    truth, dev = dev_of(f)
    smax = max(float((qkv[int(cu[b]):int(cu[b + 1]), :64].double() @ qkv[int(cu[b]):int(cu[b + 1]), H:H + 64].double().T).abs().max()) / 8
               for b in range(len(ATTN_LENGTHS)))
    return heads, H, qkv, cu, truth, dev, smax


def run_attention(q, k, v, ldq, ldkv, cu, B, heads, total, max_len, first, out):
    L = LIB()
    a = L.BertAttentionArgs(B, heads, total, max_len, int(first), q, k, v, ldq, ldkv, ldkv, L.ptr(cu), L.ptr(out), out.shape[1])
    L.check(L.lib().t2_bert_attention(C.byref(a), L.stream()))


def test_attention_ragged():
    heads, H, qkv, cu, truth, dev, smax = attention_case()
    print(f"largest |score| {smax:.1f}")
    assert 20 < smax < 60
    d, cud = qkv.to(DEV), cu.to(DEV)
    out = torch.full((d.shape[0], H), float("nan"), device=DEV)
    p = d.data_ptr()
    run_attention(p, p + 4 * H, p + 8 * H, 3 * H, 3 * H, cud, len(ATTN_LENGTHS), heads, d.shape[0], 512, False, out)
    check("attention", "all query rows", out, truth, dev)


def test_attention_first_query_only():
    heads, H, qkv, cu, truth, dev, _ = attention_case()
    first = cu[:-1].long()
    d, cud = qkv.to(DEV), cu.to(DEV)
    q = d[first.to(DEV), :H].contiguous()
    out = torch.full((len(ATTN_LENGTHS), H), float("nan"), device=DEV)
    p = d.data_ptr()
    run_attention(q.data_ptr(), p + 4 * H, p + 8 * H, H, 3 * H, cud, len(ATTN_LENGTHS), heads, d.shape[0], 512, True, out)
    check("attention", "first query of every sentence", out, truth[first], dev)


def test_attention_leaves_uncovered_rows_alone():
    """max_len below a sentence's length: that sentence is skipped, nothing is written past its rows."""
    heads, H, qkv, cu, truth, dev, _ = attention_case()
    d, cud = qkv.to(DEV), cu.to(DEV)
    out = torch.full((d.shape[0], H), 7.0, device=DEV)
    p = d.data_ptr()
    run_attention(p, p + 4 * H, p + 8 * H, 3 * H, 3 * H, cud, len(ATTN_LENGTHS), heads, d.shape[0], 129, False, out)
    n = int(cu[-2])
    check("attention", "sentences within max_len", out[:n], truth[:n], dev)
    assert bool((out[n:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------
# the LayerNorm kernels alone
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 128, 768, 1024])
def test_row_layernorm(H):
    L = LIB()
    rows, eps = 7, 1e-12                                                  # 7 rows: the last workgroup holds 3 of its 4
    g = torch.Generator().manual_seed(H)
    x = 3.0 * torch.randn(rows, H, generator=g) + 1.0
    x[3] = 1.25                                                           # variance 0 (the sums are exact in fp32): eps decides, out = bias
    w, b = 1.0 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    truth, dev = dev_of(lambda dt: R.layer_norm(x.to(dt), w.to(dt), b.to(dt), eps))
    assert torch.equal(truth[3], b.double())
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    out = torch.full((rows + 1, H), float("nan"), device=DEV)
    a = L.BertLayernormArgs(rows, H, eps, L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(out))
    L.check(L.lib().t2_bert_layernorm(C.byref(a), L.stream()))
    check("layernorm", f"H={H} to another buffer", out[:rows], truth, dev)
    assert bool(torch.isnan(out[rows]).all())                             # nothing behind the last row
    assert torch.equal(out[3].cpu(), b)
    a = L.BertLayernormArgs(rows, H, eps, L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(xd))
    L.check(L.lib().t2_bert_layernorm(C.byref(a), L.stream()))
    assert torch.equal(xd, out[:rows])                                    # in place: the same bits


@pytest.mark.parametrize("H", [64, 128, 768, 1024])
def test_embed_layernorm(H):
    L = LIB()
    lengths, vocab, max_pos, eps = [5, 1, 4], 11, 9, 1e-12                 # 5 positions: the second workgroup of a sentence holds 1 of its 4 rows
    g = torch.Generator().manual_seed(H + 1)
    word, pos, typ = torch.randn(vocab, H, generator=g), 0.5 * torch.randn(max_pos, H, generator=g), 0.5 * torch.randn(2, H, generator=g)
    word[7], pos[0], typ[0] = 0.5, 0.5, 0.25                              # token 7 at position 0: a constant row, 1.25
    ids = [[1, 2, 3, 4, 10], [7], [0, 9, 7, 5]]
    flat = torch.tensor(sum(ids, []), dtype=torch.int32)
    positions = torch.tensor(sum([list(range(n)) for n in lengths], []))
    w, b = 1.0 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    truth, dev = dev_of(lambda dt: R.layer_norm(word.to(dt)[flat.long()] + typ.to(dt)[0] + pos.to(dt)[positions], w.to(dt), b.to(dt), eps))
    assert torch.equal(truth[5], b.double())
    dv = [t.to(DEV) for t in (flat, cu_of(lengths), word, pos, typ, w, b)]
    total = sum(lengths)
    out = torch.full((total + 1, H), float("nan"), device=DEV)
    a = L.BertEmbedLnArgs(len(lengths), total, max(lengths), H, eps, *[L.ptr(t) for t in dv], L.ptr(out))
    L.check(L.lib().t2_bert_embed_ln(C.byref(a), L.stream()))
    check("embed_ln", f"H={H}", out[:total], truth, dev)
    assert bool(torch.isnan(out[total]).all())
    assert torch.equal(out[5].cpu(), b)


# ---------------------------------------------------------------------------------------------------------------
# the whole encoder, small configuration
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def small():
    from tacotron2_subword_amd.bert import BertEncoder
    z = golden()
    sd = R.make_weights(R.SMALL, int(z["seed"]))
    return sd, BertEncoder.from_state_dict(sd, R.SMALL)


@functools.lru_cache(maxsize=None)
def ragged_case():
    sd, _ = small()
    ids = R.tokens(RAGGED, seed=3, vocab=R.SMALL["vocab_size"])
    truth, dev = R.truth_and_dev(sd, R.SMALL, ids)
    return ids, truth, dev


def test_encoder_recorded_cases():
    z = golden()
    sd, enc = small()
    n = len(z["texts"])
    ids = [z[f"ids_{i}"].tolist() for i in range(n)]
    hid, cls = enc.hidden(ids), enc.cls(ids)
    for i in range(n):
        truth = R.encode(sd, R.SMALL, ids[i])
        assert float((truth - torch.from_numpy(z[f"hidden_{i}"]).double()).abs().max()) <= float(z["dev"]) + float(z["win"])
        check("encoder_small", f"recorded {i} hidden ({len(ids[i])} tokens)", hid[i], truth, float(z["dev"]))
        check("encoder_small", f"recorded {i} cls", cls[i], truth[0], float(z["dev"]))


def test_encoder_ragged_hidden_and_cls():
    _, enc = small()
    ids, truth, dev = ragged_case()
    hid, cls = enc.hidden(ids), enc.cls(ids)
    assert cls.shape == (len(ids), R.SMALL["hidden_size"]) and cls.is_cuda and cls.dtype == torch.float32
    for i, t in enumerate(truth):
        check("encoder_small", f"ragged {len(ids[i])} tokens hidden", hid[i], t, dev)
        check("encoder_small", f"ragged {len(ids[i])} tokens cls", cls[i], t[0], dev)
        check("encoder_small", f"ragged {len(ids[i])} tokens cls against row 0 of hidden", cls[i], hid[i][0].double().cpu(), dev)


def test_encoder_batch_of_one():
    _, enc = small()
    ids, truth, dev = ragged_case()
    for i in (0, 2, 6):
        check("encoder_small", f"alone, {len(ids[i])} tokens hidden", enc.hidden([ids[i]])[0], truth[i], dev)
        check("encoder_small", f"alone, {len(ids[i])} tokens cls", enc.cls([ids[i]])[0], truth[i][0], dev)


def test_encoder_order_of_sentences_changes_no_bit():
    _, enc = small()
    ids, _, _ = ragged_case()
    perm = [5, 0, 6, 3, 1, 4, 2]
    h0, c0 = enc.hidden(ids), enc.cls(ids).clone()
    h0 = [t.clone() for t in h0]
    h1, c1 = enc.hidden([ids[p] for p in perm]), enc.cls([ids[p] for p in perm])
    for j, p in enumerate(perm):
        assert torch.equal(h1[j], h0[p]), (j, p)
        assert torch.equal(c1[j], c0[p]), (j, p)


# ---------------------------------------------------------------------------------------------------------------
# the whole encoder at base width, through data_utils
# ---------------------------------------------------------------------------------------------------------------
class StubTokenizer:
    """tokenize / convert_tokens_to_ids as get_embedding_cls uses them: words "w<id>", [CLS] = 1, [SEP] = 2."""

    def tokenize(self, text):
        return text.split()

    def convert_tokens_to_ids(self, toks):
        return [1 if t == "[CLS]" else 2 if t == "[SEP]" else int(t[1:]) for t in toks]


def test_encoder_base_width_through_data_utils():
    from tacotron2_subword_amd import data_utils as D
    from tacotron2_subword_amd.bert import BertEncoder
    sd = R.make_weights(R.BASE, 4)
    enc = BertEncoder.from_state_dict(sd, R.BASE)
    body = R.tokens([0, 35, 68], seed=9, vocab=R.BASE["vocab_size"])
    texts = [" ".join(f"w{t}" for t in s) for s in body]
    texts[1] = "<en>" + texts[1] + "</en>"
    ids = [[1] + s + [2] for s in body]
    assert [len(s) for s in ids] == [2, 37, 70]
    truth, dev = R.truth_and_dev(sd, R.BASE, ids)
    tok = StubTokenizer()
    batch = D.get_embedding_cls_batch(texts, enc, tok)
    assert batch.shape == (3, 768) and batch.is_cuda
    for i in range(3):
        check("encoder_base", f"batch, {len(ids[i])} tokens cls", batch[i], truth[i][0], dev)
    one = D.get_embedding_cls(texts[1], enc, tok)
    assert one.shape == (1, 768)
    check("encoder_base", "get_embedding_cls, 37 tokens", one[0], truth[1][0], dev)
