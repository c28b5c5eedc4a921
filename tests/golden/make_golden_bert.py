#!/usr/bin/env python3
"""Golden vectors for the BERT sentence encoder, recorded once on the CPU from the reference's own
data_utils.get_embedding_cls (imported here only, never by a test).  Usage: make_golden_bert.py <reference directory>;
writes bert.npz and bert_vocab.txt (the word pieces the recording's BertTokenizer used) next to this file.

The model is a transformers BertModel at the small configuration of tests/bert_ref.py with make_weights(SEED), so the
file holds no weights.  The reference calls bert_model(tokens, segments) positionally; a shim hands its second argument
on as token_type_ids, which is what the reference means.

Per text n: ids_n, sub_n (the reference's get_embedding on a tokenizers word-piece tokenizer of the same vocabulary),
cls_n (the reference's return, fp32 [1, H]), hidden_n (BertModel's fp32 last hidden state).  dev: max
|BertModel fp32 - BertModel fp64| over all hidden states; win: max |BertModel fp64 - bert_ref fp64|, asserted here to be
at rounding level."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bert_ref as R  # noqa: E402

SEED = 11
VOCAB = os.path.join(HERE, "bert_vocab.txt")
TEXTS = ["the cat sat on the mat", "<en>hello</en> world , this is a test", "", "singing birds are playing <en>in the garden</en> today !",
         "a", "unknownword and the rest . " * 6]
PIECES = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", ",", ".", "!", "?", "the", "a", "cat", "sat", "on", "mat", "hello", "world", "this", "is", "test",
          "sing", "##ing", "bird", "##s", "are", "play", "in", "garden", "to", "##day", "and", "rest", "un", "##known", "##word", "of", "it", "he", "she", "we",
          "you", "they", "was", "be", "not", "with", "for", "as", "at", "by", "from", "or", "an", "but", "all", "one", "two", "three", "four", "five", "six",
          "seven", "eight", "nine", "ten", "red", "blue", "green", "dog", "house", "tree", "sun", "moon", "star", "sky", "sea", "land", "fire", "water",
          "wind", "##ed", "##er", "##ly", "##est", "##en", "##es", "##y", "##al", "##ic", "##ion", "day", "night", "time", "year", "man", "woman", "child",
          "work", "life", "hand"]


class Positional:
    """bert_model(tokens, segments) as the reference writes it, with `segments` as token_type_ids."""

    def __init__(self, model):
        self.model = model

    def __call__(self, tokens, segments):
        return self.model(tokens, token_type_ids=segments)


def bert_model(dtype):
    from transformers import BertConfig, BertModel
    m = BertModel(BertConfig(**R.SMALL), add_pooling_layer=False)
    missing, unexpected = m.load_state_dict(R.make_weights(R.SMALL, SEED), strict=False)
    assert not unexpected and all("position_ids" in k or "token_type_ids" in k for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


def main():
    assert len(PIECES) == R.SMALL["vocab_size"] == len(set(PIECES))
    with open(VOCAB, "w", encoding="utf-8") as f:
        f.write("\n".join(PIECES) + "\n")
    from transformers import BertTokenizer
    tok = BertTokenizer(VOCAB, do_lower_case=False)
    from tokenizers import BertWordPieceTokenizer
    wordpiece = BertWordPieceTokenizer(VOCAB, lowercase=False)           # get_embedding takes a tokenizers.Tokenizer
    sys.path.insert(0, sys.argv[1])
    cwd = os.getcwd()
    os.chdir(sys.argv[1])
    try:
        import data_utils as ref  # noqa
    finally:
        os.chdir(cwd)
    m32, m64 = bert_model(torch.float32), bert_model(torch.float64)
    sd = R.make_weights(R.SMALL, SEED)
    out = dict(texts=np.array(TEXTS), seed=np.int64(SEED))
    dev = win = 0.0
    for n, text in enumerate(TEXTS):
        cls = ref.get_embedding_cls(text, Positional(m32), tok)
        ids = tok.convert_tokens_to_ids(tok.tokenize(ref.add_cls_sep(text.replace("<en>", "").replace("</en>", ""))))
        t = torch.tensor([ids])
        with torch.no_grad():
            h32 = m32(t, token_type_ids=torch.zeros_like(t))[0][0]
            h64 = m64(t, token_type_ids=torch.zeros_like(t))[0][0]
            mine = R.encode(sd, R.SMALL, ids, torch.float64)
        assert torch.equal(cls, h32[:1]), n
        sub = ref.get_embedding(text, None, wordpiece)
        assert sub.tolist() == ids[1:-1], n
        out[f"sub_{n}"] = sub.numpy()
        dev = max(dev, float((h32.double() - h64).abs().max()))
        win = max(win, float((h64 - mine).abs().max()))
        out[f"ids_{n}"], out[f"cls_{n}"], out[f"hidden_{n}"] = np.array(ids, dtype=np.int32), cls.numpy(), h32.numpy()
        print(n, repr(text[:40]), len(ids), "tokens, max|hidden|", float(h64.abs().max()))
    assert win < 1e-12, win
    out["dev"], out["win"] = np.float64(dev), np.float64(win)
    path = os.path.join(HERE, "bert.npz")
    np.savez_compressed(path, **out)
    print("dev", dev, "win", win, "wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
