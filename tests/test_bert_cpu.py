"""CPU tests of the BERT sentence encoder's host side: the fp64 restatement tests/bert_ref.py against the recording of
the reference's get_embedding_cls (tests/golden/bert.npz) and against transformers' BertModel, the new data_utils names
on a CPU BertModel, the pure plan, and the host validation of ids."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import bert_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bert.npz")
VOCAB = os.path.join(HERE, "golden", "bert_vocab.txt")


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def weights():
    return R.make_weights(R.SMALL, int(golden()["seed"]))


def n_cases():
    return len(golden()["texts"])


def hf_model(dtype=torch.float32):
    tr = pytest.importorskip("transformers")
    m = tr.BertModel(tr.BertConfig(**R.SMALL), add_pooling_layer=False)
    m.load_state_dict(weights(), strict=False)
    return m.to(dtype).eval()


def test_fixture_holds_the_cases_the_issue_names():
    z = golden()
    texts = [str(t) for t in z["texts"]]
    assert sum("<en>" in t for t in texts) == 2 and "" in texts
    assert os.path.getsize(GOLDEN) < 300 * 1024
    assert float(z["win"]) < 1e-12 and 0 < float(z["dev"]) < 1e-4


def test_ref_reproduces_the_recording():
    """|bert_ref fp64 - recorded fp32| <= dev + win: dev is the recorded model's own fp32 - fp64 gap, win the gap between the
    two fp64 statements."""
    z = golden()
    bound = float(z["dev"]) + float(z["win"])
    for i in range(n_cases()):
        mine = R.encode(weights(), R.SMALL, z[f"ids_{i}"].tolist())
        err = float((mine - torch.from_numpy(z[f"hidden_{i}"]).double()).abs().max())
        print(f"case {i}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound
        assert np.array_equal(z[f"cls_{i}"], z[f"hidden_{i}"][:1])
        assert z[f"ids_{i}"][0] == 2 and z[f"ids_{i}"][-1] == 3                         # [CLS] ... [SEP] of the recorded vocabulary


def test_ref_matches_a_fresh_bert_model():
    m = hf_model(torch.float64)
    ids = R.tokens([1, 2, 33, 70], seed=1, vocab=R.SMALL["vocab_size"])
    for s in ids:
        t = torch.tensor([s])
        with torch.no_grad():
            theirs = m(input_ids=t, attention_mask=torch.ones_like(t), token_type_ids=torch.zeros_like(t))[0][0]
        err = float((theirs - R.encode(weights(), R.SMALL, s)).abs().max())
        print(f"{len(s)} tokens: err {err:.3e}")
        assert err < 1e-12                                                              # two fp64 statements: rounding level, |values| ~ 4


def test_weights_are_seeded_and_named_like_the_checkpoint():
    from tacotron2_subword_amd.bert import state_dict_keys
    sd = weights()
    assert sorted(sd) == sorted(state_dict_keys(R.SMALL["num_hidden_layers"]))
    again = R.make_weights(R.SMALL, int(golden()["seed"]))
    assert all(torch.equal(sd[k], again[k]) for k in sd)


def test_get_embedding_cls_on_a_cpu_model_reproduces_the_recording():
    """The keyword call of data_utils against fp64 truth, bound 4 * max(dev, 2^-23 max|truth|) as on the GPU; the recorded
    vector must lie within the same bound."""
    tr = pytest.importorskip("transformers")
    from tacotron2_subword_amd import data_utils as D
    z = golden()
    m = hf_model()
    tok = tr.BertTokenizer(VOCAB, do_lower_case=False)
    texts = [str(t) for t in z["texts"]]
    batch = D.get_embedding_cls_batch(texts, m, tok)
    assert batch.shape == (len(texts), R.SMALL["hidden_size"])
    for i, text in enumerate(texts):
        got = D.get_embedding_cls(text, m, tok)
        assert got.shape == (1, R.SMALL["hidden_size"]) and got.dtype == torch.float32
        truth = R.encode(weights(), R.SMALL, z[f"ids_{i}"].tolist())[:1]
        bound = 4 * max(float(z["dev"]), 2.0 ** -23 * float(truth.abs().max()))
        for what, v in (("single", got), ("batch", batch[i:i + 1]), ("recorded", torch.from_numpy(z[f"cls_{i}"]))):
            err = float((v.double() - truth).abs().max())
            print(f"case {i} {what}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound


def test_get_embedding_returns_the_recorded_ids():
    tk = pytest.importorskip("tokenizers")
    from tacotron2_subword_amd import data_utils as D
    z = golden()
    wp = tk.BertWordPieceTokenizer(VOCAB, lowercase=False)
    for i, text in enumerate(str(t) for t in z["texts"]):
        got = D.get_embedding(text, None, wp)
        assert got.dtype == torch.int32 and got.tolist() == z[f"sub_{i}"].tolist() == z[f"ids_{i}"][1:-1].tolist()
    assert D.add_cls_sep("x") == "[CLS] x [SEP]"


def test_modules_import_without_transformers():
    import subprocess
    code = ("import sys; import tacotron2_subword_amd.data_utils, tacotron2_subword_amd.bert; "
            "assert 'transformers' not in sys.modules and 'tokenizers' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(HERE))


# ---------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------
def plan(cfg=None, B=4, total=200, max_len=100, cls_only=True, **over):
    from tacotron2_subword_amd import _lib as L
    return L.bert_plan(L.bert_config(dict(cfg or R.BASE, **over)), B, total, max_len, cls_only)


def test_plan_answers_without_a_device():
    p = plan()
    H, I, V = 768, 3072, 128
    per_layer = 4 * (H * H + H) + 2 * (I * H) + I + H + 4 * H
    assert p.packed_floats == (V + 512 + 2) * H + 2 * H + 12 * per_layer
    assert p.launches == 1 + 7 * 11 + 9
    assert plan(cls_only=False).launches == 1 + 7 * 12 + 1
    assert p.workspace_bytes > 0


@pytest.mark.parametrize("kwargs, message", [
    (dict(num_attention_heads=8), "head dim"),
    (dict(hidden_size=96, num_attention_heads=1), "hidden=96 must be a multiple of 64"),
    (dict(hidden_size=1088, num_attention_heads=17), "hidden=1088 must be a multiple of 64 between 64 and 1024"),
    (dict(intermediate_size=3000), "intermediate=3000 must be a multiple of 64"),
    (dict(max_len=513, B=1, total=513), "max_len=513 outside 1..min(512, max_pos=512)"),
    (dict(max_position_embeddings=300, max_len=301, B=1, total=301), "max_len=301 outside 1..min(512, max_pos=300)"),
    (dict(B=0, total=0), "B=0 outside"),
    (dict(B=2, total=1), "total_tokens=1 outside"),
])
def test_plan_refuses_by_name(kwargs, message):
    call = {k: kwargs.pop(k) for k in ("B", "total", "max_len") if k in kwargs}
    with pytest.raises(RuntimeError) as e:
        plan(**call, **kwargs)
    assert message in str(e.value), str(e.value)


def test_plan_sizes_are_monotone_and_cls_only_needs_no_more():
    last = None
    for total in (4, 5, 64, 200, 400):
        full, cls = plan(total=total, cls_only=False), plan(total=total, cls_only=True)
        assert cls.workspace_bytes <= full.workspace_bytes
        assert full.packed_floats == cls.packed_floats == plan().packed_floats
        if last:
            assert full.workspace_bytes > last[0] and cls.workspace_bytes > last[1]
        last = (full.workspace_bytes, cls.workspace_bytes)
    one = dict(R.SMALL, num_hidden_layers=1)
    assert plan(one, cls_only=True).workspace_bytes < plan(one, cls_only=False).workspace_bytes


def test_gemm_layer_knows_gelu_and_refuses_what_it_does_not_know():
    from tacotron2_subword_amd import _lib as L
    def args(act):
        return L.GemmArgs(256, 256, 256, 64, 64, 64, 64, 1, 64, 1, 64, 1, 0, 0, 0, 1.0, 0.0, None, act, 0, 0, None, 0, 0)
    assert L.gemm_plan(args(3))
    with pytest.raises(RuntimeError, match="unknown activation act=4"):
        L.gemm_plan(args(4))


# ---------------------------------------------------------------------------------------------------------------
# host validation: before any device call (there is no device here)
# ---------------------------------------------------------------------------------------------------------------
def encoder():
    from tacotron2_subword_amd.bert import BertEncoder
    return BertEncoder.from_state_dict(weights(), R.SMALL)


@pytest.mark.parametrize("ids, message", [
    ([[1, 2, 100]], "id 100, outside the vocabulary 0..99"),
    ([[1, 2], [3, -1]], "sentence 1 holds id -1"),
    ([[1] * 513], "513 tokens, the encoder takes 1..512"),
    ([[1], []], "sentence 1 has 0 tokens"),
    ([], "empty batch"),
])
def test_host_validation_rejects_before_anything_is_uploaded(ids, message):
    enc = encoder()
    for call in (enc.cls, enc.hidden):
        with pytest.raises(ValueError) as e:
            call(ids)
        assert message in str(e.value), str(e.value)
    assert enc._packed is None and enc._ws is None                                     # nothing went to a device


def test_host_validation_takes_lists_and_cpu_tensors():
    from tacotron2_subword_amd.bert import validate_ids
    ids, cu, max_len = validate_ids([[5, 6, 7], torch.tensor([1, 2], dtype=torch.int32), np.array([9])], 100, 520)
    assert ids.dtype == np.int32 and ids.tolist() == [5, 6, 7, 1, 2, 9]
    assert cu.dtype == np.int32 and cu.tolist() == [0, 3, 5, 6] and max_len == 3
    with pytest.raises(ValueError, match="takes 1..300"):
        validate_ids([[1] * 301], 100, 300)


def test_from_model_reads_a_transformers_model():
    from tacotron2_subword_amd.bert import BertEncoder
    enc = BertEncoder.from_model(hf_model())                                           # packs on first use: no device here
    c = enc.config
    assert (c.hidden, c.layers, c.heads, c.intermediate, c.vocab, c.max_pos, c.type_vocab) == (128, 2, 2, 256, 100, 520, 2)
    assert abs(c.ln_eps - 1e-12) < 1e-18 and enc.device.type == "cuda"
    want = weights()
    from tacotron2_subword_amd.bert import state_dict_keys
    assert all(torch.equal(t, want[k]) for k, t in zip(state_dict_keys(2), enc._host))


def test_state_dict_with_prefix_and_pooler_and_a_wrong_shape():
    from tacotron2_subword_amd.bert import BertEncoder
    sd = {"bert." + k: v for k, v in weights().items()}
    sd["bert.pooler.dense.weight"] = torch.zeros(128, 128)
    sd["cls.predictions.bias"] = torch.zeros(100)
    enc = BertEncoder.from_state_dict(sd, R.SMALL)
    assert enc.config.hidden == 128 and enc.config.layers == 2 and len(enc._host) == 5 + 16 * 2
    with pytest.raises(ValueError, match="intermediate.dense.weight"):
        BertEncoder.from_state_dict(weights(), dict(R.SMALL, intermediate_size=512))
    with pytest.raises(RuntimeError, match="head dim"):
        BertEncoder.from_state_dict(weights(), dict(R.SMALL, num_attention_heads=4))
