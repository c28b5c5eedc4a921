"""CPU-only: the host-side plans of WaveGlow (csrc/waveglow_plan.hip) through the pure-host entry points, which launch nothing,
ask no device and allocate nothing: t2_waveglow_plan, _forward_plan, _backward_plan, _grad_offsets, _packed_floats,
_weight_grad_ws_floats and _conv_backward_packed_floats.

tests/golden/waveglow_plans.jsonl holds what the commit BEFORE waveglow_plan.hip existed answered (its first line says how it
was recorded): per configuration the gradient offsets and the packed sizes, per (configuration, B, T, n_samples) every field
of the three plans (the values, in the order of the info structs' fields) and the weight-gradient scratch of the three launch
shapes, and the full text of every refusal.  Every row must come out the same, exactly.  What the tensor table and the carves
promise is asserted from the plan alone."""
import importlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "waveglow_plans.jsonl")
FULL = dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2, WN_config=dict(n_layers=8, n_channels=256, kernel_size=3))
SMALL = dict(n_mel_channels=8, n_flows=2, n_group=8, n_early_every=1, n_early_size=2, WN_config=dict(n_layers=2, n_channels=8, kernel_size=3))
UP_K, UP_STRIDE = 1024, 256


def wn(**k):
    return dict(FULL["WN_config"], **k)


def recorded_models():
    z = np.load(os.path.join(ROOT, "tests", "golden", "waveglow.npz"))
    return json.loads(str(z["configs"]))


def configurations():
    small = recorded_models()
    return {"full": FULL, "a": small["a"], "deep": small["deep"], "one_layer_512": dict(FULL, WN_config=wn(n_layers=1, n_channels=512)),
            "group2": dict(FULL, n_group=2, n_early_size=0, n_mel_channels=4), "group4_every6": dict(FULL, n_group=4, n_early_every=6),
            "channels8": dict(FULL, WN_config=wn(n_channels=8))}


WIDE = ("full", "one_layer_512", "channels8")      # the channel counts: where the weight gradient's split depends on the configuration


def shapes(G, wide=True):
    """(B, T, n_samples): a pair on either side of every rule that changes its answer; wide: those of the weight gradient's split too."""
    out = [(1, 4, G), (1, 4, 4 * UP_STRIDE), (1, 4, 3 * UP_STRIDE + UP_K), (1, 4, 4 * UP_STRIDE + G + 1)]      # n_samples at its ends, and no multiple of G
    out += [(B, 1, G * L) for B in (1, 3) for L in (4, 5)]                       # round4(B * L)
    out += [(B, 8, G * L) for B in (1, 3) for L in (32, 33, 256, 257)]           # chunks of the weight gradient; n_blocks, n_partials, n_slots
    if not wide:
        return out + [(B, 1, 256) for B in (1, 3, 12, 65535)]
    out += [(1, 64, G * L) for L in (2048, 2049)]                                # B * ceil(L / 32) across 64, the maximum split
    out += [(3, 24, G * L) for L in (672, 673, 704, 705)] + [(12, 8, G * L) for L in (160, 161)]
    out += [(1, 24, G * L) for L in (640, 641, 672, 673)]                        # 256 channels: across 1024 / tiles = 21 (conv) chunks
    out += [(B, 1, 256) for B in (1, 3, 12, 65535)]
    return out + [(12, 63, 16000)]                                               # the training shape of waveglow/config.json


def fields(info):
    """The values of a plan's info struct in the order of its fields (the fixture stores them so, without the names)."""
    return [getattr(info, n) for n, _ in info._fields_]


def field(L, struct, values, name):
    return values[[n for n, _ in getattr(L, struct)._fields_].index(name)]


def flow_channels(cfg):
    ch, out = cfg["n_group"], []
    for k in range(cfg["n_flows"]):
        if k % cfg["n_early_every"] == 0 and k > 0:
            ch -= cfg["n_early_size"]
        out.append(ch)
    return out


def config_row(L, cfg):
    c = L.waveglow_config(**cfg)
    nc, n_mel, n_cond = cfg["WN_config"]["n_channels"], cfg["n_mel_channels"], cfg["n_mel_channels"] * cfg["n_group"]
    n = L.waveglow_plan(c, 1, 1).n_tensors
    pf = L.lib().t2_waveglow_packed_floats
    return dict(offsets=L.waveglow_grad_offsets(c, n),
                packed=[pf(L.WAVEGLOW_GATED, nc, nc, n_cond), pf(L.WAVEGLOW_RES_SKIP, 2 * nc, nc, 0), pf(L.WAVEGLOW_RES_SKIP, nc, nc, 0),
                        pf(L.WAVEGLOW_UPSAMPLE, n_mel, n_mel, 0)],
                conv_bwd_packed=L.lib().t2_waveglow_conv_backward_packed_floats(nc, n_cond))


def shape_row(L, cfg, B, T, N):
    c = L.waveglow_config(**cfg)
    nc, n_cond = cfg["WN_config"]["n_channels"], cfg["n_mel_channels"] * cfg["n_group"]
    fwd = L.waveglow_forward_plan(c, B, T, N)
    ws = L.lib().t2_waveglow_weight_grad_ws_floats
    halves = sorted({ch // 2 for ch in flow_channels(cfg)})
    return dict(infer=fields(L.waveglow_plan(c, B, T)), forward=fields(fwd), backward=fields(L.waveglow_backward_plan(c, B, T, N)),
                wgrad_ws=[ws(2 * nc, nc, n_cond, 3, B, fwd.L), ws(nc, nc, 0, 1, B, fwd.L)] + [ws(nc, h, 0, 1, B, fwd.L) for h in halves])


def refusal_rows():
    """(entry, cfg, arguments, needles) of every refusal the three CPU test modules of WaveGlow assert"""
    rows = []
    for module, entry in (("test_waveglow_cpu", "plan"), ("test_waveglow_forward_cpu", "forward_plan")):
        mark = [m for m in importlib.import_module(module).test_plan_refuses_with_the_value.pytestmark if m.name == "parametrize"][0]
        for change, *args, needles in mark.args[1]:
            rows.append((entry, dict(FULL, **change), args, [needles] if isinstance(needles, str) else needles))
    for args, needle in (((0, 2, 512), "B=0"), ((1, 0, 512), "T=0"), ((1, 2, 7), "n_samples=7"), ((1, 2, 1281), "n_samples=1281")):      # test_waveglow_backward_cpu
        rows += [(entry, SMALL, list(args), [needle]) for entry in ("backward_plan", "forward_plan")]
    rows.append(("backward_plan", dict(SMALL, WN_config=dict(n_layers=9, n_channels=8, kernel_size=3)), [1, 2, 512], ["n_layers=9"]))
    rows.append(("grad_offsets", SMALL, [3], ["3 tensors"]))
    return rows


def refusal_text(L, entry, cfg, args):
    with pytest.raises(RuntimeError) as e:
        getattr(L, "waveglow_" + entry)(L.waveglow_config(**cfg), *args)
    return str(e.value)


def load_fixture():
    with open(FIXTURE) as f:
        head, *rows = [json.loads(line) for line in f]
    assert "comment" in head and "exp" not in head
    return rows


def test_fixture_covers_the_rules():
    rows = load_fixture()
    assert os.path.getsize(FIXTURE) < 200000
    cfgs = configurations()
    assert FULL["WN_config"] == dict(n_layers=8, n_channels=256, kernel_size=3) and len(recorded_models()) == 2
    have_cfg = {r["name"]: r["cfg"] for r in rows if r["kind"] == "config"}
    assert have_cfg == cfgs
    have = {(r["name"], r["B"], r["T"], r["N"]) for r in rows if r["kind"] == "shape"}
    for name, cfg in cfgs.items():
        G = cfg["n_group"]
        assert all((name, *s) in have for s in shapes(G, name in WIDE)), name
        mine = [s for n, *s in have if n == name]
        cols = {(B, N // G) for B, T, N in mine}
        assert {B for B, _ in cols} >= {1, 3, 12, 65535} and any(N % G for _, _, N in mine)
        assert any(B * L % 4 == 0 for B, L in cols) and any(B * L % 4 for B, L in cols)
        assert all((B, L) in cols for B in (1, 3) for L in (32, 33, 256, 257))
        assert any(N == G for _, _, N in mine) and any(N == T * UP_STRIDE for _, T, N in mine) and any(N == (T - 1) * UP_STRIDE + UP_K for _, T, N in mine)
        chunks = sorted(B * -(-L // 32) for B, L in cols)
        assert name not in WIDE or (any(a <= 64 < b for a, b in zip(chunks, chunks[1:])) and {20, 21, 22} <= set(chunks))
    # the split is seen to change where it should: more partial planes on the far side of each pair
    from tacotron2_subword_amd import _lib as L
    exp = {(r["name"], r["B"], r["N"] // cfgs[r["name"]]["n_group"]): r["exp"] for r in rows if r["kind"] == "shape"}
    # (21 chunks in 21 runs, 22 chunks in 11 runs of two; 64 chunks in 64 runs, 65 in 33)
    assert exp[("full", 1, 641)]["wgrad_ws"][0] * 20 == exp[("full", 1, 640)]["wgrad_ws"][0] * 21 and exp[("full", 1, 673)]["wgrad_ws"][0] * 21 == exp[("full", 1, 672)]["wgrad_ws"][0] * 11
    assert exp[("channels8", 1, 2049)]["wgrad_ws"][0] * 64 == exp[("channels8", 1, 2048)]["wgrad_ws"][0] * 33 and exp[("channels8", 1, 33)]["wgrad_ws"][0] == 2 * exp[("channels8", 1, 32)]["wgrad_ws"][0]
    assert field(L, "WaveglowForwardInfo", exp[("full", 1, 257)]["forward"], "n_blocks") == 2 == 2 * field(L, "WaveglowForwardInfo", exp[("full", 1, 256)]["forward"], "n_blocks")
    assert field(L, "WaveglowBackwardInfo", exp[("full", 3, 257)]["backward"], "n_slots") == 24 == 2 * field(L, "WaveglowBackwardInfo", exp[("full", 3, 256)]["backward"], "n_slots")
    recorded = {(r["entry"], json.dumps(r["cfg"], sort_keys=True), json.dumps(r["args"])) for r in rows if r["kind"] == "refusal"}
    assert recorded == {(e, json.dumps(c, sort_keys=True), json.dumps(a)) for e, c, a, _ in refusal_rows()}


def test_every_recorded_answer_comes_out_the_same():
    from tacotron2_subword_amd import _lib as L
    rows, cfgs = load_fixture(), configurations()
    wrong = []
    for r in rows:
        if r["kind"] == "config":
            got = config_row(L, r["cfg"])
        elif r["kind"] == "shape":
            got = shape_row(L, cfgs[r["name"]], r["B"], r["T"], r["N"])
        else:
            got = refusal_text(L, r["entry"], r["cfg"], r["args"])
        if got != r["exp"]:
            wrong.append((r, got))
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ, first: {wrong[0]}"


def test_refusals_keep_their_text():
    from tacotron2_subword_amd import _lib as L
    recorded = {(r["entry"], json.dumps(r["cfg"], sort_keys=True), json.dumps(r["args"])): r["exp"] for r in load_fixture() if r["kind"] == "refusal"}
    for entry, cfg, args, needles in refusal_rows():
        text = refusal_text(L, entry, cfg, args)
        assert text == recorded[(entry, json.dumps(cfg, sort_keys=True), json.dumps(args))] and all(n in text for n in needles), text


def tensor_table(cfg):
    """(name, torch-layout element count) of every folded tensor in t2_waveglow_pack's order, restated from glow.py"""
    nc, nl, n_mel = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"], cfg["n_mel_channels"]
    n_cond = n_mel * cfg["n_group"]
    t = [("up_w", n_mel * n_mel * UP_K), ("up_b", n_mel)]
    for k, c in enumerate(flow_channels(cfg)):
        t += [(f"{k}.start_w", nc * (c // 2)), (f"{k}.start_b", nc), (f"{k}.cond_w", 2 * nc * nl * n_cond), (f"{k}.cond_b", 2 * nc * nl)]
        for i in range(nl):
            t += [(f"{k}.in_w{i}", 2 * nc * nc * 3), (f"{k}.in_b{i}", 2 * nc)]
        for i in range(nl):
            rows = 2 * nc if i < nl - 1 else nc
            t += [(f"{k}.rs_w{i}", rows * nc), (f"{k}.rs_b{i}", rows)]
        t += [(f"{k}.end_w", c * nc), (f"{k}.end_b", c), (f"{k}.mix", c * c)]
    return t


def test_what_the_plans_promise():
    from tacotron2_subword_amd import _lib as L
    for name, cfg in configurations().items():
        c = L.waveglow_config(**cfg)
        G, nc, n_cond = cfg["n_group"], cfg["WN_config"]["n_channels"], cfg["n_mel_channels"] * cfg["n_group"]
        table = tensor_table(cfg)
        for B, T, N in shapes(G, name in WIDE):
            inf, fwd, bwd = L.waveglow_plan(c, B, T), L.waveglow_forward_plan(c, B, T, N), L.waveglow_backward_plan(c, B, T, N)
            assert inf.n_tensors == fwd.n_tensors == bwd.n_tensors == len(table), name
            assert bwd.grad_floats == sum(n for _, n in table), name
            assert inf.packed_bytes == fwd.packed_bytes and fwd.L == bwd.L == N // G and inf.L * G == inf.out_len == T * UP_STRIDE // G * G
            assert fwd.n_blocks == -(-fwd.L // 256) and fwd.n_partials == 2 * cfg["n_flows"] * B * fwd.n_blocks and bwd.n_slots == 4 * B * fwd.n_blocks
            per = (B * fwd.L + 3) // 4 * 4
            assert fwd.workspace_bytes - 8 * (fwd.n_partials + B * (cfg["n_flows"] + 2)) == 4 * per * (n_cond + 3 * nc + 2 * G)      # the doubles end the carve
            assert all(b % 16 == 0 for b in (inf.workspace_bytes, fwd.workspace_bytes - 8 * (fwd.n_partials + B * (cfg["n_flows"] + 2)), bwd.saved_bytes))
            assert bwd.saved_bytes == 4 * per * (n_cond + sum(ch + nc * (1 + 3 * cfg["WN_config"]["n_layers"]) for ch in flow_channels(cfg)))
        offs = L.waveglow_grad_offsets(c, len(table))
        assert offs[0] == 0 and all(b - a == n for a, b, (_, n) in zip(offs, offs[1:] + [bwd.grad_floats], table)), name      # ascending, dense, ends at grad_floats
