"""CPU-only: the plans of the persistent chains (csrc/chain_plan.hip) through t2_chain_plan, which launches nothing, asks no
device and takes no claim.

tests/golden/chain_plans.jsonl holds, for about 1 100 shapes, what the commit BEFORE chain_plan.hip existed decided (its first
line says how it was recorded): covered or refused, and for a covered shape the kernel instance, tiling, LDS residency, grid,
dynamic LDS, query-partial bytes, the offset and size of every exchange part, what is cleared, and the least exchange space.
Every row must come out the same, exactly.  The rows marked parent = error are the one intended difference: the parent's plan
accepted a tiling its executor had no kernel instance for and the pass failed; the plan now refuses them (no_instance) and the
pass takes the per-step launches.  What the carve promises in comments is asserted from the plan alone."""
import itertools
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "chain_plans.jsonl")
DEFAULTS = dict(dec=0, NS=2, H=1024, E=512, A=128, P=256, M=80, Hd=1024, F=32, Kc=31, Tin=[100, 60], cus=256, claimed=1, no_resident=0, saved=1,
                backward=0)
KINDS = ("lstm", "sma", "lsa", "enc")
REASONS = ("covered", "shape", "no_instance", "device", "claim", "query_part", "lds", "lsa_resident", "short_memory", "lsa_split", "no_saved_tiles",
           "workspace")                                                     # T2_CHAIN_OK, T2_CHAIN_REFUSE_* (include/t2amd.h)
INSTANCES = ("fwd_lstm_11", "fwd_lstm_12", "fwd_sma_11", "fwd_sma_21", "fwd_sma_22", "fwd_lsa_11", "fwd_lsa_21", "fwd_lsa_22", "fwd_sma_dec",
             "fwd_lsa_dec", "bwd_lstm_1", "bwd_lstm_2", "bwd_sma_1", "bwd_sma_2", "bwd_lsa_1", "bwd_lsa_2", "enc_fwd", "enc_bwd")
LDS_LIMIT = 160 * 1024


def load_rows():
    with open(FIXTURE) as f:
        head, *rows = [json.loads(line) for line in f]
    assert "comment" in head and "exp" not in head
    return [dict(DEFAULTS, **r) for r in rows]


def plan(L, r, **over):
    """The library's plan for a fixture row (over: fields to replace), as _lib.chain_plan returns it."""
    r = dict(r, **over)
    backward = r["dir"] == "bwd" or bool(r["backward"])
    shape = {k: r[k] for k in ("dec", "NS", "B", "H", "E", "A", "P", "M", "Hd", "F", "Kc", "Tin")}
    return L.chain_plan(KINDS[r["kind"]], backward, cus=r["cus"], claimed=r["claimed"], no_resident=r["no_resident"], saved_tiles=r["saved"],
                        ws_floats=r["ws_floats"], **shape)


def as_recorded(r, p):
    """The plan in the fixture's form: the fields the parent commit's code had a value for."""
    if not p["covered"]:
        return dict(covered=0, reason=REASONS[p["reason"]])
    e = dict(covered=1, instance=p["instance_name"], grid=p["grid"], lds_bytes=p["lds_bytes"], parts={k: list(v) for k, v in p["parts"].items()},
             total=p["total_bytes"])
    if r["dir"] == "fwd":
        e.update({k: p[k] for k in ("UT", "RT", "CS", "lds_Tin", "lds_Jp", "lds_Jm", "Jp", "Jm", "q_bytes")}, pass_clear=p["pass_clear_bytes"])
    if r["dir"] == "bwd":
        e.update(MT=p["MT"], lds_Tc=p["lds_Tc"], pb_bytes=p["parts"]["PB"][1], pbc_bytes=p["parts"].get("PBC", (0, 0))[1])
    if p["clear"][1]:
        e["clear"] = list(p["clear"])
    return e


def expected(r):
    e = dict(r["exp"])
    if e.pop("parent", None):                                              # the parent's executor failed: now a refusal with a reason of its own
        assert e == dict(covered=0, reason="no_instance")
    return e


def test_fixture_covers_the_plans():
    rows = load_rows()
    assert 1000 <= len(rows) <= 3000 and os.path.getsize(FIXTURE) < 1000000
    assert {r["exp"].get("instance") for r in rows if r["exp"]["covered"]} == set(INSTANCES)
    assert {r["exp"]["reason"] for r in rows if not r["exp"]["covered"]} == set(REASONS[1:])
    errors = [r for r in rows if "parent" in r["exp"]]
    assert errors and all(r["dir"] == "fwd" and r["kind"] in (1, 2) and r["NS"] == 1 and not r["dec"] and 97 <= r["B"] <= 128 for r in errors)

    def seen(direction, key, values, **where):
        have = {json.dumps(r[key]) for r in rows if r["dir"] == direction and all(r[k] == v for k, v in where.items())}
        return all(json.dumps(v) in have for v in values)

    # both sides of every threshold in the plans
    assert seen("fwd", "B", (32, 33, 64, 65, 96, 97, 128, 129)) and seen("bwd", "B", (32, 33, 64, 65))
    for d in ("fwd", "bwd"):
        assert seen(d, "NS", (1, 2)) and seen(d, "cus", (255, 256, 304)) and seen(d, "claimed", (0, 1))
    assert seen("fwd", "M", (80, 88, 96), dec=1) and seen("fwd", "dec", (0, 1)) and seen("fwd", "no_resident", (0, 1))
    assert seen("bwd", "Tin", ([15, 15], [16, 16], [128, 128], [129, 100])) and seen("bwd", "saved", (0, 1), kind=2)
    assert seen("bwd", "Kc", (3, 31, 33, 32), kind=2) and seen("bwd", "F", (32, 16, 48, 64), kind=2)
    assert seen("fwd", "F", (32, 16, 48, 64), kind=2)
    lsa = [r for r in rows if r["dir"] == "fwd" and r["kind"] == 2]
    assert any(r["exp"]["covered"] for r in lsa) and any(r["exp"].get("reason") == "lsa_resident" for r in lsa)
    sma = [r["exp"] for r in rows if r["dir"] == "fwd" and r["kind"] == 1 and r["exp"]["covered"]]
    assert any(e["lds_Jp"] == e["lds_Tin"] == e["lds_Jm"] for e in sma) and any(e["lds_Jp"] < e["lds_Tin"] for e in sma)
    assert seen("enc", "backward", (0, 1)) and seen("enc", "B", (128, 129)) and seen("enc", "cus", (255, 256, 304))


def parts_of(p):
    return sorted((off, off + n, name) for name, (off, n) in p["parts"].items())


def check_invariants(r, p):
    if not p["covered"]:
        return
    assert p["grid"] <= r["cus"] and p["lds_bytes"] <= LDS_LIMIT and INSTANCES[p["instance"]] == p["instance_name"]
    parts = parts_of(p)
    assert all(a % 16 == 0 and b % 16 == 0 for a, b, _ in parts)
    assert all(x[1] <= y[0] for x, y in zip(parts, parts[1:])), parts                     # pairwise disjoint
    assert parts[-1][1] <= p["ws_bytes"] and p["total_bytes"] <= p["ws_bytes"] and sum(b - a for a, b, _ in parts) <= p["total_bytes"]
    clear = (p["clear"][0], p["clear"][0] + p["clear"][1])
    if r["dir"] == "fwd":
        if r["kind"] != 0:
            assert 0 < p["q_bytes"] <= p["parts"]["Q"][1]
            for s in range(r["NS"]):
                assert p["Jp"][s] <= r["Tin"][s] and p["Jm"][s] <= r["Tin"][s] and p["Jm"][s] % 2 == 0
            assert p["lds_Jm"] % 2 == 0 and p["lds_Jp"] <= p["lds_Tin"] == max(r["Tin"][:r["NS"]] + [4])
            if r["kind"] == 2:
                assert p["lds_Jp"] == p["lds_Tin"] and p["Jp"][:r["NS"]] == r["Tin"][:r["NS"]]
        status, teacher, decode = p["pass_clear_bytes"]
        assert status == p["parts"]["status"][1] == 256 and decode == p["ws_bytes"]
        tagged = [x for x in parts if x[2] in ("status", "Q", "X", "XD")]
        assert all(b <= teacher for _, b, _ in tagged)                                  # the teacher clear covers every tagged buffer ...
        assert teacher == p["ws_bytes"] - 16 * 1024 - 16 * 16 * 32 * 4                  # ... and neither the mel fragments nor a counter
        if r["dec"]:
            assert teacher <= p["parts"]["XM"][0] < p["parts"]["cnt"][0] and clear == tuple(x for x in parts if x[2] == "cnt")[0][:2]
    elif r["dir"] == "bwd":
        tagged = [x for x in parts if x[2] != "WDT"]
        assert clear[0] == min(a for a, _, _ in tagged) and clear[1] == max(b for _, b, _ in tagged)
        assert all(b <= clear[0] or a >= clear[1] for a, b, n in parts if n == "WDT")
    else:
        assert clear == (0, p["parts"]["X"][0])                                           # status words and counters


def test_every_recorded_shape_takes_the_recorded_plan():
    from tacotron2_subword_amd import _lib as L
    rows = load_rows()
    plans = [plan(L, r) for r in rows]
    wrong = [(r, as_recorded(r, p)) for r, p in zip(rows, plans) if as_recorded(r, p) != expected(r)]
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ, first: {wrong[0]}"
    for r, p in zip(rows, plans):
        check_invariants(r, p)


def test_the_chains_of_a_pass_share_its_exchange_space():
    """The attention chain's parts (from the front) and the decoder-LSTM chain's (from the back) are disjoint in a space of exactly
    chain_fwd_ws_floats / chain_bwd_ws_floats floats, and that is what the layout queries reserve."""
    from tacotron2_subword_amd import _lib as L
    from oracle import tacotron2_oracle as O
    hp = O.default_hparams()
    seen = 0
    for att, backward, NS, B in itertools.product(("sma", "lsa"), (False, True), (1, 2), (1, 32, 33, 64, 65, 96, 128)):
        dims = L.dims_from_hparams(dict(hp, attention=dict(sma="StepwiseMonotonicAttention", lsa="LocationSensitiveAttention")[att]), n_streams=NS)
        T, Tin, Tsub = 8, 60, 40
        lay = (L.decoder_bwd_layout if backward else L.decoder_layout)(dims, B, T, Tin, Tsub)
        space = lay.chain_floats * 4                                                     # = chain_fwd_ws_floats / chain_bwd_ws_floats of the pass
        pa = L.chain_plan(att, backward, NS=NS, B=B, Tin=(Tin, Tsub), ws_floats=lay.chain_floats)
        pb = L.chain_plan("lstm", backward, NS=1, B=B, ws_floats=lay.chain_floats)
        if not (pa["covered"] and pb["covered"]):                                        # (backward: B > 64; forward: one stream above 64 rows)
            assert B > 64
            continue
        assert pa["ws_bytes"] == pb["ws_bytes"] == space
        # forward: the attention chain's shape carries the whole pass, its total is the pass's; backward: the two chains' sum
        assert (pa["total_bytes"] + pb["total_bytes"] if backward else pa["total_bytes"]) == space and pb["total_bytes"] <= space
        both = sorted(parts_of(pa) + [x for x in parts_of(pb) if x[2] != "status"])
        assert all(x[1] <= y[0] for x, y in zip(both, both[1:])), both
        assert both[-1][1] <= space
        seen += 1
    assert seen == 38


def test_a_space_too_small_is_an_error_not_a_plan():
    import pytest
    from tacotron2_subword_amd import _lib as L
    full = L.chain_plan("sma", B=8)
    with pytest.raises(RuntimeError, match="exchange space too small"):
        L.chain_plan("sma", B=8, ws_floats=full["total_bytes"] // 4 - 1)
    need = L.lib().t2_lstm_seq_chain_ws_floats(2, 8, 256, 0)
    assert L.chain_plan("enc", NS=2, B=8, H=256, ws_floats=need)["covered"]
    assert L.chain_plan("enc", NS=2, B=8, H=256, ws_floats=need - 1)["reason_text"] == "the exchange space is too small"
