"""CPU-only: the plans of the three decoder passes (csrc/decoder_plan.hip) through t2_decoder_pass_plan, which launches nothing,
asks no device and takes no claim.

tests/golden/decoder_pass_plans.jsonl holds, for 192 passes (one per decision class and a pair per switch and threshold, of 1 214 recorded), what the decoder drivers of the commit BEFORE
decoder_plan.hip existed decided (its first line says how it was recorded): the recurrent steps, the chains with their refusal
reasons and kernel instances, overlap and the step-range bounds, every condition of the GEMM-scratch carves with the offsets
the products were then given, where the decoder-LSTM weight gradients went, the tail's stream, and the total_floats of both
layouts.  Every row must come out the same, exactly.  What the rules promise is asserted from the plan alone."""
import json
import os

from helpers import DCA, FA2, GMM, LSA, SMA, hp_for, tiny_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "decoder_pass_plans.jsonl")
DEFAULTS = dict(dims="default", att="sma", NS=2, B=8, T=12, Tin=40, Tsub=20, precision="bf16", split_steps=0, chain=1, chain_bwd=1, overlap=1,
                cus=256, claimed=1, no_resident=0, saved=1, defer=0, poll=0)
ATT = dict(sma=SMA, lsa=LSA, fwd2=FA2, gmm=GMM, dca=DCA)
CLEAR = ("status", "teacher", "decode")


def load_rows():
    with open(FIXTURE) as f:
        head, *rows = [json.loads(line) for line in f]
    assert "comment" in head and "exp" not in head
    return [dict(DEFAULTS, **r) for r in rows]


def plan(L, r, **over):
    """The library's plan for a fixture row (over: fields to replace), as _lib.decoder_pass_plan returns it."""
    r = dict(r, **over)
    dims = L.dims_from_hparams((tiny_hp if r["dims"] == "tiny" else hp_for)(ATT[r["att"]]), n_streams=r["NS"])
    env = {k: r[k] for k in ("precision", "split_steps", "chain", "chain_bwd", "overlap", "cus", "claimed", "no_resident")}
    return L.decoder_pass_plan(dims, r["pass"], r["B"], r["T"], r["Tin"], r["Tsub"], defer_weight_grads=r["defer"], poll_every=r["poll"],
                               saved_tiles=r["saved"], **env)


def chain_as_recorded(c, exp_reason):
    """(on, refusal, instance) of a chain as the parent had them.  The parent planned a chain only behind its own early returns
    (switch, step mode, attention kind, and for the LSA backward the saved tiles) and had no reason otherwise (0); the plan now
    states the one reason the parent had no word for, the missing tiles."""
    from tacotron2_subword_amd._lib import CHAIN_REFUSE_NO_SAVED_TILES
    reason = c["reason"] if c["asked"] else 0
    if not c["on"] and exp_reason == 0 and reason == CHAIN_REFUSE_NO_SAVED_TILES:
        reason = 0
    return int(c["on"]), reason, c.get("instance", -1)


def as_recorded(r, p, exp):
    """The plan in the fixture's form: the variables the parent commit's drivers had."""
    a = chain_as_recorded(p["chain_a"], exp["ra"])
    e = dict(use16=int(p["use16"]), chain_a=a[0], ra=a[1], ia=a[2], total_floats=p["layout"].total_floats)
    if r["pass"] == "infer":
        e.update(poll=p["poll"], clear=CLEAR.index(p["clear"]), poison=p["poison_words"], shadow_floats=p["shadow_floats"])
        return e
    b = chain_as_recorded(p["chain_b"], exp["rb"])
    e.update(split=int(p["split"]), pre16=int(p["pre16"]), chain_b=b[0], rb=b[1], ib=b[2], overlap=int(p["overlap"]), bounds=p["bounds"])
    if r["pass"] == "forward":
        e.update(w16_bytes=p["scratch"]["w_ih16"][1], gemm_ws_floats=p["layout"].gemm_ws_floats, chained=int(p["chained"]), saves=int(p["saves_tiles"]),
                 clear=CLEAR.index(p["clear"]), pred_ws=list(p["scratch"]["rest"]), poison=p["poison_words"])
        return e
    s, t = p["scratch"], p["tail_scratch"]
    e.update(defer=int(p["defer"]), bwd_total_floats=p["bwd_layout"].total_floats, gemm_ws_floats=p["bwd_layout"].gemm_ws_floats, nsplit=p["nsplit"],
             dg16_off=s["dg16"][0], share=int(p["share"]), chunk_cast=int(p["chunk_cast"]), ddin_ws=list(p["ddin_ws"]), wg=p["dec_wgrads"],
             wg_staged=int(p["dec_wgrads_staged"]), tail_on_side=int(p["tail_on_side"]), tail_share=int(p["tail_share"]), lsa_chain=int(p["lsa_chain"]),
             nsp=p["dq_parts"])
    if p["share"]:
        e["dg"] = [s["dg16"][0], s["rest"][0], s["rest"][1]]
    if p["tail_share"]:
        e["tail_dg"] = [t["dg16"][0], t["rest"][0], t["rest"][1]]
    return e


def test_fixture_covers_the_rules():
    rows = load_rows()
    assert os.path.getsize(FIXTURE) < 1000000

    def seen(key, values, **where):
        have = {json.dumps(r[key]) for r in rows if all(r[k] == v for k, v in where.items())}
        return all(json.dumps(v) in have for v in values)

    def both(key, **where):                                                 # a decision seen taken and not taken
        return {r["exp"][key] for r in rows if key in r["exp"] and all(r[k] == v for k, v in where.items())} >= {0, 1}

    def flips(key, decision, values=None, **where):
        """two rows that differ in the input `key` alone (taking `values`, if given) and in the recorded `decision`: the input decides"""
        group = {}
        for r in rows:
            if decision in r["exp"] and all(r[k] == v for k, v in where.items()) and (values is None or r[key] in values):
                rest = json.dumps({k: v for k, v in r.items() if k not in (key, "exp")}, sort_keys=True)
                group.setdefault(rest, set()).add(json.dumps([r[key], r["exp"][decision]]))
        return any(len({json.loads(x)[0] for x in g}) > 1 and len({json.dumps(json.loads(x)[1]) for x in g}) > 1 for g in group.values())

    # every switch, device answer and threshold where it decides: a pair of rows apart in that input alone, with another decision
    back, fwd, inf = {"pass": "backward"}, {"pass": "forward"}, {"pass": "infer"}
    for where in (back, fwd, inf):
        assert flips("chain", "chain_a", **where) and flips("cus", "chain_a", (255, 256), **where) and flips("claimed", "chain_a", **where)
        assert flips("B", "use16", (128, 129), **where) and flips("precision", "use16", **where) and flips("dims", "use16", **where)
    for where in (back, fwd):
        assert flips("overlap", "overlap", **where) and flips("T", "overlap", (31, 32), **where) and flips("split_steps", "split", **where)
        assert flips("chain", "chain_b", **where) and flips("chain", "overlap", **where)
    assert flips("chain_bwd", "chain_a", att="sma", **back) and flips("chain_bwd", "chain_a", att="lsa", **back) and flips("chain_bwd", "chain_b", **back)
    assert flips("saved", "chain_a", att="lsa", NS=1, **back) and flips("saved", "chain_a", att="lsa", NS=2, **back) and flips("saved", "lsa_chain", **back)
    assert not flips("saved", "chain_a", att="sma", **back)
    assert flips("overlap", "defer", defer=1, **back) and flips("overlap", "tail_on_side", defer=1, **back) and flips("defer", "defer", **back)
    assert flips("T", "defer", (31, 32), defer=1, **back) and flips("defer", "wg", **back) and flips("chain", "wg", defer=1, **back)
    assert flips("Tsub", "nsplit", (15, 16), NS=2, **back) and flips("Tin", "nsplit", (15, 16), NS=2, **back) and flips("Tsub", "chain_a", (15, 16), NS=2, **back)
    assert flips("T", "share", (32, 34), B=8, **back) and flips("T", "chunk_cast", (32, 34), B=8, **back) and flips("T", "tail_share", (1, 2), **back)
    assert flips("T", "share", (425, 426), B=128, **back) and flips("T", "tail_share", (384, 385), B=128, **back)
    assert flips("poll", "poll", **inf) and flips("chain", "poll", **inf) and flips("NS", "chain_a", **inf) and flips("chain", "clear", **inf)
    assert flips("att", "chain_a", ("sma", "gmm"), **fwd) and flips("att", "saves", ("sma", "lsa"), **fwd) and flips("chain", "poison", **fwd)
    assert any(r["exp"]["ra"] == 0 and not r["exp"]["chain_a"] and r["att"] == "lsa" and not r["saved"] and r["chain"] and r["chain_bwd"] and r["precision"] == "bf16"
               and r["dims"] == "default" and r["B"] <= 64 for r in rows if r["pass"] == "backward")      # the parent's early return: the plan's no_saved_tiles

    for kind in ("forward", "backward", "infer"):
        assert seen("B", (128, 129), **{"pass": kind}) and seen("precision", ("f32", "bf16", "bf16x3"), **{"pass": kind})
        assert seen("split_steps", (0, 1), precision="bf16x3", **{"pass": kind}) and seen("dims", ("default", "tiny"), **{"pass": kind})
        assert seen("att", tuple(ATT), **{"pass": kind}) and seen("NS", (1, 2), **{"pass": kind}) and both("use16", **{"pass": kind})
        assert seen("chain", (0, 1), **{"pass": kind}) and both("chain_a", **{"pass": kind})
        assert seen("cus", (255, 256, 304), **{"pass": kind}) and seen("claimed", (0, 1), **{"pass": kind})
    for kind in ("forward", "backward"):
        assert seen("T", (1, 2, 31, 32), **{"pass": kind}) and both("overlap", **{"pass": kind}) and both("split", **{"pass": kind})
        assert both("chain_b", **{"pass": kind}) and both("pre16", **{"pass": kind})
        assert seen("B", (97,), NS=1, **{"pass": kind})
    assert any(r["exp"]["ra"] == 2 and not r["exp"]["chain_b"] and r["exp"]["rb"] == 0 for r in rows if r["pass"] == "forward")     # no instance: chain B not asked
    assert seen("chain_bwd", (0, 1)) and seen("overlap", (0, 1)) and seen("defer", (0, 1), **{"pass": "backward"})
    assert any(not (r["chain"] or r["chain_bwd"] or r["overlap"]) for r in rows)
    back = [r for r in rows if r["pass"] == "backward"]
    for key in ("share", "chunk_cast", "tail_share", "defer", "lsa_chain", "tail_on_side", "wg_staged"):
        assert both(key, **{"pass": "backward"}), key
    assert {r["exp"]["wg"] for r in back} == {"chain_b", "tail"} and {r["exp"]["nsp"] for r in back} == {1, 2} == {r["exp"]["nsplit"] for r in back}
    assert seen("T", (32, 34), B=8, chain=0, **{"pass": "backward"})                  # B*T % 64 and range rows % 64
    assert seen("Tin", (15, 16), **{"pass": "backward"}) and seen("Tsub", (15, 16), **{"pass": "backward"})
    assert seen("saved", (0, 1), att="lsa", **{"pass": "backward"})
    # a scratch on either side of the two carve conditions a shape reaches (the pre16 conditions hold for every shape the ABI admits)
    assert seen("T", (425, 426), B=128, **{"pass": "backward"}) and seen("T", (384, 385), B=128, **{"pass": "backward"})
    assert {r["exp"]["share"] for r in back if r["B"] == 128 and r["T"] in (425, 426)} == {0, 1}
    assert {r["exp"]["tail_share"] for r in back if r["B"] == 128 and r["T"] in (384, 385)} == {0, 1}
    infer = [r for r in rows if r["pass"] == "infer"]
    assert seen("poll", (0, 8), **{"pass": "infer"}) and {r["exp"]["poll"] for r in infer} == {8, 16, 32}
    assert seen("NS", (1,), chain=1, **{"pass": "infer"}) and {r["exp"]["clear"] for r in infer} == {0, 2}


def check_invariants(r, p):
    carves = [p["scratch"]] + ([p["tail_scratch"]] if r["pass"] == "backward" else [])
    for c in carves:
        parts = sorted((off, off + n) for off, n in (c["w_ih16"], c["dg16"], c["rest"]) if n)
        assert all(a % 256 == 0 and b % 256 == 0 for a, b in parts), parts
        assert all(x[1] <= y[0] for x, y in zip(parts, parts[1:])) and parts[-1][1] <= c["total"], parts
        assert c["rest"][1] >= 0 and c["rest"][0] + c["rest"][1] == c["total"]
    b = p["bounds"]
    assert b[0] == 0 and b[-1] == r["T"] and all(x < y for x, y in zip(b, b[1:]))
    assert p["overlap"] or len(b) == 2
    if p["overlap"]:
        # even bounds (rows per range a multiple of 128 at B = 64).  An odd T cannot end on one: the evenly split front part then
        # ends odd, and the short ranges behind it (16, 32, ... steps) keep that parity; every bound in front of them is even.
        odd = [x % 2 for x in b]
        assert odd == sorted(odd) and (r["T"] % 2 == 1 or not any(odd))
        assert all(y - x in (16, 32, 64, 128, 256) for x, y in zip(b, b[1:]) if x % 2)
        assert r["T"] >= 32 and not p["chain_a"]["on"] and not (r["pass"] == "forward" and p["chained"])
    assert not p["chain_b"]["on"] or r["pass"] == "forward" or p["chain_a"]["on"]              # backward: chain_b => chain_a
    for c in (p["chain_a"], p["chain_b"]):
        assert c["on"] == (c["asked"] and c["reason"] == 0) and (c["asked"] or c["reason_text"] == "not asked for")
    if r["pass"] == "backward":
        assert p["ddin_ws"][0] >= p["scratch"]["w_ih16"][1] and sum(p["ddin_ws"]) == p["scratch"]["total"]
        assert not p["chunk_cast"] or (p["share"] and p["pre16"] and list(p["ddin_ws"]) == list(p["scratch"]["rest"]))
        assert (p["dec_wgrads"] == "tail") == (p["chain_a"]["on"] and p["defer"]) and p["tail_on_side"] == p["defer"]
    else:
        assert p["chained"] == (p["chain_a"]["on"] or p["chain_b"]["on"]) == (p["poison_words"] > 0) == (p["clear"] != "status")


def test_every_recorded_pass_takes_the_recorded_decisions():
    from tacotron2_subword_amd import _lib as L
    rows = load_rows()
    plans = [plan(L, r) for r in rows]
    wrong = [(r, as_recorded(r, p, r["exp"])) for r, p in zip(rows, plans) if as_recorded(r, p, r["exp"]) != r["exp"]]
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ, first: {wrong[0]}"
    for r, p in zip(rows, plans):
        check_invariants(r, p)


def test_forward_and_backward_take_the_same_steps():
    """The backward pass reads the weight shadows the forward pass cast: one rule (teacher_step_mode) serves both plans."""
    from tacotron2_subword_amd import _lib as L
    seen = set()
    for r in load_rows():
        if r["pass"] == "infer":
            continue
        f, b = plan(L, r, **{"pass": "forward"}), plan(L, r, **{"pass": "backward"})
        assert (f["use16"], f["split"]) == (b["use16"], b["split"]) and not (f["use16"] and f["split"])
        assert all(getattr(f["layout"], n) == getattr(b["layout"], n) for n, _ in f["layout"]._fields_)
        seen.add((f["use16"], f["split"]))
    assert seen == {(False, False), (True, False), (False, True)}


def test_the_plan_reads_its_environment_from_its_arguments():
    """No mode or switch in force changes a plan: the same row under another precision mode in force gives the same answer."""
    from tacotron2_subword_amd import _lib as L
    rows = [r for r in load_rows() if r["precision"] == "bf16"][:40]
    before = [plan(L, r) for r in rows]
    mode = L.get_precision()
    try:
        L.set_precision("bf16x3" if mode != "bf16x3" else "f32")
        after = [plan(L, r) for r in rows]
    finally:
        L.set_precision(mode)
    strip = lambda p: {k: v for k, v in p.items() if k not in ("layout", "bwd_layout")}
    assert [strip(p) for p in before] == [strip(p) for p in after]
    assert all(x["layout"].total_floats == y["layout"].total_floats for x, y in zip(before, after))
