"""CPU-only: the GEMM dispatch (csrc/gemm_dispatch.hip plan_gemm) through t2_gemm_plan, which launches nothing.

tests/golden/gemm_plans.jsonl holds, for about 1 500 products, what the commit BEFORE plan_gemm existed decided (its first
line says how it was recorded): kernel, split-K factor, which operands gemm() stages, or the refusal.  Every row must come
out the same, exactly.  The invariants the dispatch promises in comments are asserted from the plan alone."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_plans.jsonl")
PLACEHOLDER = dict(A=0x10000000, B=0x20000000, C=0x30000000, ws=0x40000000)      # only their alignment is looked at


def load_rows(t256=None):
    with open(FIXTURE) as f:
        head, *rows = [json.loads(line) for line in f]
    assert "comment" in head and "exp" not in head
    return [r for r in rows if t256 is None or r.get("t256", 1) == t256]


def plan_row(L, r):
    """The library's answer for one fixture row: the plan as a dict, or dict(rc=, error=) for a refusal."""
    g = r.get
    L.set_precision({0: "f32", 1: "bf16", 2: "bf16x3"}[r["mode"]])
    L.lib().t2_set_gemm_staging(g("stage", 1))
    L.set_gemm_split_min_mflop(g("split_min", -1))
    M, N, K, batch = r["M"], r["N"], r["K"], g("batch", 1)
    a = L.GemmArgs()
    a.A, a.B, a.C, a.M, a.N, a.K = PLACEHOLDER["A"] + g("a_off", 0), PLACEHOLDER["B"] + g("b_off", 0), PLACEHOLDER["C"], M, N, K
    a.sam, a.sak = (1, g("lda") or M) if g("ta") else (g("lda") or K, 1)          # ta: A is stored [K][M]
    a.sbn, a.sbk = (g("ldb") or K, 1) if g("tb") else (1, g("ldb") or N)          # tb: B is stored [N][K]
    if "strides" in r:
        a.sam, a.sak, a.sbn, a.sbk = r["strides"]
    a.ldc, a.batch, a.alpha, a.beta, a.splitk = N, batch, 1.0, g("beta", 0.0), g("splitk", 0)
    if batch > 1:
        a.bsA, a.bsB, a.bsC = M * K, N * K, M * N
    if g("ws"):
        a.ws, a.ws_bytes = PLACEHOLDER["ws"] + g("ws_off", 0), r["ws"]
    conv, a16, b16 = g("conv", ""), g("a16"), g("b16")
    opts = dict(conv_a=int("a" in conv), conv_b=int("b" in conv), conv_T=g("conv_T", 0), conv_C=g("conv_C", 0), fp32_only=g("fp32_only", 0),
                a16=int(bool(a16)), b16=int(bool(b16)), split16=g("split16", 0))
    if a16:
        opts.update(lda16=a16["ld"], a16_kmajor=a16["km"])
    if b16:
        opts.update(ldb16=b16["ld"], b16_kmajor=b16["km"])
    info = L.GemmPlanInfo()
    rc = L.lib().t2_gemm_plan(C.byref(a), C.byref(L.GemmPlanOpts(**opts)), C.byref(info))
    if rc != 0:
        return dict(rc=rc, error=L.lib().t2_last_error().decode())
    assert L.gemm_plan(a, **opts)["name"] == info.name.decode()
    return {k: (getattr(info, k).decode() if k == "name" else getattr(info, k)) for k, _ in L.GemmPlanInfo._fields_}


def plan_rows(rows):
    from tacotron2_subword_amd import _lib as L
    try:
        return [plan_row(L, r) for r in rows]
    finally:
        L.set_precision("f32"); L.lib().t2_set_gemm_staging(1); L.set_gemm_split_min_mflop(-1)


def as_recorded(p):
    if "rc" in p:
        return p
    return dict(kernel=p["name"], splitk=p["splitk"], stageA=int(p["a_src"] == 1), stageB=int(p["b_src"] == 1))


def check_against_fixture(rows, plans):
    assert len(rows) == len(plans)
    wrong = [(r, as_recorded(p)) for r, p in zip(rows, plans) if as_recorded(p) != r["exp"]]
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ, first: {wrong[0]}"


def check_invariants(r, p):
    if "rc" in p:
        return
    M, N, K, batch, ws, name = r["M"], r["N"], r["K"], r.get("batch", 1), r.get("ws", 0), p["name"]
    src = p["kernel"] >= 3                                               # T2_GEMM_SRC128 and up: reads bf16 copies
    assert name == ("x3" if p["split"] else "") + ("f32_64", "f32_128", "bf16conv", "src128", "src256", "src256km")[p["kernel"]]
    assert (p["a_src"] != 0 and p["b_src"] != 0) if src else (p["a_src"] == 0 and p["b_src"] == 0 and not p["split"])
    assert (p["stage_bytes_a"] > 0) == (p["a_src"] == 1) and (p["stage_bytes_b"] > 0) == (p["b_src"] == 1)
    assert p["splitk"] >= 1 and batch * p["splitk"] <= 65535
    partials = p["splitk"] * M * N * 4 * batch if p["splitk"] > 1 else 0
    if p["splitk"] > 1:
        assert ws > 0 and r.get("beta", 0.0) == 0.0
    assert partials + p["stage_bytes_a"] + p["stage_bytes_b"] <= ws
    kch = -(-(3 * K if p["split"] else K) // 16)                         # 16-wide K-chunks of the product the kernel sees
    assert (p["splitk"] - 1) * p["kchunks"] < kch <= p["splitk"] * p["kchunks"]          # every split has work, all of K is covered
    if "src256" in name:                                                 # two 64-wide K-tiles in every split, the last included
        assert p["kchunks"] >= 8 and kch - (p["splitk"] - 1) * p["kchunks"] >= 8
    if r["mode"] == 0:
        assert name in ("f32_64", "f32_128")
    if r["mode"] == 2:
        assert name in ("f32_64", "f32_128") or name.startswith("x3src")
    if r.get("fp32_only") or r.get("stage", 1) == 0:
        assert not src


def test_fixture_covers_the_dispatch():
    rows = load_rows()
    assert 1500 <= len(rows) <= 3000 and os.path.getsize(FIXTURE) < (1 << 20)
    seen = {(r["mode"], r["exp"].get("kernel", "refused")) for r in rows}
    for mode, names in ((0, ("f32_64", "f32_128")), (1, ("f32_64", "f32_128", "bf16conv", "src128", "src256", "src256km")),
                        (2, ("f32_64", "f32_128", "x3src128", "x3src256", "x3src256km"))):
        assert all((mode, n) in seen for n in names + ("refused",)), mode
    assert sum(r.get("t256", 1) == 0 for r in rows) >= 100


def test_every_recorded_product_takes_the_recorded_plan():
    rows = load_rows(t256=1)
    if os.environ.get("T2_GEMM_256", "1") != "1":
        pytest.fail("T2_GEMM_256 is set in the environment: the fixture's t256=1 rows need the default")
    plans = plan_rows(rows)
    check_against_fixture(rows, plans)
    for r, p in zip(rows, plans):
        check_invariants(r, p)


def test_rows_recorded_without_the_256_tile_kernel():
    """T2_GEMM_256 is read once per process: those rows get a process of their own."""
    code = ("import json, sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']\n"
            "import test_gemm_plan_cpu as T\n"
            "print('PLANS ' + json.dumps(T.plan_rows(T.load_rows(t256=0))))\n")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code, ROOT]
    p = subprocess.run(cmd, env=dict(os.environ, T2_GEMM_256="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    plans = json.loads([line for line in p.stdout.splitlines() if line.startswith("PLANS ")][-1][6:])
    rows = load_rows(t256=0)
    check_against_fixture(rows, plans)
    for r, q in zip(rows, plans):
        assert "256" not in q.get("name", "")
        check_invariants(r, q)
