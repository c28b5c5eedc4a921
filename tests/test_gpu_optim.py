"""GPU tests of the gradient-norm + Adam kernels (csrc/optim.hip) through the C ABI with hand-built tables, and of
optim.FusedAdam itself, against the fp64 restatement of tests/adam_ref.py: one step at a time, from a snapshot of the
float32 inputs and with the clip coefficient the device itself computed.

ABI level: p, g, m and v live in four flat device buffers; each table row is a slice at an element offset the test chooses,
so that rows start 0 to 3 elements past a 16-byte boundary (the scalar branches of sumsq_kernel and adam_kernel: the path
every gradient of distributed.GradArena takes behind the one-element gate bias).  Everything between the rows holds a
sentinel value; after every launch the sentinels of all four buffers and the whole of g must be bit-identical.

Bounds (derived in adam_ref.py, u = 2^-24): norm within 32u relative; the coefficient bit for bit min(1, max_norm /
(norm + 1e-6)) in float32 from the device's own norm; p, m and v per element within bp, bm, bv.  Each test prints the worst
share of its bounds.  Measured on an MI355X (profiles/r11_adam_tests.txt): the norm uses at most 4 % of 32u, p at most
0.50 of bp (the rounding of p itself), m 0.16 of bm, v 0.46 of bv; the coefficient is bit for bit the float32 formula."""
import copy
import functools

import numpy as np
import pytest
import torch

import adam_ref as A

pytestmark = pytest.mark.gpu

SENT = 8                 # sentinel floats between rows
SENTINEL = 1234.5        # finite: a kernel that reads one moves the norm far out of its bound, one that steps it changes its bits
CHUNK = 8192             # elements per workgroup (optim.hip kChunk): a row of n elements covers ceil(n / 8192) chunks
HP = A.hyper(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
SIZES = [1, 3, 4, 5, 255, 256, 1023, 1024, 1025, 8191, 8192, 8193, 2 * 8192 + 7]
STEPS = [1, 2, 7, 1000, 100000]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def lib():
    from tacotron2_subword_amd import _lib as L
    return L.lib()


class Table:
    """A table of rows over four flat buffers.  numels[i] elements per row; g_align[i] / pmv_align[i] = elements past a
    16-byte boundary at which the row starts in g / in p, m, v, or None = packed right behind the previous row's sentinels
    (alignments then mix on their own).  lead = sentinel floats in front of the first row."""

    def __init__(self, numels, g_align=None, pmv_align=None, lead=SENT):
        from tacotron2_subword_amd.optim import _AdamTensor
        self.lib, self.n, self.numels = lib(), len(numels), list(numels)
        assert lead >= SENT and lead % 4 == 0

        def place(aligns):
            offs, cur = [], lead
            for n, a in zip(numels, aligns or [None] * self.n):
                if a is not None:
                    cur = (cur + 3) // 4 * 4 + a
                offs.append(cur)
                cur += n + SENT
            return offs, cur

        self.off_g, size_g = place(g_align)
        self.off, size = place(pmv_align)
        self.size = dict(g=size_g, p=size, m=size, v=size)
        self.row_of = np.repeat(np.arange(self.n), numels)
        self.idx_g = np.concatenate([np.arange(o, o + n) for o, n in zip(self.off_g, numels)])
        self.idx = np.concatenate([np.arange(o, o + n) for o, n in zip(self.off, numels)])
        self.total = int(sum(numels))
        self.first_chunk = np.concatenate([[0], np.cumsum([(n + CHUNK - 1) // CHUNK for n in numels])]).astype(int)
        assert all(self.lib.t2_adam_chunks(n) == (n + CHUNK - 1) // CHUNK for n in numels)
        self.chunks = int(self.first_chunk[-1])
        self.dev = {k: torch.full((self.size[k],), SENTINEL, dtype=torch.float32, device="cuda") for k in "pgmv"}
        assert all(self.dev[k].data_ptr() % 16 == 0 for k in "pgmv")
        rows = (_AdamTensor * self.n)()
        for i in range(self.n):
            rows[i].p, rows[i].m, rows[i].v = (self.dev[k].data_ptr() + 4 * self.off[i] for k in "pmv")
            rows[i].g = self.dev["g"].data_ptr() + 4 * self.off_g[i]
            rows[i].numel, rows[i].first_chunk = numels[i], int(self.first_chunk[i])
        self.tab = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).cuda()
        self.partial = torch.zeros(self.chunks + 2, dtype=torch.float32, device="cuda")
        self.norm_out = torch.zeros(4, dtype=torch.float32, device="cuda")

    def misaligned(self, key):
        base, offs = self.dev[key].data_ptr(), self.off_g if key == "g" else self.off
        return [(base + 4 * o) % 16 != 0 for o in offs]

    def fill(self, p, g, m, v):
        """Row contents from flat float32 arrays of `total` elements (rows in order); everything else becomes the sentinel."""
        for k, x in zip("pgmv", (p, g, m, v)):
            h = np.full(self.size[k], SENTINEL, dtype=np.float32)
            h[self.idx_g if k == "g" else self.idx] = x
            self.dev[k].copy_(torch.from_numpy(h))
        self.norm_out.fill_(-1.0)

    def read(self):
        torch.cuda.synchronize()
        out = {k: self.dev[k].cpu().numpy() for k in "pgmv"}
        out["norm_out"] = self.norm_out.cpu().numpy()
        return out

    def norm(self, max_norm):
        from tacotron2_subword_amd import _lib as L
        L.check(self.lib.t2_adam_norm(L.adam_table(self.tab.data_ptr()), self.n, self.chunks, self.partial.data_ptr(), self.norm_out.data_ptr(),
                                      float(max_norm), L.stream()))

    def step(self, max_norm, t, hp=HP, rows=None):
        """t2_adam_step over rows [r0, r1) (default: all), as FusedAdam calls it: a pointer to row r0 and those rows' chunks."""
        from tacotron2_subword_amd import _lib as L
        r0, r1 = rows or (0, self.n)
        L.check(self.lib.t2_adam_step(L.adam_table(self.tab.data_ptr() + 48 * r0), r1 - r0, int(self.first_chunk[r1] - self.first_chunk[r0]),
                                      self.partial.data_ptr(), self.norm_out.data_ptr(), float(max_norm), hp["lr"], hp["b1"], hp["b2"],
                                      hp["eps"], hp["wd"], int(t), L.stream()))

    def check_untouched(self, before, after, rows=None):
        """Bit-identical: g as a whole, everything outside the rows in p, m, v, and every row outside [r0, r1)."""
        assert np.array_equal(bits(before["g"]), bits(after["g"])), "g was written"
        r0, r1 = rows or (0, self.n)
        stepped = np.zeros(self.size["p"], dtype=bool)
        stepped[self.idx[(self.row_of >= r0) & (self.row_of < r1)]] = True
        for k in "pmv":
            same = bits(before[k]) == bits(after[k])
            assert bool(same[~stepped].all()), f"{k}: {int((~same[~stepped]).sum())} words outside rows [{r0}, {r1}) changed"

    def check_norm(self, before, after, max_norm, label):
        """Norm within its bound, coefficient bit for bit, skip flag clear.  Returns (the device's coefficient, share)."""
        norm64 = A.total_norm([before["g"][self.idx_g]])
        norm, coef, skip = after["norm_out"][:3]
        if np.isfinite(norm64):
            err = abs(float(norm) - norm64)
            share = err / (A.NORM_BOUND * norm64) if norm64 > 0 else float(err != 0)
        else:
            share = 0.0 if (np.isnan(norm) if np.isnan(norm64) else norm == norm64) else np.inf
        print(f"{label}: norm {float(norm):.9g}, fp64 {norm64:.9g}, used {100 * share:.1f}% of 32u")
        assert share <= 1.0
        want = A.clip_coef_f32(norm, max_norm)
        assert (np.isnan(coef) and np.isnan(want)) or bits(np.float32(coef)) == bits(np.float32(want)), (label, float(coef), float(want))
        assert skip == 0.0
        return float(coef), share

    def check_rows(self, before, after, clip, t, label, hp=HP, rows=None):
        """p, m, v of rows [r0, r1) against one fp64 step from `before`; non-finite exactly where fp64 is.  Returns the shares."""
        r0, r1 = rows or (0, self.n)
        sel = (self.row_of >= r0) & (self.row_of < r1)
        ip, ig = self.idx[sel], self.idx_g[sel]
        ref = A.step(before["p"][ip], before["g"][ig], before["m"][ip], before["v"][ip], clip, t, **hp)
        shares = {}
        for k in "pmv":
            got, want, bound = after[k][ip].astype(np.float64), ref[k], ref["b" + k]
            ok = np.isfinite(want)
            assert np.array_equal(np.isfinite(got), ok), f"{label} {k}: non-finite values differ from fp64"
            assert bool(np.isnan(got[~ok]).all())
            shares[k] = float((np.abs(got[ok] - want[ok]) / bound[ok]).max()) if ok.any() else 0.0
        print(f"{label}: t={t} clip={clip:.6g}: share of bound used: p {shares['p']:.3f}, m {shares['m']:.3f}, v {shares['v']:.3f}")
        assert max(shares.values()) <= 1.0, (label, shares)
        return shares


def inputs(total, t, pscale, gkind, seed, hp=HP):
    """Flat p, g, m, v (float32) and max_norm.  gkind: a gradient scale (1, 1e-3, 0) or "cancel": g = -wd*p/clip to within
    1e-6 at clip = 0.37, so that g' = g*clip + wd*p cancels.  max_norm = 0.37 * (norm + 1e-6), which makes the device's
    coefficient 0.37 to rounding (for g = 0: 1.0, coefficient exactly 1).  t = 1: m = v = 0, as on a first step."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(total) * pscale).astype(np.float32)
    if gkind == "cancel":
        g = (-hp["wd"] * p.astype(np.float64) / 0.37 * (1.0 + 1e-6 * rng.uniform(-1, 1, total))).astype(np.float32)
        s = hp["wd"] * pscale
    else:
        g = (rng.standard_normal(total) * gkind).astype(np.float32)
        s = gkind if gkind > 0 else 1e-3
    if t == 1:
        m, v = np.zeros(total, np.float32), np.zeros(total, np.float32)
    else:
        m = (0.1 * s * rng.standard_normal(total)).astype(np.float32)
        v = np.square(0.1 * s * rng.standard_normal(total)).astype(np.float32)
    norm = A.total_norm([g])
    return p, g, m, v, (A.f32(0.37 * (norm + 1e-6)) if norm > 0 else 1.0)


def run_full(tab, p, g, m, v, max_norm, t, label, hp=HP):
    """One t2_adam_step over the whole table with every check; returns (before, after)."""
    tab.fill(p, g, m, v)
    before = tab.read()
    tab.step(max_norm, t, hp)
    after = tab.read()
    tab.check_untouched(before, after)
    clip, _ = tab.check_norm(before, after, max_norm, label)
    tab.check_rows(before, after, clip, t, label, hp)
    return before, after


# ---------------------------------------------------------------------------------------------------------------- ABI level

@functools.lru_cache(maxsize=None)
def alignment_table():
    """Every size with g starting 0, 1, 2, 3 elements past a 16-byte boundary while p, m, v are aligned (gradients packed
    in an arena), then once more with all four 1 element past."""
    cases = [(n, ag, 0) for n in SIZES for ag in range(4)] + [(n, 1, 1) for n in SIZES]
    tab = Table([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert sum(tab.misaligned("g")) == 4 * len(SIZES) and sum(tab.misaligned("p")) == len(SIZES)
    return tab


@pytest.mark.parametrize("pscale", [1.0, 1e-4])
@pytest.mark.parametrize("t", STEPS)
def test_sizes_by_alignment(t, pscale):
    tab = alignment_table()
    for k, gkind in enumerate([1.0, 1e-3, 0.0, "cancel"]):
        p, g, m, v, max_norm = inputs(tab.total, t, pscale, gkind, seed=1000 * STEPS.index(t) + 10 * k + int(pscale < 1))
        _, after = run_full(tab, p, g, m, v, max_norm, t, f"align t={t} p~{pscale:g} g={gkind}")
        if gkind == "cancel":
            assert abs(float(after["norm_out"][1]) - 0.37) < 1e-6


def test_many_rows_more_than_1024_chunks():
    """1300 small rows at mixed alignments with one four-chunk row in the middle: norm_finish_kernel strides over 1303
    partials, find_tensor searches 1300 rows, and behind the large row a row's index and its first chunk differ."""
    numels = [1 + i % 9 for i in range(1300)]
    numels[650] = 3 * CHUNK + 5
    tab = Table(numels)
    assert tab.chunks == 1303 and 0 < sum(tab.misaligned("g")) < tab.n
    p, g, m, v, max_norm = inputs(tab.total, 2, 1.0, 1.0, seed=7)
    run_full(tab, p, g, m, v, max_norm, 2, "many rows")
    p, g, m, v, _ = inputs(tab.total, 2, 1.0, 1.0, seed=8)
    g[:] = 0
    row = int(np.flatnonzero(tab.first_chunk[:-1] == 1024)[0])
    g[tab.row_of == row] = 3.0            # the whole norm sits in the partial at index 1024, the first of the second stride
    before, after = run_full(tab, p, g, m, v, 1.0, 2, "many rows, one live partial")
    assert after["norm_out"][0] > 0


def test_sub_table_steps_only_its_rows():
    """The multi-batch path of FusedAdam.step: the norm over all 12 rows, then t2_adam_step(max_norm = -1) per run of rows,
    each with hyper-parameters and a step count of its own.  The buffers carry a band of sentinels in front as long as the
    table's chunks, so that a kernel which loses a sub-table's first chunk lands in checked memory."""
    numels = [5, 8193, 100, 9000, 3, 8192, 8200, 1, 10000, 257, 2 * CHUNK + 1, 7]
    tab = Table(numels, lead=sum((n + CHUNK - 1) // CHUNK for n in numels) * CHUNK)
    p, g, m, v, max_norm = inputs(tab.total, 7, 1.0, 1.0, seed=11)
    tab.fill(p, g, m, v)
    before = tab.read()
    tab.norm(max_norm)
    after = tab.read()
    tab.check_untouched(before, after, rows=(0, 0))
    clip, _ = tab.check_norm(before, after, max_norm, "sub-table")
    assert clip < 1.0
    runs = [((5, 9), 7, HP), ((0, 5), 3, A.hyper(lr=3e-4, betas=(0.9, 0.999), weight_decay=1e-6)),
            ((9, 12), 1000, A.hyper(lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1))]
    for rows, t, hp in runs:
        before = after
        tab.step(-1.0, t, hp, rows=rows)
        after = tab.read()
        tab.check_untouched(before, after, rows=rows)
        assert np.array_equal(bits(before["norm_out"]), bits(after["norm_out"]))
        tab.check_rows(before, after, clip, t, f"sub-table rows {rows}", hp, rows=rows)


@functools.lru_cache(maxsize=None)
def small_table():
    return Table([5, 8193, 300, 1, 1025], [1, 0, 2, 3, 0], [0, 0, 0, 1, 0])


def test_coefficient_edges():
    tab = small_table()
    p, g, m, v, _ = inputs(tab.total, 7, 1.0, 1.0, seed=21)
    norm = A.total_norm([g])
    for name, max_norm in (("far above", 1e-3 * norm), ("far below", 1e3 * norm), ("max_norm 0", 0.0)):
        before, after = run_full(tab, p, g, m, v, max_norm, 7, f"coefficient, norm {name}")
        coef = after["norm_out"][1]
        assert after["norm_out"][2] == 0.0 and abs(float(after["norm_out"][0]) - norm) <= A.NORM_BOUND * norm
        if name == "far above":
            assert 0.999e-3 < coef < 1.001e-3
        else:
            assert bits(np.float32(coef)) == bits(np.float32(1.0))


def test_skip_flag_leaves_everything_untouched():
    tab = small_table()
    p, g, m, v, _ = inputs(tab.total, 7, 1.0, 1.0, seed=22)
    tab.fill(p, g, m, v)
    tab.norm_out.copy_(torch.tensor([1.0, 0.5, 1.0, 0.0]))       # norm, coefficient, "skip the update"
    before = tab.read()
    tab.step(-1.0, 7)
    after = tab.read()
    tab.check_untouched(before, after, rows=(0, 0))
    assert np.array_equal(bits(before["norm_out"]), bits(after["norm_out"]))
    tab.norm_out.copy_(torch.tensor([1.0, 0.5, 0.0, 0.0]))       # the same call with the flag clear does step
    tab.step(-1.0, 7)
    after = tab.read()
    tab.check_untouched(before, after)
    tab.check_rows(before, after, 0.5, 7, "skip flag clear")


def test_same_table_twice_gives_the_same_bits():
    tab = small_table()
    p, g, m, v, max_norm = inputs(tab.total, 7, 1.0, 1.0, seed=23)
    runs = []
    for _ in range(2):
        tab.fill(p, g, m, v)
        tab.step(max_norm, 7)
        runs.append(tab.read())
    for k in ("norm_out", "p", "g", "m", "v"):
        assert np.array_equal(bits(runs[0][k]), bits(runs[1][k])), k
    assert runs[0]["norm_out"][1] < 1.0


def test_nan_gradient_makes_every_parameter_nan():
    """One NaN gradient: norm NaN, coefficient NaN (fminf would have made it 1 and stepped every other parameter with its
    unclipped gradient), every row's p NaN, as after clip_grad_norm_."""
    tab = small_table()
    p, g, m, v, _ = inputs(tab.total, 7, 1.0, 1.0, seed=24)
    g[tab.row_of == 2] = np.where(np.arange(300) == 17, np.float32("nan"), g[tab.row_of == 2])
    tab.fill(p, g, m, v)
    before = tab.read()
    tab.step(1.0, 7)
    after = tab.read()
    tab.check_untouched(before, after)
    assert np.isnan(after["norm_out"][0]) and np.isnan(after["norm_out"][1]) and after["norm_out"][2] == 0.0
    assert bool(np.isnan(after["p"][tab.idx]).all())
    tab.check_norm(before, after, 1.0, "NaN gradient")
    tab.check_rows(before, after, float("nan"), 7, "NaN gradient")


def test_inf_gradient_gives_coefficient_zero():
    """One +Inf gradient: norm +Inf, coefficient 0; that element becomes NaN (Inf * 0), every other one steps with g' = wd*p."""
    tab = small_table()
    p, g, m, v, _ = inputs(tab.total, 7, 1.0, 1.0, seed=25)
    at = int(np.flatnonzero(tab.row_of == 1)[8000])
    g[at] = np.float32("inf")
    tab.fill(p, g, m, v)
    before = tab.read()
    tab.step(1.0, 7)
    after = tab.read()
    tab.check_untouched(before, after)
    assert after["norm_out"][0] == np.float32("inf") and bits(after["norm_out"][1:2]) == bits(np.float32(0.0)) and after["norm_out"][2] == 0.0
    tab.check_norm(before, after, 1.0, "Inf gradient")
    nan = np.isnan(after["p"][tab.idx])
    assert nan[at] and nan.sum() == 1
    tab.check_rows(before, after, 0.0, 7, "Inf gradient")          # fp64 with clip = 0: NaN at that element, g' = wd*p elsewhere


# ------------------------------------------------------------------------------------------------------------- module level

def state_of(opt, p):
    return opt.state.get(p, {})          # (opt.state is a defaultdict: indexing would create the entry the test looks for)


def snapshot(opt):
    torch.cuda.synchronize()
    snap = []
    for group in opt.param_groups:
        h = A.hyper(group["lr"], group["betas"], group["eps"], group["weight_decay"])
        for p in group["params"]:
            st = state_of(opt, p)
            snap.append(dict(param=p, h=h, p=p.detach().cpu().numpy().copy(), g=None if p.grad is None else p.grad.detach().cpu().numpy().copy(),
                             m=st["exp_avg"].cpu().numpy().copy() if st else np.zeros(p.shape, np.float32),
                             v=st["exp_avg_sq"].cpu().numpy().copy() if st else np.zeros(p.shape, np.float32),
                             t=int(st["step"]) if st else 0, empty=len(st) == 0))
    return snap


def checked_step(opt, max_norm, label, **kw):
    """opt.step(max_norm=max_norm, **kw) with every tensor checked against one fp64 step from a snapshot taken just before:
    norm, coefficient (opt.last_clip), p, exp_avg, exp_avg_sq and state["step"] of every live parameter; a parameter
    without a gradient keeps its bits and its state.  Returns what step() returned."""
    snap = snapshot(opt)
    ret = opt.step(max_norm=max_norm, **kw)
    torch.cuda.synchronize()
    live = [s for s in snap if s["g"] is not None]
    norm64 = A.total_norm([s["g"] for s in live])
    norm, clip = np.float32(float(opt.last_norm)), np.float32(float(opt.last_clip))
    nshare = abs(float(norm) - norm64) / (A.NORM_BOUND * norm64)
    assert nshare <= 1.0, (label, float(norm), norm64)
    want = A.clip_coef_f32(norm, max_norm if max_norm else 0.0)
    assert bits(clip) == bits(np.float32(want)), (label, float(clip), float(want))
    shares = dict(p=0.0, m=0.0, v=0.0)
    for s in snap:
        p, st = s["param"], state_of(opt, s["param"])
        if s["g"] is None:
            assert np.array_equal(bits(p.detach().cpu().numpy()), bits(s["p"])), f"{label}: a parameter without a gradient moved"
            assert (len(st) == 0) if s["empty"] else (int(st["step"]) == s["t"] and np.array_equal(bits(st["exp_avg"].cpu().numpy()), bits(s["m"]))
                                                      and np.array_equal(bits(st["exp_avg_sq"].cpu().numpy()), bits(s["v"])))
            continue
        assert np.array_equal(bits(p.grad.detach().cpu().numpy()), bits(s["g"])), f"{label}: a gradient was written"
        assert int(st["step"]) == s["t"] + 1, (label, int(st["step"]), s["t"] + 1)
        ref = A.step(s["p"], s["g"], s["m"], s["v"], float(clip), s["t"] + 1, **s["h"])
        for k, got in (("p", p.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            got = got.cpu().numpy().astype(np.float64)
            assert bool(np.isfinite(got).all())
            shares[k] = max(shares[k], float((np.abs(got - ref[k]) / ref["b" + k]).max()))
    print(f"{label}: norm used {100 * nshare:.1f}% of 32u, clip={float(clip):.6g}, steps {sorted({s['t'] + 1 for s in live})}: "
          f"share of bound used: p {shares['p']:.3f}, m {shares['m']:.3f}, v {shares['v']:.3f}")
    assert max(shares.values()) <= 1.0, (label, shares)
    return ret


def make_params(shapes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, device="cuda", generator=g)) for s in shapes]


def set_grads(params, gen, scale=1.0, dead=()):
    for i, p in enumerate(params):
        p.grad = None if i in dead else torch.randn(p.shape, device="cuda", generator=gen) * scale


def fast_path_is_warm(opt):
    return getattr(opt, "_fast", None) is not None


def test_arena_gradients_five_steps():
    """Gradients as views of distributed.GradArena's flat buffer: behind the one-element parameter most of them start off
    a 16-byte boundary.  Step 1 takes the general path, steps 2 to 5 the fast path; step 3 has its norm below max_norm."""
    from tacotron2_subword_amd.distributed import GradArena
    from tacotron2_subword_amd.optim import FusedAdam
    module = torch.nn.Module()
    module.ps = torch.nn.ParameterList(make_params([(2048,), (1,), (80,), (8193,), (33, 7, 5), (3,)], seed=31))
    params = list(module.parameters())
    arena = GradArena(module)
    gen = torch.Generator(device="cuda").manual_seed(32)
    set_grads(params, gen)
    for p in params:
        arena.adopt(p)
    assert all(p.grad.data_ptr() == arena.view(p).data_ptr() for p in params)
    assert sum(p.grad.data_ptr() % 16 != 0 for p in params) >= 4
    opt = FusedAdam(params, lr=1e-3, weight_decay=1e-6)
    for step in range(1, 6):
        arena.flat.copy_(torch.randn(arena.flat.shape, device="cuda", generator=gen) * (1e-4 if step == 3 else 1.0))
        assert fast_path_is_warm(opt) == (step > 2)
        norm = checked_step(opt, 1.0, f"arena step {step}")
        assert norm is opt.last_norm and (float(opt.last_clip) == 1.0) == (step == 3)
    assert fast_path_is_warm(opt)


def test_two_groups_and_mixed_step_counts():
    """Two groups with different lr, betas, eps and weight decay; one parameter has no gradient for the first two steps.
    One norm over all live parameters of both groups, each parameter corrected with its own step count."""
    from tacotron2_subword_amd.optim import FusedAdam
    params = make_params([(300,), (8200,), (17,), (5, 3)], seed=41)
    opt = FusedAdam([dict(params=params[:2], lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-6),
                     dict(params=params[2:], lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-2)])
    gen = torch.Generator(device="cuda").manual_seed(42)
    for step in range(1, 5):
        set_grads(params, gen, dead=(2,) if step <= 2 else ())
        checked_step(opt, 0.0 if step == 4 else 1.0, f"two groups step {step}")
        if step <= 2:
            assert len(state_of(opt, params[2])) == 0
    assert [int(opt.state[p]["step"]) for p in params] == [4, 4, 2, 4]


def test_restored_state():
    from tacotron2_subword_amd.optim import FusedAdam
    params = make_params([(300,), (8200,), (17,), (5, 3)], seed=51)
    opt = FusedAdam(params, lr=1e-3, weight_decay=1e-6)
    gen = torch.Generator(device="cuda").manual_seed(52)
    for step in range(3):
        set_grads(params, gen)
        checked_step(opt, 1.0, f"restore warm-up {step}")
    assert fast_path_is_warm(opt)
    sd = copy.deepcopy(opt.state_dict())
    for st in sd["state"].values():
        st["step"] = torch.tensor(999.0)
    opt.load_state_dict(sd)
    set_grads(params, gen)
    checked_step(opt, 1.0, "restored at step 999")
    assert all(int(opt.state[p]["step"]) == 1000 for p in params)
    set_grads(params, gen)
    checked_step(opt, 1.0, "restored, second step")                 # warm again: the cache below is a live one
    sd = copy.deepcopy(opt.state_dict())
    del sd["state"][0], sd["state"][2]                              # only parameters 1 and 3 restored
    opt.load_state_dict(sd)
    assert len(state_of(opt, params[0])) == 0 and len(state_of(opt, params[2])) == 0
    set_grads(params, gen)
    checked_step(opt, 1.0, "half restored")
    assert [int(opt.state[p]["step"]) for p in params] == [1, 1002, 1, 1002]


def warm(shapes, seed):
    from tacotron2_subword_amd.optim import FusedAdam
    params = make_params(shapes, seed)
    opt = FusedAdam(params, lr=1e-3, weight_decay=1e-6)
    gen = torch.Generator(device="cuda").manual_seed(seed + 1)
    for step in range(3):
        set_grads(params, gen)
        checked_step(opt, 1.0, f"warm-up {step}")
    assert fast_path_is_warm(opt)
    return params, opt, gen


def test_cache_invalidation_parameter_storage_moved():
    params, opt, gen = warm([(300,), (8200,), (17,)], seed=61)
    old = params[1].data
    old_bits = bits(old.cpu().numpy()).copy()
    params[1].data = params[1].data.clone()
    assert params[1].data_ptr() != old.data_ptr()
    set_grads(params, gen)
    checked_step(opt, 1.0, "p.data replaced")
    assert np.array_equal(bits(old.cpu().numpy()), old_bits), "the old storage was stepped"
    set_grads(params, gen)
    checked_step(opt, 1.0, "p.data replaced, next step")
    assert fast_path_is_warm(opt)


def test_cache_invalidation_moments_replaced_by_load_state_dict():
    params, opt, gen = warm([(300,), (8200,), (17,)], seed=71)
    old = [(opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in params]
    old_bits = [(bits(m.cpu().numpy()).copy(), bits(v.cpu().numpy()).copy()) for m, v in old]
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))            # a checkpoint round trip: new moment tensors
    assert all(opt.state[p]["exp_avg"].data_ptr() != m.data_ptr() for p, (m, _) in zip(params, old))
    set_grads(params, gen)
    checked_step(opt, 1.0, "moments replaced")
    for (m, v), (mb, vb) in zip(old, old_bits):
        assert np.array_equal(bits(m.cpu().numpy()), mb) and np.array_equal(bits(v.cpu().numpy()), vb), "the old moments were stepped"
    assert all(int(opt.state[p]["step"]) == 4 for p in params)


def test_cache_invalidation_parameter_dead_for_a_step():
    """A live parameter loses its gradient for one step, gets it back, and loses it once more: its step count falls behind
    the others', and every step must correct each parameter with its own."""
    params, opt, gen = warm([(300,), (8200,), (17,)], seed=81)
    for k, dead in enumerate([(1,), (), (1,), ()]):
        set_grads(params, gen, dead=dead)
        checked_step(opt, 1.0, f"dead {dead} ({k})")
    assert [int(opt.state[p]["step"]) for p in params] == [7, 5, 7]


def test_max_norm_none_and_closure():
    from tacotron2_subword_amd.optim import FusedAdam
    params = make_params([(300,), (8200,)], seed=91)
    opt = FusedAdam(params, lr=1e-3, weight_decay=1e-6)
    gen = torch.Generator(device="cuda").manual_seed(92)
    for step in range(2):                                           # general path, then fast path
        set_grads(params, gen, scale=10.0)
        norm = checked_step(opt, None, f"max_norm None step {step}")
        assert float(opt.last_clip) == 1.0 and norm is opt.last_norm and float(norm) > 100.0
    for step in range(2):
        loss = torch.tensor(3.25)
        assert checked_step(opt, 1.0, f"closure step {step}", closure=lambda: loss) is loss
    fresh = FusedAdam(make_params([(9,)], seed=93), lr=1e-3)
    set_grads(fresh.param_groups[0]["params"], gen)
    assert checked_step(fresh, 1.0, "closure, general path", closure=lambda: loss) is loss
