"""Pins tests/adam_ref.py, the fp64 yardstick of the FusedAdam GPU tests, against torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam(foreach=False) on fp64 tensors: 1e-12 relative on every parameter and both moments after every step."""
import numpy as np
import torch

import adam_ref as A

RTOL = 1e-12


def run_both(groups, grad_plan, max_norm, seed):
    """groups: list of (shapes, hyper dict); grad_plan[step][k] = gradient scale of parameter k (over all groups, in order)
    or None for no gradient.  Steps torch and the restatement side by side and compares after each step."""
    rng = np.random.default_rng(seed)
    params, tgroups, hyp = [], [], []
    for shapes, h in groups:
        ps = [torch.tensor(rng.standard_normal(s), dtype=torch.float64, requires_grad=True) for s in shapes]
        params += ps
        hyp += [h] * len(ps)
        tgroups.append(dict(params=ps, lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"]))
    opt = torch.optim.Adam(tgroups, foreach=False)
    state = [dict(p=p.detach().numpy().copy(), m=np.zeros(p.shape), v=np.zeros(p.shape), t=0) for p in params]
    coefs = []
    for plan in grad_plan:
        grads = [None if s is None else rng.standard_normal(p.shape) * s for p, s in zip(params, plan)]
        for p, g in zip(params, grads):
            p.grad = None if g is None else torch.tensor(g, dtype=torch.float64)
        want_norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        opt.step()
        norm = A.total_norm([g for g in grads if g is not None])
        assert abs(norm - want_norm) <= RTOL * want_norm
        clip = A.clip_coef(norm, max_norm)
        coefs.append(clip)
        for p, g, st, h in zip(params, grads, state, hyp):
            if g is None:
                assert len(opt.state[p]) == 0 or float(opt.state[p]["step"]) == st["t"]
                np.testing.assert_array_equal(p.detach().numpy(), st["p"])
                continue
            st["t"] += 1
            r = A.step(st["p"], g, st["m"], st["v"], clip, st["t"], **h)
            st["p"], st["m"], st["v"] = r["p"], r["m"], r["v"]
            assert float(opt.state[p]["step"]) == st["t"]
            np.testing.assert_allclose(st["p"], p.detach().numpy(), rtol=RTOL, atol=0)
            np.testing.assert_allclose(st["m"], opt.state[p]["exp_avg"].numpy(), rtol=RTOL, atol=0)
            np.testing.assert_allclose(st["v"], opt.state[p]["exp_avg_sq"].numpy(), rtol=RTOL, atol=0)
            for k in ("bp", "bm", "bv"):
                assert r[k].shape == r["p"].shape and bool((r[k] > 0).all()) and bool(np.isfinite(r[k]).all())
    return coefs


def test_one_group_three_steps_clip_active_and_inactive():
    h = A.hyper(lr=1e-3, weight_decay=1e-6)
    coefs = run_both([([(257,), (3, 5), (1,)], h)], [[1.0] * 3, [1.0] * 3, [1e-3] * 3], max_norm=1.0, seed=0)
    assert coefs[0] < 1.0 and coefs[1] < 1.0 and coefs[2] == 1.0


def test_two_groups_and_a_parameter_that_joins_at_step_two():
    h0 = A.hyper(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6)
    h1 = A.hyper(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-2)
    plan = [[1.0, 1.0, None, 1.0], [1.0, 1.0, 1.0, 1.0], [1e-3, 1e-3, 1e-3, 1e-3]]       # parameter 2 (group 1) joins at step 2
    coefs = run_both([([(64,), (7, 3)], h0), ([(33,), (2,)], h1)], plan, max_norm=0.5, seed=1)
    assert coefs[0] < 1.0 and coefs[1] < 1.0 and coefs[2] == 1.0


def test_hyper_parameters_are_the_c_floats():
    h = A.hyper(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6)
    for k, x in (("lr", 1e-3), ("b1", 0.9), ("b2", 0.999), ("eps", 1e-8), ("wd", 1e-6)):
        assert h[k] == float(np.float32(x)) and np.float32(h[k]) == np.float32(x)
    assert float(np.float32(1.0) - np.float32(0.999)) == 1.0 - h["b2"]       # the kernel's 1.0f - b2 is exact
    assert float(np.float32(1.0) - np.float32(0.9)) == 1.0 - h["b1"]


def test_coefficient_edges():
    assert A.clip_coef(10.0, 1.0) == 1.0 / (10.0 + 1e-6) and A.clip_coef(0.1, 1.0) == 1.0
    assert np.isnan(A.clip_coef(float("nan"), 1.0)) and A.clip_coef(float("inf"), 1.0) == 0.0
    assert np.isnan(A.clip_coef_f32(np.float32("nan"), 1.0)) and A.clip_coef_f32(np.float32("inf"), 1.0) == 0.0
    assert A.clip_coef_f32(np.float32(0.1), 1.0) == 1.0 and A.clip_coef_f32(np.float32(5.0), 0.0) == 1.0
    want = float(torch.clamp(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(3.0, dtype=torch.float32) + 1e-6), max=1.0))
    assert float(A.clip_coef_f32(np.float32(3.0), 1.0)) == want
