"""Dev tool: the SSIM loss term on the GPU, HIP path against the torch-op statement, in one process.

  python scripts/time_ssim.py [--batch 64] [--frames 400] [--repeats 3] [--warmup 2] [--timed 5] [--train-step]

Workload: x, y [B,1,80,T] fp32 mel-like, x requires grad; one call = forward + backward of -SSIM(11, True)(x, y), as
Tacotron2Loss(ssim_weight > 0) issues it.  "hip" is tacotron2_subword_amd.ssim.SSIM (csrc/ssim.hip), "torch" is the
module's _ssim (5 grouped conv2d + element-wise ops + autograd) on the same CUDA tensors.  The two alternate; per repeat
--warmup calls, then --timed calls each between its own pair of events; reported: the median of all timed calls and their
min-to-max spread.  The HIP path counts as not slower when its median lies below the other's by more than the larger of
the two spreads.  Then the entry points alone (t2_ssim_forward with and without stored maps, t2_ssim_backward), the same
way, with the bytes each moves and the rate that makes.

--train-step: one train_step (forward, loss, backward, clip, Adam) of the model at the bench shape with ssim_weight 0,
with ssim_weight 1 on the HIP path, and with ssim_weight 1 forced onto _ssim.  A run without a GPU fails."""
import argparse, os, statistics, sys
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--frames", type=int, default=400)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--timed", type=int, default=5)
ap.add_argument("--train-step", action="store_true")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from tacotron2_subword_amd import _lib as L
from tacotron2_subword_amd import ssim as S

assert torch.cuda.is_available(), "time_ssim.py measures on the GPU: none found"
B, T, WS = a.batch, a.frames, 11


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(work):
    """work: [(name, fn)]; returns {name: [ms of every timed call]}."""
    times = {name: [] for name, _ in work}
    for _ in range(a.repeats):
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
        print(f"{name:44s} {len(v):3d} calls  median {med:9.4f} ms  min {min(v):9.4f}  max {max(v):9.4f}  spread {spread:.4f} ms"
              + (f"  {extra[name]}" if extra and name in extra else ""), flush=True)
    return stats


if a.train_step:
    from tacotron2_subword_amd import train as TR
    from tacotron2_subword_amd.hparams import create_hparams
    hp = create_hparams()
    model, optimizer, _ = TR.make_training_objects(hp)
    x, y = model.parse_batch(TR.synthetic_batch(hp, B, 100, 60, T))
    from tacotron2_subword_amd.loss_function import Tacotron2Loss
    crit = {"ssim_weight 0": Tacotron2Loss(hp.alignloss), "ssim_weight 1, HIP path": Tacotron2Loss(hp.alignloss, ssim_weight=1.0),
            "ssim_weight 1, torch-op _ssim forced": Tacotron2Loss(hp.alignloss, ssim_weight=1.0)}
    forced = crit["ssim_weight 1, torch-op _ssim forced"].ssim
    win = S.create_window(WS, 1).cuda()
    forced.forward = lambda i1, i2: S._ssim(i1, i2, win, WS, 1, True)
    work = [(f"train_step B={B} T={T}, {n}", (lambda c=c: TR.train_step(model, c, optimizer, x, y, hp))) for n, c in crit.items()]
    report(alternate(work))
    sys.exit(0)

g = torch.Generator().manual_seed(11)
y = (torch.randn(B, 1, 80, T, generator=g) * 2 - 5).clamp(-11.5129, 2.0).cuda()
x = (y + 0.3 * torch.randn(B, 1, 80, T, generator=g).cuda()).requires_grad_(True)
mod = S.SSIM(WS, True)
win = S.create_window(WS, 1).cuda()


def hip():
    x.grad = None
    (-mod(x, y)).backward()


def torch_ops():
    x.grad = None
    (-S._ssim(x, y, win, WS, 1, True)).backward()


hip(); g_hip = x.grad.clone()
torch_ops(); g_ref = x.grad.clone()
with torch.no_grad():
    v_hip, v_ref = float(mod(x, y)), float(S._ssim(x, y, win, WS, 1, True))
print(f"B={B} [B,1,80,{T}] ws={WS}: value hip {v_hip:.7f} torch-op {v_ref:.7f}; max |dx hip - dx torch-op| {float((g_hip - g_ref).abs().max()):.3e} "
      f"(max |dx| {float(g_ref.abs().max()):.3e})", flush=True)
st = report(alternate([("hip forward + backward", hip), ("torch-op forward + backward", torch_ops)]))
(mh, sh), (mt, stt) = st["hip forward + backward"], st["torch-op forward + backward"]
margin = max(sh, stt)
print(f"ratio torch-op / hip = {mt / mh:.2f}; hip median below torch-op median by {mt - mh:.4f} ms, larger spread {margin:.4f} ms: "
      f"{'NOT SLOWER (passes)' if mt - mh > margin else 'FAILS the condition'}", flush=True)

# the entry points alone
N, H, W = B, 80, T
xd = x.detach()
taps = S._taps(WS, xd.device)
plans = {n: L.ssim_plan(N, H, W, WS, n) for n in (0, 1)}
partial = torch.empty(plans[0].partial_bytes // 8, device="cuda", dtype=torch.float64)
coef = torch.empty(plans[1].map_bytes // 8, device="cuda", dtype=torch.float64)
value, dx, gr = torch.empty(1, device="cuda"), torch.empty_like(xd), torch.full((1,), -1.0, device="cuda")
img = L.ssim_image


def fwd(need):
    L.ssim_forward(L.SsimFwdArgs(B, 1, H, W, WS, need, img(xd), img(y), img(None), L.ptr(taps), L.ptr(partial), L.ptr(coef) if need else None, L.ptr(value), None))


def bwd():
    L.ssim_backward(L.SsimBwdArgs(B, 1, H, W, WS, 1, 0, img(xd), img(y), img(dx), img(None), L.ptr(taps), L.ptr(coef), L.ptr(gr)))


plane = 4.0 * N * H * W
moved = {"t2_ssim_forward, no gradient (tile + finish)": 2 * plane, "t2_ssim_forward, need_grad=1 (tile + finish)": 8 * plane,
         "t2_ssim_backward, dx": 9 * plane}
times = alternate([("t2_ssim_forward, no gradient (tile + finish)", lambda: fwd(0)), ("t2_ssim_forward, need_grad=1 (tile + finish)", lambda: fwd(1)),
                   ("t2_ssim_backward, dx", bwd)])
report(times, {n: f"{moved[n] / 1e6:.1f} MB compulsory -> {moved[n] / (statistics.median(v) * 1e-3) / 1e9:.0f} GB/s" for n, v in times.items()})
p = plans[1]
print(f"plan: tile {p.tile_h}x{p.tile_w}, {p.tiles_h}x{p.tiles_w} tiles per plane, {p.partials} partials ({p.partial_bytes} B), stored maps {p.map_bytes / 1e6:.1f} MB, "
      f"LDS {p.lds_fwd_bytes} B forward / {p.lds_bwd_bytes} B backward per workgroup", flush=True)
