"""Dev tool: times of the soft-DTW module (tacotron2_subword_amd/soft_dtw_cuda.py) on the GPU, seeded random mel-like
inputs, gamma = 0.1 as the checkpoint scoring sets it:

  (B, N, M, d) = (1, 800, 800, 80)      forward without gradient, and forward + backward
  (1, 6000, 6000, 80)                   forward without gradient only (the decoder's max_decoder_steps)
  B = 32, 400-800 frames per side, padded to 800 with x_lengths / y_lengths: both

  python scripts/time_softdtw.py [--leg-ms 400] [--warmup 3] [--legs 3] [--host-ref]

Per leg: --warmup calls, then as many calls as fill --leg-ms (sized per workload from a first timed call, at least 5)
between two synchronises on the host clock; every shape is warmed before it is timed and the legs of all workloads
alternate, so the spread between legs is on show.  These are times of the MODULE call: the distance kernel, the scratch
allocations and, with lengths, the host's range check of them (one device-to-host read) are inside; the kernels' own
times come from a kernel trace of this script (profiles/README.md).  A run without a GPU fails.
--host-ref also times the fp64 numpy restatement of tests/softdtw_ref.py on the first shape (host seconds: the kind of
loop the reference runs above 1024 frames, here already vectorised along anti-diagonals)."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--leg-ms", type=float, default=400.0)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--legs", type=int, default=3)
ap.add_argument("--host-ref", action="store_true")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from tacotron2_subword_amd.soft_dtw_cuda import SoftDTW

assert torch.cuda.is_available(), "time_softdtw.py measures on the GPU: none found"
sdtw = SoftDTW(True, gamma=0.1)
g = torch.Generator().manual_seed(7)


def inputs(B, N, M, d=80):
    return torch.randn(B, N, d, generator=g).cuda(), torch.randn(B, M, d, generator=g).cuda()


def workload(name, X, Y, grad, **kw):
    if grad:
        X = X.clone().requires_grad_(True)

        def fn():
            X.grad = None
            sdtw(X, Y, **kw).sum().backward()
    else:
        def fn():
            with torch.no_grad():
                sdtw(X, Y, **kw)
    return name, fn


Xa, Ya = inputs(1, 800, 800)
Xb, Yb = inputs(1, 6000, 6000)
Xc, Yc = inputs(32, 800, 800)
xl = torch.randint(400, 801, (32,), generator=g).to(torch.int32).cuda()
yl = torch.randint(400, 801, (32,), generator=g).to(torch.int32).cuda()
work = [workload("B=1 800x800x80 forward (no grad)", Xa, Ya, False),
        workload("B=1 800x800x80 forward + backward", Xa, Ya, True),
        workload("B=1 6000x6000x80 forward (no grad)", Xb, Yb, False),
        workload("B=32 ragged 400-800 x80 forward (no grad)", Xc, Yc, False, x_lengths=xl, y_lengths=yl),
        workload("B=32 ragged 400-800 x80 forward + backward", Xc, Yc, True, x_lengths=xl, y_lengths=yl)]


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


times, iters = {name: [] for name, _ in work}, {}
for leg in range(a.legs):
    for name, fn in work:
        for _ in range(a.warmup):
            fn()
        if name not in iters:
            iters[name] = max(5, int(a.leg_ms / timed(fn, 3)) + 1)
        times[name].append(timed(fn, iters[name]))
for name, v in times.items():
    print(f"{name:46s} {iters[name]:5d} calls/leg  legs {' '.join(f'{x:9.3f}' for x in v)}  min {min(v):9.3f} ms  spread {max(v) - min(v):.3f} ms", flush=True)

if a.host_ref:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import softdtw_ref as S
    x, y = Xa[0].cpu().numpy(), Ya[0].cpu().numpy()
    t0 = time.perf_counter()
    D = S.sqdist(x, y)
    R = S.forward(D, 0.1)
    t1 = time.perf_counter()
    S.backward(D, R, 0.1)
    t2 = time.perf_counter()
    print(f"host fp64 restatement, 800x800x80: forward {1e3 * (t1 - t0):.1f} ms, backward {1e3 * (t2 - t1):.1f} ms "
          f"(value {R[800, 800]:.3f}, module {float(sdtw(Xa, Ya)[0]):.3f})", flush=True)
