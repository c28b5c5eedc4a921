"""Dev tool: the B=64 / 100 / 60 / 400 synthetic training iteration of scripts/phase_times.py and the B=128 no-grad
forward (the GTA workload) in several precision modes, ALTERNATING in one process (f32, bf16x3, f32, bf16x3, ...): per
leg a warm-up and then --iters timed iterations ending in a synchronise; per mode the gemm_counts of one iteration.

  python scripts/time_precision_modes.py [--modes f32,bf16x3] [--legs 2] [--iters 5] [--lib PATH] [--tree DIR]

A mode written "bf16x3@N" runs bf16x3 with the dispatch threshold of the split path at N MFLOP instead of the default
(--modes f32,bf16x3,bf16x3@0 compares threshold on and off in one run).  "bf16x3+steps" runs bf16x3 with the split-bf16
recurrent steps on (t2_set_split_steps; --modes bf16x3,bf16x3+steps compares switch off and on); per mode the step_counts
of one iteration are printed next to the gemm_counts.
--lib PATH (or T2AMD_LIB, as scripts/build_variant.sh uses it): another build of the library with the same ABI.
--tree DIR: import the package from another checkout (with its own library) instead — a library of an older ABI version
does not load under this binding, so the legs of an older commit run from that commit's tree, in a process of their own."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="f32,bf16x3")
ap.add_argument("--legs", type=int, default=2)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--lib", default=None)
ap.add_argument("--tree", default=None)
ap.add_argument("--skip-gta", action="store_true")
a = ap.parse_args()
if a.lib:
    os.environ["T2AMD_LIB"] = os.path.abspath(a.lib)
sys.path.insert(0, os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tacotron2_subword_amd import _lib as L
from tacotron2_subword_amd.hparams import create_hparams
from tacotron2_subword_amd import train as T

modes = a.modes.split(",")         # "bf16x3@0": mode bf16x3 with the dispatch threshold set to 0 MFLOP (every qualifying product split)


def set_mode(m):
    name, _, thr = m.partition("@")
    name, plus, steps = name.partition("+")
    assert not plus or steps == "steps", m
    L.set_precision(name)
    if hasattr(L, "set_split_steps"):
        L.set_split_steps(bool(plus))
    else:
        assert not plus, "this library has no split-steps switch"
    if hasattr(L, "set_gemm_split_min_mflop"):
        L.set_gemm_split_min_mflop(int(thr) if thr else -1)


hp = create_hparams()
model, optimizer, criterion = T.make_training_objects(hp)
print(f"library {L.LIB_PATH} ABI {L.lib().t2_version()}  modes {modes}  legs {a.legs} x {a.iters} iterations", flush=True)
counts = getattr(L, "gemm_counts", None)
step_counts = getattr(L, "step_counts", None)


def timed(fn, label):
    per_mode = {m: [] for m in modes}
    for leg in range(a.legs):
        for m in modes:
            set_mode(m)
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            if counts and leg == 0:
                counts(reset=True); fn(); torch.cuda.synchronize()
                print(f"{label} {m:12s} gemm_counts of one iteration (exact, converting, single-bf16 source, split source): {counts(reset=True)}", flush=True)
            if step_counts and leg == 0:
                step_counts(reset=True); fn(); torch.cuda.synchronize()
                print(f"{label} {m:12s} step_counts of one iteration (forward exact, bf16, split; gradient exact, bf16, split): {step_counts(reset=True)}", flush=True)
            t0 = time.perf_counter()
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / a.iters * 1e3
            per_mode[m].append(ms)
            print(f"{label} leg {leg} {m:12s} {ms:8.2f} ms / iteration", flush=True)
    for m in modes:
        v = per_mode[m]
        print(f"{label} {m:12s} legs {' '.join(f'{x:.2f}' for x in v)}  min {min(v):.2f}  max {max(v):.2f}  spread {max(v) - min(v):.2f} ms", flush=True)
    set_mode("f32")


model.train()
x, y = model.parse_batch(T.synthetic_batch(hp, 64, 100, 60, 400, seed=1234))
it = [0]
def train_iter():
    T.train_step(model, criterion, optimizer, x, y, hp, it[0]); it[0] += 1
timed(train_iter, "train B=64 T=400")

if not a.skip_gta:
    model.eval()
    xg, _ = model.parse_batch(T.synthetic_batch(hp, 128, 100, 60, 400, seed=4321))
    def gta():
        with torch.no_grad():
            model(xg)
    timed(gta, "forward B=128 T=400 (no grad)")
