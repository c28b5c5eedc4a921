"""Dev tool: TFLOP/s of the GEMM kernels on the shapes of one training iteration (fp32 vs bf16 vs split-bf16 operands).
--modes picks the modes (a library older than the split-bf16 mode knows f32,bf16 only); T2AMD_LIB / --tree as in
scripts/time_precision_modes.py."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="f32,bf16,bf16x3")
ap.add_argument("--tree", default=None)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tacotron2_subword_amd import _lib as L, ops
shapes = [("PRED fwd NT", 25600, 4096, 3072, False, True), ("dDIN NN", 25600, 3072, 4096, False, False),
          ("dW_dec_ih TN", 4096, 3072, 25600, True, False), ("dW_att_hh TN", 4096, 1024, 25600, True, False),
          ("PREA fwd NT", 25600, 4096, 256, False, True), ("postnet conv NT-like", 25600, 512, 2560, False, True),
          ("dWq TN", 128, 1024, 25600, True, False),
          ("PRED chunk NT", 3200, 4096, 3072, False, True), ("dDIN chunk NN", 3200, 3072, 4096, False, False),
          ("dW_att_ctx TN", 4096, 512, 25600, True, False)]
ws = torch.empty(448 << 20, device="cuda")        # split-bf16 stages 6 bytes per operand element: 1.1 GB for dW_dec_ih
counts = getattr(L, "gemm_counts", None)
for name, M, N, K, ta, tb in shapes:
    A = torch.randn((K, M) if ta else (M, K), device="cuda")
    B = torch.randn((N, K) if tb else (K, N), device="cuda")
    out = torch.empty(M, N, device="cuda")
    ref = None
    for mode in a.modes.split(","):
        L.set_precision(mode)
        for _ in range(2):
            ops.gemm(A, B, trans_a=ta, trans_b=tb, out=out, ws=ws)
        if counts:
            counts(reset=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        n = 5
        for _ in range(n):
            ops.gemm(A, B, trans_a=ta, trans_b=tb, out=out, ws=ws)
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / n
        route = ""
        if counts:
            c = counts(reset=True)
            route = " route=" + ("exact", "converting", "src", "split")[max(range(4), key=lambda i: c[i])]
        note = ""
        if mode == "f32":
            ref = out.clone()
        elif ref is not None:
            aerr = (out - ref).abs().max().item()
            err = aerr / ref.abs().max().item()
            note = f"  max |d| vs f32 {aerr:.3e} (rel {err:.2e}; sqrt(K)*2^-17 = {K ** 0.5 * 2.0 ** -17:.3e})"
            if mode == "bf16":
                assert err < 2e-2, (name, err)
            else:       # split scheme <= 8 sqrt(K) 2^-17 from the exact product, the f32 kernel an eighth of that at most
                assert aerr <= 9 * K ** 0.5 * 2.0 ** -17, (name, aerr)
        print(f"{name:24s} {mode:6s} M={M} N={N} K={K}: {dt*1e3:7.3f} ms  {2*M*N*K/dt/1e12:7.1f} TFLOP/s{route}{note}", flush=True)
L.set_precision("f32")
