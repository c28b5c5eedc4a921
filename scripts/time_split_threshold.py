"""Dev tool: where does the split-bf16 GEMM path ("bf16x3") start to pay?  Small and medium products, exact fp32 kernel
against the split path with the dispatch threshold lifted (set_gemm_split_min_mflop(0)), alternating, two legs of 200
calls each.  The default threshold (2*M*N*K >= 2^31 FLOP) comes from this table: profiles/r05_split_threshold.txt."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tacotron2_subword_amd import _lib as L, ops
ws = torch.empty(64 << 20, device="cuda")
shapes = [(256, 256, 128, False, True), (256, 256, 128, True, False), (256, 384, 192, False, True), (1024, 640, 64, False, True),
          (512, 512, 320, False, True), (512, 256, 4096, False, True), (768, 256, 4160, True, False), (1536, 1024, 512, False, True),
          (1024, 256, 3776, True, False), (1024, 256, 6336, True, False), (2048, 512, 2560, False, True), (3840, 1024, 512, False, True),
          (1024, 512, 6400, True, False)]
L.set_gemm_split_min_mflop(0)
try:
    for M, N, K, ta, tb in shapes:
        A = torch.randn((K, M) if ta else (M, K), device="cuda"); B = torch.randn((N, K) if tb else (K, N), device="cuda")
        out = torch.empty(M, N, device="cuda")
        res = {}
        for leg in range(2):
            for mode in ("f32", "bf16x3"):
                L.set_precision(mode)
                for _ in range(5):
                    ops.gemm(A, B, trans_a=ta, trans_b=tb, out=out, ws=ws)
                L.gemm_counts(reset=True)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(200):
                    ops.gemm(A, B, trans_a=ta, trans_b=tb, out=out, ws=ws)
                torch.cuda.synchronize(); res.setdefault(mode, []).append((time.perf_counter() - t0) / 200 * 1e6)
                assert L.gemm_counts()[3] == (200 if mode == "bf16x3" else 0)
        f, x = res["f32"], res["bf16x3"]
        print(f"M={M:5d} N={N:5d} K={K:5d} {'A[k][m]' if ta else 'A[m][k]'} {'B[n][k]' if tb else 'B[k][n]'} {2e-9 * M * N * K:6.2f} GFLOP: "
              f"f32 {f[0]:6.1f} / {f[1]:6.1f} us   bf16x3 {x[0]:6.1f} / {x[1]:6.1f} us   {'split faster' if max(x) < min(f) else 'exact faster' if max(f) < min(x) else 'even'}", flush=True)
finally:
    L.set_precision("f32"); L.set_gemm_split_min_mflop(-1)
