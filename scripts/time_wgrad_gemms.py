"""Dev tool: t2_prof_gemm (ms_total = with the staging casts, ms_kernel = matrix kernel + split-K reduce alone) on the
weight-gradient shapes of one training iteration, operands k-major as the iteration holds them (A[k][m], B[k][n]: the
256-tile kernel's k-major variant).  With `kc`: also the same matrices K-contiguous (the K-contiguous variant) in the
same process, the comparison profiles/r04_wgrad_gemms.txt records."""
import ctypes as C, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tacotron2_subword_amd import _lib as L
L.set_precision("bf16")
shapes = [(4096, 3072, 25600), (4096, 1024, 25536), (4096, 512, 25536), (4096, 256, 25600), (1024, 512, 6400), (512, 1280, 6400),
          (256, 256, 25600), (1024, 256, 6336), (512, 2560, 6400)]
ws = torch.empty(200 << 20, device="cuda")


def prof(a):
    res = []
    for _ in range(3):
        t, k = C.c_float(), C.c_float()
        L.check(L.lib().t2_prof_gemm(C.byref(a), 10, C.byref(t), C.byref(k), L.stream()))
        res.append((round(t.value, 4), round(k.value, 4)))
    return res


for M, N, K in shapes:
    A = torch.randn(K, M, device="cuda"); B = torch.randn(K, N, device="cuda"); out = torch.empty(M, N, device="cuda")
    a = L.GemmArgs()
    for f, v in dict(A=L.ptr(A), B=L.ptr(B), C=L.ptr(out), M=M, N=N, K=K, batch=1, sam=1, sak=M, sbn=1, sbk=N, ldc=N, alpha=1.0, beta=0.0,
                     ws=L.ptr(ws), ws_bytes=ws.numel() * 4).items():
        setattr(a, f, v)
    print(f"M={M} N={N} K={K} k-major (ms_total, ms_kernel) x3: {prof(a)}", flush=True)
    if "kc" in sys.argv[1:]:
        At, Bt = A.t().contiguous(), B.t().contiguous()
        for f, v in dict(A=L.ptr(At), B=L.ptr(Bt), sam=K, sak=1, sbn=K, sbk=1).items():
            setattr(a, f, v)
        print(f"   K-contiguous (ms_total, ms_kernel) x3: {prof(a)}", flush=True)
L.set_precision("f32")
