"""Experiment (test infrastructure, not collected by pytest): what does the split-bf16 precision mode ("bf16x3") cost in
accuracy?  The oracle is re-run with EVERY F.linear / F.conv1d whose three extents (rows, outputs, reduction length) are
all >= 64 replaced by the 3-term split (x = hi + lo with hi = RN-bf16(x), lo = RN-bf16(x - hi), both operands split;
x.w ~ hi.hi + lo.hi + hi.lo, fp32 accumulation), eval forward, against the unmodified fp32 oracle.
   python tests/tools/split_bf16_gemm_accuracy.py [B Tin Tsub T] [--terms 1|3] [--only linear|conv]"""
import os, sys
import torch
import torch.nn.functional as F
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
from oracle import recipe
from oracle import tacotron2_oracle as O

args = [a for a in sys.argv[1:] if not a.startswith("--")]
terms = 1 if "--terms" in sys.argv and sys.argv[sys.argv.index("--terms") + 1] == "1" else 3
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
shapes = [tuple(int(v) for v in args[:4])] if len(args) >= 4 else [(2, 100, 60, 400), (8, 100, 60, 200), (8, 96, 64, 128), (4, 64, 32, 256)]


def parts(x):
    hi = x.to(torch.bfloat16).to(torch.float32)
    return hi, (x - hi).to(torch.bfloat16).to(torch.float32)


class SplitF:
    """torch.nn.functional with linear / conv1d on split operands where the product is large."""
    def __getattr__(self, name):
        return getattr(F, name)

    def linear(self, x, w, b=None):
        rows = x.numel() // x.shape[-1]
        if only == "conv" or min(rows, w.shape[0], w.shape[1]) < 64:
            return F.linear(x, w, b)
        (xh, xl), (wh, wl) = parts(x), parts(w)
        y = F.linear(xh, wh) if terms == 1 else F.linear(xh, wh) + F.linear(xl, wh) + F.linear(xh, wl)
        return y if b is None else y + b

    def conv1d(self, x, w, b=None, padding=0, groups=1):
        if only == "linear" or groups != 1 or min(x.shape[0] * x.shape[2], w.shape[0], w.shape[1] * w.shape[2]) < 64:
            return F.conv1d(x, w, b, padding=padding, groups=groups)
        (xh, xl), (wh, wl) = parts(x), parts(w)
        c = lambda a, k: F.conv1d(a, k, None, padding=padding)
        y = c(xh, wh) if terms == 1 else c(xh, wh) + c(xl, wh) + c(xh, wl)
        return y if b is None else y + b[None, :, None]


hp = O.default_hparams()
P = recipe.make_weights(hp)
names = ("mel", "mel_postnet", "gate", "align", "align_bert")
for B, Tin, Tsub, T in shapes:
    x, _ = recipe.parse_batch(recipe.make_batch(hp, B, Tin, Tsub, T))
    with torch.no_grad():
        ref = O.forward(P, hp, x, training=False)
        O.F = SplitF()
        try:
            out = O.forward(P, hp, x, training=False)
        finally:
            O.F = F
    errs = {n: float((a - b).abs().max()) for n, a, b in zip(names, out, ref)}
    print(f"B={B} Tin={Tin} Tsub={Tsub} T={T} terms={terms} only={only}: " + "  ".join(f"{k} {v:.1e}" for k, v in errs.items()), flush=True)
