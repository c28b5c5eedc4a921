"""Dev tool: the end of backward in a rocprofv3 kernel trace (csv), last iteration: the span from the end of the
decoder's attention backward chain (chain_bwd_att_kernel) to the gradient norm (sumsq_kernel).  Prints its wall and
GPU-busy time, every enc_chain_bwd_kernel with its duration, and which kernels of OTHER streams start inside the span of
each encoder chain and of the encoders' conv/BN backward (first to last conv_bn kernel), i.e. what actually overlaps.
usage: tail_timeline.py <kernel_trace.csv> [which_iteration_from_the_end=1]"""
import csv, sys
from collections import Counter

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Stream_Id", "?")))
rows.sort()
which = int(sys.argv[2]) if len(sys.argv) > 2 else 1


def short(k):
    k = k.replace("void ", "").replace("t2::(anonymous namespace)::", "").replace("t2::", "")
    return k.split("(")[0][:60]


att = [r for r in rows if "chain_bwd_att_kernel" in r[2]]
sums = [r for r in rows if "sumsq_kernel" in r[2]]
a = att[-which]
t0 = a[1]
t1 = min(r[0] for r in sums if r[0] > t0)
span = [r for r in rows if r[0] >= t0 and r[0] < t1]
busy, end = 0, t0
for s, e, k, st in span:
    e = min(e, t1)
    if s > end:
        busy += e - s
    elif e > end:
        busy += e - end
    end = max(end, e)
print(f"chain_bwd_att_kernel: {1e-6 * (a[1] - a[0]):.3f} ms on stream {a[3]}")
print(f"end of chain_bwd_att_kernel -> first sumsq_kernel: {1e-6 * (t1 - t0):.3f} ms wall, {1e-6 * busy:.3f} ms busy, {len(span)} kernels, "
      f"sum of kernel times {1e-6 * sum(e - s for s, e, _, _ in span):.3f} ms")
by = Counter()
for s, e, k, st in span:
    by[st] += e - s
print("kernel time by stream:", {st: f"{1e-6 * t:.3f} ms" for st, t in sorted(by.items(), key=lambda kv: -kv[1])})
km = Counter()                                            # the K = B*T weight-gradient GEMMs (k-major 256-tile kernel) by stream
for s, e, k, st in span:
    if "gemm_bf16src256_kernel<false, true" in k:
        km[st] += e - s
tail_stream = max(km, key=km.get) if km else None
print("weight-gradient tail on stream", tail_stream, "(the chain's own stream)" if tail_stream == a[3] else "(a side stream)")
if tail_stream is not None and tail_stream != a[3]:
    ts = [r for r in span if r[3] == tail_stream]
    print(f"  its kernels in the span: first start +{1e-6 * (ts[0][0] - t0):.3f} ms, last end +{1e-6 * (max(r[1] for r in ts) - t0):.3f} ms")


def inside(lo, hi, own):
    c = Counter()
    for s, e, k, st in span:
        if lo <= s < hi and st != own:
            c[(st, short(k))] += 1
    return c


for r in [r for r in span if "enc_chain_bwd_kernel" in r[2]]:
    c = inside(r[0], r[1], r[3])
    print(f"enc_chain_bwd_kernel on stream {r[3]}: start +{1e-6 * (r[0] - t0):.3f} ms, {1e-6 * (r[1] - r[0]):.3f} ms; kernels of other streams starting inside: {sum(c.values())}")
    for (st, k), n in sorted(c.items(), key=lambda kv: -kv[1])[:12]:
        print(f"    {n:3d} x [stream {st}] {k}")
conv = [r for r in span if "conv_bn" in r[2] or "bn_" in r[2]]
if conv:
    lo, hi = conv[0][0], max(r[1] for r in conv)
    streams = {r[3] for r in conv}
    c = Counter()
    for s, e, k, st in span:
        if lo <= s < hi and st not in streams:
            c[(st, short(k))] += 1
    print(f"encoders' conv/BN backward: +{1e-6 * (lo - t0):.3f} .. +{1e-6 * (hi - t0):.3f} ms on streams {sorted(streams)}; kernels of other streams starting inside: {sum(c.values())}")
    for (st, k), n in sorted(c.items(), key=lambda kv: -kv[1])[:12]:
        print(f"    {n:3d} x [stream {st}] {k}")
