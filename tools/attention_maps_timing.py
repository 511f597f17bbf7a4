#!/usr/bin/env python3
"""`ops.expand_maps` against the composition the library offered before it had the entry: torch head mean +
`ops.guided_gradcam(ones, .)` + `evaluation.project_maxabs`.

    python tools/attention_maps_timing.py [--reps 20] [--out profiles/attention_maps_timing.txt]

320 normalised attention maps at p = 14 -> 224 x 224 (a batch of 16 captions of 20 words): single-head rows (gridTD / AdaAtt) and 8-head
rows reduced to their mean (AoA).  The two sides alternate in one process after a warm-up of both; a time is host time of one call around a
device synchronise and, second, HIP events around 10 calls enqueued back to back (the new entry writing into one preallocated result),
--reps >= 20 repetitions each: median (min .. max).  The outputs of the two sides are compared before anything is timed
(single head: the same bits; the mean: torch's mean is another summation, within 1e-5 of the map's peak).  Bytes per second: the one write of
the (rows, 224, 224) fp32 result - the entry reads 196 values per map - over the median event time.  Without a GPU the file says that nothing was
measured."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=320)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_maps_timing.txt"))
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20 repetitions each")
    sys.path.insert(0, ROOT)
    import torch
    import lrp_amd  # noqa: F401
    from lrp_amd import evaluation, ops
    lines = ["== ops.expand_maps against head mean + guided_gradcam(ones, .) + project_maxabs"]

    def write():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if not torch.cuda.is_available():
        lines.append("nothing was measured: no GPU on this machine")
        print("\n".join(lines))
        write()
        return
    lines[0] += f", {torch.cuda.get_device_name(0)}; host time around a device synchronise, median of {a.reps} (min .. max), the two sides alternating"

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def events(fn, n=10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def fmt(v):
        return f"{statistics.median(v):8.3f} ms ({min(v):.3f} .. {max(v):.3f})"

    R, p, hw = a.rows, 14, 224
    gen = torch.Generator().manual_seed(0)
    ones = torch.ones(R, 1, hw, hw, device="cuda")
    for name, heads in (("single-head rows", 1), ("8-head rows, mean over the heads", 8)):
        alpha = torch.softmax(torch.randn(R, heads, p * p, generator=gen) * 3.0, dim=-1).cuda()
        if heads == 1:
            alpha = alpha[:, 0].contiguous()
        new = lambda: ops.expand_maps(alpha, hw, normalize=True)
        old = lambda: evaluation.project_maxabs(ops.guided_gradcam(ones, alpha if heads == 1 else alpha.mean(dim=1), p)[:, 0])
        x, y = new(), old()
        d = (x - y).abs().max().item()
        assert (d == 0.0) if heads == 1 else (d <= 1e-5), "the two sides disagree: %g" % d
        for _ in range(3):
            new(); old()
        tn, to = [], []
        for _ in range(a.reps):
            tn.append(timed(new)[1])
            to.append(timed(old)[1])
        mn, mo = statistics.median(tn), statistics.median(to)
        # device time: HIP events around 10 calls enqueued back to back, the result buffer of the new entry allocated once
        out = torch.empty(R, hw, hw, device="cuda")
        new_into = lambda: ops.expand_maps(alpha, hw, normalize=True, out=out)
        dn, do = [], []
        for _ in range(a.reps):
            dn.append(events(new_into))
            do.append(events(old))
        en = statistics.median(dn)
        out_bytes = R * hw * hw * 4
        lines.append(f"  {name}: {R} maps, p = {p} -> {hw} x {hw}, {out_bytes / 1e6:.1f} MB written; the two sides differ by {d:.1e}")
        lines.append(f"    one call, host time:       expand_maps {fmt(tn)}   composition {fmt(to)}   composition / expand_maps = {mo / mn:.2f}")
        lines.append(f"    10 calls, HIP events / 10: expand_maps {fmt(dn)}   composition {fmt(do)}   composition / expand_maps = {statistics.median(do) / en:.2f}")
        lines.append(f"    expand_maps writes {out_bytes / (en * 1e-3) / 1e9:.0f} GB/s by the event time ({out_bytes / (mn * 1e-3) / 1e9:.0f} GB/s by the host time of one call, "
                     "allocation of the result and the synchronise included)")
        print("\n".join(lines[-4:]), flush=True)
    write()


if __name__ == "__main__":
    main()
