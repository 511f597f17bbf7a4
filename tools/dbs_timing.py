#!/usr/bin/env python3
"""One `diverse_beam_search_batch` of N images against N calls of one image each, and `beam_search_batch` at the same number of decoder
rows as the yardstick for what a step of that many rows costs.

    python tools/dbs_timing.py [--reps 20] [--out profiles/dbs_timing.txt]

gridTD (VGG16) at beam 3 / 50 steps and AoA at beam 3 / 20 steps for N = 1, 7, 16 seeded images, encoded once outside the timed region;
the beam search runs on 3 N images, which are the same 9 N rows.  The sides alternate in one process after a warm-up of all; a time is
host time around a device synchronise, --reps >= 20 repetitions each: median (min .. max).  Random weights never emit <end>: every search
runs all its steps, the longest case.  The results of the batched and the one-by-one side are compared before anything is timed.  The
selection kernels' share of a search is the sum of their launches between two device events each, in a separate pass.  Without a GPU the
file says that nothing was measured."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbs_timing.txt"))
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20 repetitions each")
    sys.path.insert(0, ROOT)
    import torch
    import lrp_amd  # noqa: F401
    from lrp_amd import _lib, weights
    lines = ["== one diverse_beam_search_batch of N images against N calls of one image; beam_search_batch at the same rows"]

    def write():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if not torch.cuda.is_available():
        lines.append("nothing was measured: no GPU on this machine")
        print("\n".join(lines))
        write()
        return
    from lrp_amd.explainers.aoa import AOAEngine
    from lrp_amd.explainers.beam import beam_search_batch, diverse_beam_search_batch
    from lrp_amd.explainers.gridtd import GridTDEngine
    lines[0] += f", {torch.cuda.get_device_name(0)}; host time around a device synchronise, median of {a.reps} (min .. max), the sides alternating"
    lib = _lib.load()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def fmt(v):
        return f"{statistics.median(v):8.3f} ms ({min(v):.3f} .. {max(v):.3f})"

    def pick(enc, idx):
        e = {k: (v[idx].contiguous() if torch.is_tensor(v) else v) for k, v in enc.items()}
        e["B"] = len(idx)
        return e

    def kernel_ms(symbol, fn):
        """device time of the launches of `symbol` during fn(), each between two events"""
        real, events = getattr(lib, symbol), []

        def spy(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = real(*args)
            e1.record()
            events.append((e0, e1))
            return rc
        setattr(lib, symbol, spy)
        try:
            fn()
        finally:
            setattr(lib, symbol, real)
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in events), len(events)

    for name, make, V, beam, steps in (("gridTD (VGG16)", lambda V: GridTDEngine(weights.make_gridtd_state(seed=0, vocab_size=V)), 9586, 3, 50),
                                       ("AoA (VGG16)", lambda V: AOAEngine(weights.make_aoa_state(seed=0, vocab_size=V)), 11027, 3, 20)):
        eng = make(V)
        wm = weights.make_word_map(V)
        start, end = wm['<start>'], wm['<end>']
        lines.append(f"  {name}, V = {V}, beam {beam} ({beam} groups) / {steps} steps")
        for N in (1, 7, 16):
            enc = eng.encode(torch.from_numpy(weights.make_images(100 + N, N)).cuda())
            wide = pick(enc, [i % N for i in range(beam * N)])              # beam N images: the same beam^2 N rows for the beam search
            singles = [pick(enc, [i]) for i in range(N)]
            serial = lambda: [diverse_beam_search_batch(eng, e, beam, steps, start, end)[0] for e in singles]
            batch = lambda: diverse_beam_search_batch(eng, enc, beam, steps, start, end)
            plain = lambda: beam_search_batch(eng, wide, beam, steps, start, end)
            assert serial() == batch(), "the two sides disagree"
            plain()
            ts, tb, tp = [], [], []
            for _ in range(a.reps):
                ts.append(timed(serial)[1])
                tb.append(timed(batch)[1])
                tp.append(timed(plain)[1])
            ms, mb, mp = statistics.median(ts), statistics.median(tb), statistics.median(tp)
            kd, nd = kernel_ms("lrpx_dbs_step_batch", batch)
            kp, npl = kernel_ms("lrpx_beam_step_batch", plain)
            lines.append(f"    N = {N:2d} ({beam * beam * N:3d} rows): one by one {fmt(ts)}   batch {fmt(tb)}   one by one / batch = {ms / mb:.2f}")
            lines.append(f"             beam_search_batch of {beam * N} images {fmt(tp)}   diverse / beam = {mb / mp:.2f}")
            lines.append(f"             selection kernel: diverse {kd / nd * 1e3:7.1f} us per step ({kd / mb * 100:.1f} % of the search), "
                         f"beam {kp / npl * 1e3:7.1f} us per step ({kp / mp * 100:.1f} %)")
            print("\n".join(lines[-3:]), flush=True)
        del eng
    write()


if __name__ == "__main__":
    main()
