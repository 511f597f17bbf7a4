#!/usr/bin/env python3
"""Phase times of the single-LSTM adaptive-attention explainer (`AdaAttEngine`) next to `GridTDEngine` on the same box,
in the same process, at the same B, T and vocabulary.

    python tools/adaatt_timing.py [--iters 9] [--vocab 9586] [--out profiles/adaatt_timing.txt]

Two set-ups: B = 16, T = 20 with the VGG16 encoder (phases encode, trace, relevance, chain of `explain_batch`), and B = 32, T = 20 on
(B, 196, 512) features (the decoder alone: trace and relevance; gridTD's decoder runs on the same features, taken from its encoder).
HIP-event times, median of --iters >= 5 (min .. max) after two warm-up steps; the two engines alternate step by step, so a drift of the
clocks hits both.  Also the A/B of `cut_dead_columns` (relevance phase) and of the decoupled against the per-step trace, alternating
likewise.  No ratio is asserted.  Without a GPU the file says that nothing was measured."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--vocab", type=int, default=9586)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaatt_timing.txt"))
    a = ap.parse_args()
    if a.iters < 5:
        raise SystemExit("--iters: the median of at least 5 runs")
    sys.path.insert(0, ROOT)
    import torch
    import lrp_amd  # noqa: F401
    from lrp_amd import weights
    V, T = a.vocab, 20
    lines = []

    def write():
        with open(a.out, "w") as f:
            f.write("\n".join(lines).rstrip("\n") + "\n")
        print("\n".join(lines))

    if not torch.cuda.is_available():
        lines.append("== AdaAttEngine next to GridTDEngine: nothing was measured: no GPU on this machine")
        write()
        return
    from lrp_amd.explainers.adaatt import AdaAttEngine
    from lrp_amd.explainers.gridtd import GridTDEngine
    lines.append(f"== AdaAttEngine next to GridTDEngine, T = {T}, V = {V}, {torch.cuda.get_device_name(0)}, HIP events, ms, median of {a.iters} "
                 "(min .. max) after two warm-up steps, engines alternating")
    ada = AdaAttEngine(weights.make_adaatt_state(seed=0, vocab_size=V))
    grid = GridTDEngine(weights.make_gridtd_state(seed=0, vocab_size=V))
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def phases(fns):
        """fns: [(name, callable)] run in order; -> {name: ms}"""
        marks = [ev()]
        marks[0].record()
        for _, fn in fns:
            fn()
            marks.append(ev())
            marks[-1].record()
        torch.cuda.synchronize()
        return {n: marks[i].elapsed_time(marks[i + 1]) for i, (n, _) in enumerate(fns)}

    def fmt(xs):
        return "%.3f (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))

    def compare(title, steps):
        """steps: {label: callable -> {phase: ms}}; alternating, warm-up 2"""
        acc = {k: {} for k in steps}
        for it in range(a.iters + 2):
            for k, step in steps.items():
                r = step()
                if it >= 2:
                    for n, v in r.items():
                        acc[k].setdefault(n, []).append(v)
        lines.append(title)
        for k, d in acc.items():
            tot = [sum(v[i] for v in d.values()) for i in range(a.iters)]
            lines.append("  %-28s " % k + "  ".join("%s %s" % (n, fmt(v)) for n, v in d.items()) + ("  | sum %s" % fmt(tot) if len(d) > 1 else ""))

    def full_step(eng, images, caps):
        st = {}

        def run():
            return phases([("encode", lambda: st.__setitem__("enc", eng.encode(images))),
                           ("trace", lambda: st.__setitem__("tr", eng.trace(st["enc"], caps, predictions=False))),
                           ("relevance", lambda: st.__setitem__("rel", eng.relevance(st["enc"], st["tr"]))),
                           ("chain", lambda: eng.cnn.relevance(st["rel"][0], st["rel"][2]))])
        return run

    def decoder_step(eng, enc, caps):
        st = {}

        def run():
            return phases([("trace", lambda: st.__setitem__("tr", eng.trace(enc, caps, predictions=False))),
                           ("relevance", lambda: st.__setitem__("rel", eng.relevance(enc, st["tr"])))])
        return run

    # ---- B = 16 with the VGG16 encoder
    B = 16
    images = torch.from_numpy(weights.make_images(100, B)).cuda()
    caps = torch.from_numpy(weights.make_captions(200, B, T, V)).cuda()
    compare(f"-- B = {B}, VGG16 encoder, 224 x 224: the phases of explain_batch",
            {"AdaAttEngine": full_step(ada, images, caps), "GridTDEngine": full_step(grid, images, caps)})
    # ---- B = 32 on features: the decoders alone
    B = 32
    images = torch.from_numpy(weights.make_images(101, B)).cuda()
    caps = torch.from_numpy(weights.make_captions(201, B, T, V)).cuda()
    genc = grid.encode(images)
    feats = genc["feats"].clone()
    aenc = ada.encode(features=feats)
    compare(f"-- B = {B} on (B, 196, 512) features: the decoders alone",
            {"AdaAttEngine": decoder_step(ada, aenc, caps), "GridTDEngine (its decoder)": decoder_step(grid, genc, caps)})

    # ---- A/B: dead columns of the gate rule, decoupled against per-step trace
    tr = ada.trace(aenc, caps, predictions=False)

    def rel(cut):
        def run():
            ada.cut_dead_columns = cut
            try:
                return phases([("relevance", lambda: ada.relevance(aenc, tr))])
            finally:
                ada.cut_dead_columns = True
        return run

    def trace(decoupled):
        def run():
            ada.decoupled = decoupled
            try:
                return phases([("trace", lambda: ada.trace(aenc, caps, predictions=False))])
            finally:
                ada.decoupled = True
        return run
    compare(f"-- A/B at B = {B}: cut_dead_columns (the gate rule of lock-steps s >= 1 at N = H + E instead of H + 2E)",
            {"cut_dead_columns = True": rel(True), "cut_dead_columns = False": rel(False)})
    compare(f"-- A/B at B = {B}: the teacher-forced trace", {"decoupled (1 serial launch / step)": trace(True), "per step (5 launches / step)": trace(False)})
    write()


if __name__ == "__main__":
    main()
