#!/usr/bin/env python3
"""Phase times of the gradient family of the single-LSTM adaptive-attention model (`AdaAttGradEngine`) next to
`GridTDEngine.guided_gradient` on the same box, in the same process, at the same B, T and vocabulary.

    python tools/adaatt_grad_timing.py [--iters 9] [--vocab 9586] [--out profiles/adaatt_grad_timing.txt]

Two set-ups at T = 20: B = 16 with the VGG16 encoder (phases trace(grad=True), decoder back-pass, encoder chain = `vgg.gradient` on the
B*T maps), and B = 32 on (B, 196, 512) features (trace and decoder back-pass; gridTD's decoder runs on the same features, taken from its
encoder).  HIP-event times, median of --iters >= 5 (min .. max) after two warm-up steps; the two engines alternate step by step, so a
drift of the clocks hits both.  The decoder back-pass is also given per LSTM cell of the model (this model has one, gridTD two).  No
ratio is asserted.  Without a GPU the file says that nothing was measured."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = {"AdaAttGradEngine": 1, "GridTDEngine": 2}           # LSTM cells per decoder step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--vocab", type=int, default=9586)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaatt_grad_timing.txt"))
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
        lines.append("== AdaAttGradEngine next to GridTDEngine.guided_gradient: nothing was measured: no GPU on this machine")
        write()
        return
    from lrp_amd.explainers.adaatt_grad import AdaAttGradEngine
    from lrp_amd.explainers.gridtd import GridTDEngine
    lines.append(f"== AdaAttGradEngine next to GridTDEngine (gradient family), T = {T}, V = {V}, {torch.cuda.get_device_name(0)}, HIP events, ms, "
                 f"median of {a.iters} (min .. max) after two warm-up steps, engines alternating")
    ada = AdaAttGradEngine(weights.make_adaatt_state(seed=0, vocab_size=V))
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
        """steps: {engine name: callable -> {phase: ms}}; alternating, warm-up 2"""
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
            lines.append("  %-18s " % k + "  ".join("%s %s" % (n, fmt(v)) for n, v in d.items()) + "  | sum %s" % fmt(tot))
        for k, d in acc.items():
            lines.append("  %-18s decoder back-pass per LSTM cell (%d): %s" % (k, CELLS[k], fmt([v / CELLS[k] for v in d["back-pass"]])))

    def step(eng, enc, caps, chain):
        st = {}

        def run():
            fns = [("trace", lambda: st.__setitem__("tr", eng.trace(enc, caps, predictions=False, grad=True))),
                   ("back-pass", lambda: st.__setitem__("g", eng.guided_gradient(enc, st["tr"], mask_features=False)))]
            if chain:
                fns.append(("chain", lambda: eng.vgg.gradient(st["g"][0], st["g"][2])))
            return phases(fns)
        return run

    # ---- B = 16 with the VGG16 encoder
    B = 16
    images = torch.from_numpy(weights.make_images(100, B)).cuda()
    caps = torch.from_numpy(weights.make_captions(200, B, T, V)).cuda()
    compare(f"-- B = {B}, VGG16 encoder, 224 x 224: trace(grad=True), decoder back-pass, vgg.gradient on the {B * T} maps",
            {"AdaAttGradEngine": step(ada, ada.encode(images), caps, True), "GridTDEngine": step(grid, grid.encode(images), caps, True)})
    # ---- B = 32 on features: the decoders alone
    B = 32
    images = torch.from_numpy(weights.make_images(101, B)).cuda()
    caps = torch.from_numpy(weights.make_captions(201, B, T, V)).cuda()
    genc = grid.encode(images)
    aenc = ada.encode(features=genc["feats"].clone())
    compare(f"-- B = {B} on (B, 196, 512) features: the decoders alone",
            {"AdaAttGradEngine": step(ada, aenc, caps, False), "GridTDEngine": step(grid, genc, caps, False)})
    write()


if __name__ == "__main__":
    main()
