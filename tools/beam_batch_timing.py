#!/usr/bin/env python3
"""The serial loop of `beam_search` over N images against ONE `beam_search_batch` of the same N.

    python tools/beam_batch_timing.py [--reps 20] [--out profiles/beam_batch_timing.txt]

gridTD (VGG16) at beam 2 / 50 steps and AoA at beam 3 / 20 steps - the searches `get_hidden_parameters` runs - for N = 1, 16, 32 seeded
images, encoded once outside the timed region.  The two sides alternate in one process after a warm-up of both; a time is host time
around a device synchronise, --reps >= 20 repetitions each: median (min .. max).  Random weights never emit <end>: every search runs all
its steps, the longest case.  The sequences of the two sides are compared before anything is timed.  Then one `image_ablation` of 64
rows (beam 3 / 20 steps, 4 images) against the same work done row by row (block_image, encode, `beam_search`, the teacher-forced
prefix, the picked probability), 5 repetitions each.  Without a GPU the file says that nothing was measured."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_batch_timing.txt"))
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20 repetitions each")
    sys.path.insert(0, ROOT)
    import torch
    import lrp_amd  # noqa: F401
    from lrp_amd import evaluation, weights
    lines = ["== serial beam_search over N images against one beam_search_batch of the same N"]

    def write():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if not torch.cuda.is_available():
        lines.append("nothing was measured: no GPU on this machine")
        print("\n".join(lines))
        write()
        return
    from lrp_amd.explainers import ablation
    from lrp_amd.explainers.aoa import AOAEngine
    from lrp_amd.explainers.beam import beam_search_batch
    from lrp_amd.explainers.gridtd import GridTDEngine
    lines[0] += f", {torch.cuda.get_device_name(0)}; host time around a device synchronise, median of {a.reps} (min .. max), the two sides alternating"

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def fmt(v):
        return f"{statistics.median(v):9.3f} ms ({min(v):.3f} .. {max(v):.3f})"

    def one(enc, i):
        e = {k: (v[i:i + 1].contiguous() if torch.is_tensor(v) else v) for k, v in enc.items()}
        e["B"] = 1
        return e

    grid = None
    for name, make, V, beam, steps in (("gridTD (VGG16)", lambda V: GridTDEngine(weights.make_gridtd_state(seed=0, vocab_size=V)), 9586, 2, 50),
                                       ("AoA (VGG16)", lambda V: AOAEngine(weights.make_aoa_state(seed=0, vocab_size=V)), 11027, 3, 20)):
        eng = make(V)
        wm = weights.make_word_map(V)
        start, end = wm['<start>'], wm['<end>']
        lines.append(f"  {name}, V = {V}, beam {beam} / {steps} steps")
        for N in (1, 16, 32):
            enc = eng.encode(torch.from_numpy(weights.make_images(100 + N, N)).cuda())
            singles = [one(enc, i) for i in range(N)]
            serial = lambda: [eng.beam_search(e, beam, steps, start, end) for e in singles]
            batch = lambda: beam_search_batch(eng, enc, beam, steps, start, end)
            assert serial() == batch(), "the two sides disagree"
            ts, tb = [], []
            for _ in range(a.reps):
                ts.append(timed(serial)[1])
                tb.append(timed(batch)[1])
            ms, mb = statistics.median(ts), statistics.median(tb)
            lines.append(f"    N = {N:2d}: serial {fmt(ts)}   batch {fmt(tb)}   serial / batch = {ms / mb:.2f}")
            print(lines[-1], flush=True)
        if grid is None:
            grid = (eng, wm)
        else:
            del eng
    # image ablation: 64 rows at once against the same rows one by one
    eng, wm = grid
    R = 64
    images = torch.from_numpy(weights.make_images(7, 4)).cuda()
    row2img = torch.arange(R) % 4
    spatial = torch.randn(R, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    special = [wm[k] for k in ('<start>', '<end>', '<unk>', '<pad>')]
    kw = dict(start_id=wm['<start>'], end_id=wm['<end>'], special_ids=special)
    caps = ablation.image_ablation(eng, images, row2img, spatial, [0] * R, **kw)[3]
    targets = [c[r % len(c)] for r, c in enumerate(caps)]          # every word is found: the teacher-forced half runs for all rows

    def per_row():
        out = []
        for r in range(R):
            masked = evaluation.block_image(spatial[r:r + 1])[:, None] * images[row2img[r]][None]
            enc = eng.encode(masked)
            seq = eng.beam_search(enc, 3, 20, wm['<start>'], wm['<end>'])
            sen = [w for w in seq if w not in special]
            k = sen.index(targets[r])
            cap = torch.tensor([[wm['<start>']] + sen[:k] + [0]], dtype=torch.int64, device="cuda")
            tr = eng.trace(enc, cap, model_bias=False, predictions=False)
            sc = eng.logits(tr["hc"].view(cap.shape[1] - 1, eng.H))[-1:]
            out.append(ablation.softmax_pick(eng, sc, torch.tensor([targets[r]])))
        return torch.cat(out)
    batched = lambda: ablation.image_ablation(eng, images, row2img, spatial, targets, **kw)[2]
    assert torch.equal(per_row(), batched()), "the two sides disagree"
    ts, tb = [], []
    for _ in range(5):
        ts.append(timed(per_row)[1])
        tb.append(timed(batched)[1])
    lines.append(f"  image_ablation, gridTD (VGG16), {R} rows of 4 images, beam 3 / 20 steps, median of 5")
    lines.append(f"    row by row {fmt(ts)}   image_ablation {fmt(tb)}   ratio = {statistics.median(ts) / statistics.median(tb):.2f}")
    print("\n".join(lines))
    write()


if __name__ == "__main__":
    main()
