#!/usr/bin/env python3
"""Phase times of the bottom-up gridTD explainer (`GridTDBUEngine`): B images of 36 x 2048 region features x T words.

    python tools/gridtd_bu_timing.py [B [T]] [--iters 7] [--vocab 9586] [--out profiles/gridtd_bu_timing.txt]

Prints the host arithmetic of the sizes (memory per map), warms up, then takes HIP-event times (median of --iters >= 5, with min ..
max) of the phases of `explain_batch` - `encode` (projector, mean, global feature, attention constants), the decoder trace, the T
lock-steps of the decoder relevance, the tail (global rule -> r_avg, the pixel rule with the mean term) and the projector rule - and of
the whole step, eager and as a recorded step.  Beside it, for orientation, `AOAEngine`'s bottom-up step (`features=`, head 0) of the same
B, T and vocabulary from the same process.  No ratio is asserted: the parent of this engine cannot run the workload, there is nothing
to compare with.  Text that follows a line starting with "# python bench.py" in the output file is kept as it is (the alternating
headline runs are recorded there).  Without a GPU the file holds the host arithmetic and says that nothing was measured."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, C, H, E = 36, 2048, 512, 512
KEEP = "# python bench.py"


def per_map_bytes(T):
    """what one (image, word) row holds while it is explained: its r_feat and a_proj rows, the lock-step state (ten (H) / (E) rows, rx,
    the accumulated weights of its t + 1 <= T words, r_words)"""
    return dict(r_feat=4 * P * C, a_proj=4 * P * H, lockstep=4 * (8 * H + E + (2 * E + 2 * H) + T * H + T), r_avg=4 * H)


def trace_bytes(B, T):
    """`GridTDEngine._alloc_trace` (grad=False)"""
    return 4 * B * (T * (2 * E + 2 * H) + T * 3 * H + 4 * (T + 1) * H + 10 * T * H + T * P + T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", type=int, nargs="?", default=32)
    ap.add_argument("words", type=int, nargs="?", default=20)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--vocab", type=int, default=9586)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gridtd_bu_timing.txt"))
    a = ap.parse_args()
    if a.iters < 5:
        raise SystemExit("--iters: the median of at least 5 runs")
    sys.path.insert(0, ROOT)
    import torch
    import lrp_amd  # noqa: F401
    from lrp_amd import weights
    B, T, V = a.batch, a.words, a.vocab
    pm = per_map_bytes(T)
    head = f"== bottom-up gridTD (GridTDBUEngine), {B} images of {P} x {C} region features x {T} words = {B * T} maps, V = {V}"
    lines = [head, "host arithmetic, per map: " + ", ".join(f"{k} {v} bytes" for k, v in pm.items()) + f" = {sum(pm.values())} bytes "
                   f"({sum(pm.values()) / 2**10:.0f} KiB); per batch: features {4 * B * P * C} bytes, decoder trace {trace_bytes(B, T)} bytes, "
                   f"Vp + proj_pre + att_img {4 * B * P * (2 * H + P)} bytes, predictions (when asked) {4 * B * T * V} bytes"]
    kept = []
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = f.read().split("\n")
        at = [i for i, ln in enumerate(old) if ln.startswith(KEEP)]
        kept = old[at[0]:] if at else []

    def write():
        with open(a.out, "w") as f:
            f.write("\n".join(lines + ([""] + kept if kept else [])).rstrip("\n") + "\n")

    if not torch.cuda.is_available():
        lines.append("nothing was measured: no GPU on this machine")
        print("\n".join(lines))
        write()
        return
    from lrp_amd.explainers.aoa import AOAEngine
    from lrp_amd.explainers.gridtd import GridTDBUEngine
    lines[0] = head + f", {torch.cuda.get_device_name(0)}, HIP events, median of {a.iters} (min .. max) after two warm-up steps"
    feats = torch.from_numpy(weights.make_bu_features(1, B, P, C)).cuda()
    cap = torch.from_numpy(weights.make_captions(2, B, T, V)).cuda()
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0, e1 = ev(), ev()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1)

    def report(title, ms, total_line=True):
        lines.append(f"  {title}")
        total = 0.0
        for k, v in ms.items():
            med = statistics.median(v)
            total += med
            lines.append(f"    {k:<22s} {med:9.3f} ms  ({min(v):.3f} .. {max(v):.3f})")
        if total_line:
            lines.append(f"    {'sum':<22s} {total:9.3f} ms")
        return total

    eng = GridTDBUEngine(weights.make_gridtd_bu_state(seed=0, vocab_size=V))
    for _ in range(2):
        r_feat, r_words = eng.explain_batch(feats, cap)
    torch.cuda.synchronize()
    assert r_feat.shape == (B, T, P, C) and bool(torch.isfinite(r_feat).all()) and bool(torch.isfinite(r_words).all())
    del r_feat, r_words
    # the phases: events recorded at the entry of the tail and of the projector rule split `relevance` in three
    marks = {}
    tail, proj = eng._rel_tail, eng._proj_rule

    def mark(name, fn):
        def wrapped(*args, **kw):
            marks[name] = ev()
            marks[name].record()
            return fn(*args, **kw)
        return wrapped
    ms = {k: [] for k in ("encode", "decoder trace", "lock-steps", "tail", "projector rule")}
    eng._rel_tail, eng._proj_rule = mark("tail", tail), mark("proj", proj)
    for _ in range(a.iters):
        enc, t0 = timed(lambda: eng.encode(feats))
        tr, t1 = timed(lambda: eng.trace(enc, cap, predictions=False))
        e0, e1 = ev(), ev()
        e0.record()
        out = eng.relevance(enc, tr)
        e1.record()
        e1.synchronize()
        for k, v in zip(ms, (t0, t1, e0.elapsed_time(marks["tail"]), marks["tail"].elapsed_time(marks["proj"]), marks["proj"].elapsed_time(e1))):
            ms[k].append(v)
        del out
    del eng._rel_tail, eng._proj_rule                                  # (instance attributes: the class's methods are back)
    total = report("phases of explain_batch (each timed alone, the host waits between them)", ms)
    lines.append(f"    = {total / (B * T) * 1e3:.2f} us per map")
    whole = {"explain_batch": [], "explain_batch_replay": []}
    eng.explain_batch_replay(feats, cap)
    for _ in range(a.iters):
        whole["explain_batch"].append(timed(lambda: eng.explain_batch(feats, cap))[1])
        whole["explain_batch_replay"].append(timed(lambda: eng.explain_batch_replay(feats, cap))[1])
    report("the whole step, one batch in flight", whole, total_line=False)
    for k, v in whole.items():
        med = statistics.median(v)
        lines.append(f"    {k}: {B * T / med * 1e3:.0f} maps/s, {med / (B * T) * 1e3:.2f} us per map")
    lines.append(f"  peak device memory {torch.cuda.max_memory_allocated() / 2**20:.0f} MiB (weights and packs of V = {V} included)")
    del eng
    torch.cuda.empty_cache()
    # for orientation: the sibling model's bottom-up step
    aoa = AOAEngine(weights.make_aoa_state(seed=0, vocab_size=V, feat_dim=C, with_encoder=False))
    for _ in range(2):
        aoa.explain_batch(cap, 0, features=feats)
    aoa.explain_batch_replay(cap, 0, features=feats)
    torch.cuda.synchronize()
    whole = {"explain_batch": [], "explain_batch_replay": []}
    for _ in range(a.iters):
        whole["explain_batch"].append(timed(lambda: aoa.explain_batch(cap, 0, features=feats))[1])
        whole["explain_batch_replay"].append(timed(lambda: aoa.explain_batch_replay(cap, 0, features=feats))[1])
    report(f"for orientation: AOAEngine's bottom-up step (features=, head 0), the same {B} x {T}, V = {V}, the same process", whole, total_line=False)
    for k, v in whole.items():
        med = statistics.median(v)
        lines.append(f"    {k}: {B * T / med * 1e3:.0f} maps/s, {med / (B * T) * 1e3:.2f} us per map")
    print("\n".join(lines))
    write()


if __name__ == "__main__":
    main()
