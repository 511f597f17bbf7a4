#!/usr/bin/env python3
"""Phase times of the gridTD LRP explainer on a ResNet encoder: a random-init ResNet-101-shaped net -
tests/golden/make_golden_resnet.py `bottleneck_net(base=64, blocks=[3, 4, 23, 3])`, seeded - at 448 x 448 (the size at which a stride-32
encoder gives the decoder's 196 attention pixels), B images x T words, in both encoder conv modes.

    python tools/gridtd_resnet_timing.py [B [T]] [--iters 3] [--blocks 3,4,23,3] [--out profiles/gridtd_resnet_timing.txt]

Prints `trace_bytes` (the encoder trace of the B images) and the encoder workspace of the B x T maps, warms up once, then takes HIP-event
times (median of --iters) of the four phases of `explain_batch` - `encode` (encoder trace + image-side constants), decoder trace, decoder
relevance, encoder relevance - per mode.  No ratio is asserted: the parent of this engine cannot run the workload, there is nothing to
compare with.  Without a GPU the file says that nothing was measured."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", type=int, nargs="?", default=4)
    ap.add_argument("words", type=int, nargs="?", default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--blocks", default="3,4,23,3")
    ap.add_argument("--vocab", type=int, default=9586)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gridtd_resnet_timing.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import numpy as np
    import torch
    B, T, blocks = a.batch, a.words, [int(v) for v in a.blocks.split(",")]
    head = f"== gridTD LRP on bottleneck_net(base=64, blocks={blocks}), {B} images x {T} words = {B * T} maps at 448 x 448"
    if not torch.cuda.is_available():
        lines = [head, "nothing was measured: no GPU on this machine"]
        print("\n".join(lines))
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    import lrp_amd  # noqa: F401
    from lrp_amd import weights
    from lrp_amd.LRPtools import lrp_modules
    from lrp_amd.explainers.gridtd import GridTDEngine
    from make_golden_resnet import bottleneck_net
    net = bottleneck_net(np.random.RandomState(0), lrp_modules.resAdd, 64, blocks).cuda()
    sd = weights.make_gridtd_resnet_state(seed=0, vocab_size=a.vocab)
    x = torch.from_numpy(weights.make_images(1, B, 448, 448)).cuda()
    cap = torch.from_numpy(weights.make_captions(2, B, T, a.vocab)).cuda()
    lines = [head + f", {torch.cuda.get_device_name(0)}, HIP events, median of {a.iters} after one warm-up"]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1)

    for mode in (0, 1):
        eng = GridTDEngine(sd, encoder=net, encoder_conv_mode=mode)
        tb = eng.cnn.trace_bytes(B, 448, 448)
        lines.append(f"encoder_conv_mode {mode}: trace_bytes = {tb} ({tb / B / 2**20:.1f} MiB per image)")
        print(lines[-1], flush=True)
        maps = eng.explain_batch(x, cap)[0]                                   # warm-up (packs, workspaces, kernel attributes)
        torch.cuda.synchronize()
        assert maps.shape == (B, T, 3, 448, 448) and bool(torch.isfinite(maps).all())
        ws = sum(v.numel() * 4 if torch.is_tensor(v) else sum(t.numel() * 4 for t in v) for v in eng.cnn._workspace(B * T).values())
        lines.append(f"  encoder workspace of the {B * T} maps: {ws} bytes ({ws / (B * T) / 2**20:.1f} MiB per map), result "
                     f"{maps.numel() * 4 / (B * T) / 2**20:.1f} MiB per map; peak device memory {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")
        del maps
        ms = {k: [] for k in ("encode", "decoder trace", "decoder relevance", "encoder relevance")}
        for _ in range(a.iters):
            enc, t0 = timed(lambda: eng.encode(x))
            tr, t1 = timed(lambda: eng.trace(enc, cap, predictions=False))
            (r_feat, r_words, row2img), t2 = timed(lambda: eng.relevance(enc, tr))
            m, t3 = timed(lambda: eng.cnn.relevance(r_feat, row2img))
            for k, v in zip(ms, (t0, t1, t2, t3)):
                ms[k].append(v)
            del m
        med = {k: statistics.median(v) for k, v in ms.items()}
        total = sum(med.values())
        for k, v in med.items():
            lines.append(f"  {k:<18s} {v:9.2f} ms  ({100 * v / total:4.1f} %)")
        lines.append(f"  {'sum':<18s} {total:9.2f} ms  = {total / (B * T):.2f} ms per map")
        print("\n".join(lines[-5:]), flush=True)
        del eng
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
