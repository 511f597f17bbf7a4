#!/usr/bin/env python3
"""Phase times of the AoA explainers on a ResNet encoder: a random-init ResNet-101-shaped net -
tests/golden/make_golden_resnet.py `bottleneck_net(base=64, blocks=[3, 4, 23, 3])`, seeded - at 224 x 224 (the reference's default
args.height / args.width: 7 x 7 = 49 attention pixels of 2048 channels), B images x T words, one head, in both encoder conv modes.

    python tools/aoa_resnet_timing.py [B [T]] [--iters 3] [--head 0] [--blocks 3,4,23,3] [--out profiles/aoa_resnet_timing.txt]

Prints the host arithmetic of the sizes - `trace_bytes` (the encoder trace of the B images), the decoder trace, the encoder workspace of
the B x T maps - warms up once, then takes HIP-event times (median of --iters, with min .. max) of the four phases of `explain_batch` -
`encode` (encoder trace + image-side constants), decoder trace, decoder relevance, encoder relevance - and of the same four phases of
`explain_batch_gradient(kind="gradient")`, per mode.  No ratio is asserted: the parent of this engine cannot run the workload, there is
nothing to compare with.  Without a GPU the file holds the host arithmetic and says that nothing was measured."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 224


def decoder_trace_bytes(B, T, P, H=512, E=512, NH=8):
    """bytes of `AOAEngine._alloc_trace` (grad=False): xh, h, c, alpha, seven (B, T, H) tensors and the three rows of maxima"""
    return 4 * (B * T * (E + 2 * H) + 2 * B * (T + 1) * H + B * T * NH * P + 7 * B * T * H + 3 * B * T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", type=int, nargs="?", default=4)
    ap.add_argument("words", type=int, nargs="?", default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--head", type=int, default=0)
    ap.add_argument("--blocks", default="3,4,23,3")
    ap.add_argument("--vocab", type=int, default=11027)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aoa_resnet_timing.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import numpy as np
    import torch
    import lrp_amd  # noqa: F401
    from lrp_amd import ops, weights
    from lrp_amd.LRPtools import lrp_modules
    from make_golden_resnet import bottleneck_net
    B, T, blocks = a.batch, a.words, [int(v) for v in a.blocks.split(",")]
    net = bottleneck_net(np.random.RandomState(0), lrp_modules.resAdd, 64, blocks)
    plan = ops.match_bottleneck_resnet(net)
    P = (-(-SIZE // 32)) ** 2
    head = f"== AoA on bottleneck_net(base=64, blocks={blocks}), {B} images x {T} words = {B * T} maps at {SIZE} x {SIZE}, head {a.head}"
    lines = [head, f"host arithmetic: {len(plan.convs)} convs, P = {P} attention pixels of 2048 channels; decoder trace "
                   f"{decoder_trace_bytes(B, T, P)} bytes; features {4 * B * P * 2048} bytes, r_feat / d_feat of the maps {4 * B * T * P * 2048} bytes, "
                   f"maps {4 * B * T * 3 * SIZE * SIZE} bytes"]
    if not torch.cuda.is_available():
        lines.append("nothing was measured: no GPU on this machine")
        print("\n".join(lines))
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    from lrp_amd.explainers.aoa import AOAResNetEngine
    net = net.cuda()
    sd = weights.make_aoa_state(seed=0, vocab_size=a.vocab, feat_dim=2048, with_encoder=False)
    x = torch.from_numpy(weights.make_images(1, B, SIZE, SIZE)).cuda()
    cap = torch.from_numpy(weights.make_captions(2, B, T, a.vocab)).cuda()
    lines[0] = head + f", {torch.cuda.get_device_name(0)}, HIP events, median of {a.iters} (min .. max) after one warm-up"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1)

    def report(title, ms):
        med = {k: statistics.median(v) for k, v in ms.items()}
        total = sum(med.values())
        lines.append(f"  {title}")
        for k, v in med.items():
            lines.append(f"    {k:<18s} {v:9.2f} ms  ({min(ms[k]):.2f} .. {max(ms[k]):.2f}; {100 * v / total:4.1f} %)")
        lines.append(f"    {'sum':<18s} {total:9.2f} ms  = {total / (B * T):.3f} ms per map")
        print("\n".join(lines[-6:]), flush=True)

    for mode in (0, 1):
        eng = AOAResNetEngine(sd, encoder=net, encoder_conv_mode=mode)
        tb = eng.cnn.trace_bytes(B, SIZE, SIZE)
        lines.append(f"encoder_conv_mode {mode}: trace_bytes = {tb} ({tb / B / 2**20:.1f} MiB per image)")
        print(lines[-1], flush=True)
        maps = eng.explain_batch(cap, a.head, images=x)[0]                     # warm-up (packs, workspaces, kernel attributes)
        grads = eng.explain_batch_gradient(cap, a.head, x, kind="gradient")[0]
        torch.cuda.synchronize()
        assert maps.shape == grads.shape == (B, T, 3, SIZE, SIZE) and bool(torch.isfinite(maps).all()) and bool(torch.isfinite(grads).all())
        ws = sum(v.numel() * 4 if torch.is_tensor(v) else sum(t.numel() * 4 for t in v) for v in eng.cnn._workspace(B * T).values())
        lines.append(f"  encoder workspace of the {B * T} maps: {ws} bytes ({ws / (B * T) / 2**20:.2f} MiB per map); peak device memory "
                     f"{torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")
        del maps, grads
        names = ("encode", "decoder trace", "decoder relevance", "encoder relevance")
        ms = {k: [] for k in names}
        for _ in range(a.iters):
            enc, t0 = timed(lambda: eng.encode(x))
            tr, t1 = timed(lambda: eng.trace(enc, cap, predictions=False))
            (r_feat, r_words, row2img), t2 = timed(lambda: eng.relevance(enc, tr, a.head))
            m, t3 = timed(lambda: eng.cnn.relevance(r_feat, row2img))
            for k, v in zip(ms, (t0, t1, t2, t3)):
                ms[k].append(v)
            del m
        report("LRP (explain_batch)", ms)
        names = ("encode", "decoder trace", "decoder gradient", "encoder gradient")
        ms = {k: [] for k in names}
        for _ in range(a.iters):
            enc, t0 = timed(lambda: eng.encode(x))
            tr, t1 = timed(lambda: eng.trace(enc, cap, predictions=False, grad=True))
            (d_feat, r_words, row2img), t2 = timed(lambda: eng.gradient(enc, tr, a.head))
            m, t3 = timed(lambda: eng.cnn.gradient(d_feat, row2img))
            for k, v in zip(ms, (t0, t1, t2, t3)):
                ms[k].append(v)
            del m
        report('plain gradient (explain_batch_gradient(kind="gradient"))', ms)
        del eng
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
