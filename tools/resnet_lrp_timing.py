#!/usr/bin/env python3
"""What one `compute_lrp` through a ResNet-50-shaped bottleneck encoder costs on the generic leaf driver: the net of
tests/golden/make_golden_resnet.py (`bottleneck_net(base=64, blocks=[3, 4, 6, 3])`, seeded weights) on a (4, 3, 224, 224) batch.

    python tools/resnet_lrp_timing.py [--out profiles/resnet_lrp_timing.txt] [--batch 4] [--iters 3]
    python tools/resnet_lrp_timing.py --engine [--engine-out profiles/resnet_engine_timing.txt] [--words 5]
    python tools/resnet_lrp_timing.py --engine --conv-mode both --batch 16 [--engine-only] [--engine-out profiles/resnet_engine_b6_timing.txt]
    python tools/resnet_lrp_timing.py --engine --alpha 2 --beta 1 [--conv-mode 0|1] [--engine-only]      (profiles/resnet_engine_ab_timing.txt)
    python tools/resnet_lrp_timing.py --engine --pass all --conv-mode both --batch 4 --words 10 --size 448 --blocks 3,4,23,3 --reps 3
                                                                                                      (profiles/resnet_grad_timing.txt)

Reports the whole call, the milliseconds per leaf type (HIP events around each rule call, layout conversions and the rule's checks
included) and every distinct launch of the runtime-geometry conv engine (csrc/conv_geom.hip) with its flop as issued -
2 n OH OW kh kw K n_oc with the K and n_oc the launch was given, i.e. with the doubled channels of the split [x+ | x-] storage - as
achieved TFLOP/s against the 157 TFLOP/s fp32-MFMA peak.  Times are HIP events on one stream after a warm-up call, averaged over
--iters calls; an interval around one launch on an otherwise idle stream includes that launch's latency.  Nothing is asserted.

--engine adds a second leg after that report (which it leaves as it is): the batched engine (`ops.ResNetEncoder`) on
--batch images x --words words = 20 maps, against the generic driver given the same 20 maps as 20 replicated images, in the same
process.  It reports the milliseconds per trace and per relevance call, the engine's per-layer times, the achieved TFLOP/s of its
transposed convs (flop as issued: 2 n_maps OH OW kh kw K n_oc) and the speed-up, and says whether the 2x floor of the engine's issue
is met; which layers hold it back is read off the per-layer table.

--conv-mode picks the engine's arithmetic for that leg (0: fp32 MFMA, 1: the exact bf16 split of DESIGN.md 5.9).  `both` runs the leg
in mode 0 and then compares the modes: both engines in this process, warmed, mode 0 and mode 1 ALTERNATING for --reps repetitions
each (at least 5), HIP events around `forward` and around `relevance`; then the per-layer tables of both.  Baseline: the mode-0 engine
of the same run.  Noise: the spread (max - min) of mode 0 over its repetitions - a difference inside it is reported as "no
difference".  --engine-only skips the generic driver (the first report and the engine leg's comparison against it).

--alpha / --beta (with --engine) run the general alpha-beta rule instead (`ops.ResNetEncoder.relevance_alpha_beta`): in
one process, warmed and ALTERNATING for --reps repetitions (at least 5), the alpha-beta map pass, the preset's map pass on the same
engine and the generic driver under the same lrp_params on replicated images; then the time of a forward plus the first alpha-beta
call (which makes qn) and the per-layer table of both map passes.  It prints medians, the spread (max - min) of the repetitions as the
noise, and the measured ratios; no ratio is fixed.  By flop count the alpha-beta map pass is 2 x the preset's and the generic driver
does about 4 x the preset's conv work per map.  The targets are scaled by 1e-8: with beta != 0 the relevance grows by up to
(alpha + beta) per conv, and the generic driver refuses a non-finite result.  Writes --engine-out, by default
profiles/resnet_engine_ab_timing.txt.

--pass gradient | guided | all (with --engine; `relevance`, the default, is the legs above) times the gradient chain of the engine
(`ops.ResNetEncoder.gradient` / `guided_backprop`) beside `relevance` on the same trace: per conv mode (--conv-mode 0, 1
or both) one engine, one forward of --batch images of --size x --size pixels through `bottleneck_net(64, --blocks)`, every pass
warmed once, then the passes ALTERNATING for --reps repetitions (at least 3) on --batch x --words maps with HIP events around each
call.  `gradient` times relevance and the plain gradient, `guided` relevance and guided backprop with relus = "stem" and "all", `all`
the four.  It prints the median, the spread (min .. max) and the median per map, and each pass against `relevance`; nothing is
asserted.  Writes --engine-out, by default profiles/resnet_grad_timing.txt."""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TFLOPS = 157.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--engine", action="store_true", help="add the batched-engine leg (ops.ResNetEncoder against the generic driver)")
    ap.add_argument("--words", type=int, default=5, help="--engine: maps per image")
    ap.add_argument("--engine-out", default=None, help="--engine: also write that leg's report to this file")
    ap.add_argument("--conv-mode", choices=["0", "1", "both"], default="0", help="--engine: the engine's arithmetic; both: compare them")
    ap.add_argument("--reps", type=int, default=5, help="--conv-mode both: alternating repetitions per mode (at least 5)")
    ap.add_argument("--engine-only", action="store_true", help="--engine: skip the generic driver's legs")
    ap.add_argument("--alpha", type=float, default=None, help="--engine: time the general alpha-beta rule (with --beta)")
    ap.add_argument("--beta", type=float, default=None)
    ap.add_argument("--pass", dest="passes", choices=["relevance", "gradient", "guided", "all"], default="relevance",
                    help="--engine: time the gradient chain beside relevance (DESIGN.md 5.12)")
    ap.add_argument("--size", type=int, default=224, help="--pass: image side")
    ap.add_argument("--blocks", default="3,4,6,3", help="--pass: blocks per stage (3,4,23,3 is the ResNet-101 shape)")
    a = ap.parse_args()
    if (a.alpha is None) != (a.beta is None) or (a.alpha is not None and not a.engine):
        ap.error("--alpha and --beta go together, and with --engine")
    if a.alpha is not None and a.conv_mode == "both":
        ap.error("--alpha / --beta: one conv mode per run")
    if a.passes != "relevance" and (not a.engine or a.alpha is not None):
        ap.error("--pass goes with --engine, without --alpha / --beta")
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import lrp_amd  # noqa: F401
    from lrp_amd import _lib, ops
    from lrp_amd.LRPtools import lrp_modules, lrp_wrapper
    from make_golden_resnet import bottleneck_net
    if not torch.cuda.is_available():
        raise SystemExit("resnet_lrp_timing: no GPU - a time is measured on the device or not at all")
    if a.passes != "relevance":
        return pass_leg(a)
    net = bottleneck_net(np.random.RandomState(0), lrp_modules.resAdd, 64, [3, 4, 6, 3]).cuda()
    lrp_wrapper.add_lrp(net)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.batch, 3, 224, 224, generator=g).cuda()
    if a.alpha is not None:
        return ab_leg(a, net, x)
    if a.engine and a.engine_only:
        return engine_leg(a, net, x)
    with torch.no_grad():
        target = torch.randn(net(x).shape, generator=g).cuda()

    events = []                                   # (kind, key, start, end)

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e
    real_get, real_geom = lrp_modules.get_lrp_module, ops.conv_geom

    def get_timed(module):
        rule = real_get(module)
        real = rule.propagate_relevance

        def timed(*args, **kw):
            e0 = ev()
            out = real(*args, **kw)
            events.append(("leaf", type(module).__name__, e0, ev()))
            return out
        rule.propagate_relevance = timed
        return rule

    def geom_timed(inp, wpacked, direction, n, hw, ohw, geom, k, n_oc, **kw):
        e0 = ev()
        out = real_geom(inp, wpacked, direction, n, hw, ohw, geom, k, n_oc, **kw)
        events.append(("launch", (direction, geom, hw, k, n_oc, n, ohw), e0, ev()))
        return out

    def call():
        e0 = ev()
        net.compute_lrp(x.clone(), target=target)
        events.append(("call", "compute_lrp", e0, ev()))
    call()                                        # warm-up: packs the weights, loads every kernel
    torch.cuda.synchronize()
    lrp_modules.get_lrp_module, ops.conv_geom = get_timed, geom_timed
    try:
        for _ in range(a.iters):
            call()
        torch.cuda.synchronize()
    finally:
        lrp_modules.get_lrp_module, ops.conv_geom = real_get, real_geom
    ms = collections.defaultdict(float)
    cnt = collections.Counter()
    for kind, key, e0, e1 in events[1:]:
        ms[(kind, key)] += e0.elapsed_time(e1) / a.iters
        cnt[(kind, key)] += 1
    lines = [f"# tools/resnet_lrp_timing.py --batch {a.batch} --iters {a.iters}",
             f"== bottleneck_net(base=64, blocks=[3,4,6,3]) on ({a.batch}, 3, 224, 224), {torch.cuda.get_device_name(0)}",
             f"compute_lrp, whole call : {ms[('call', 'compute_lrp')]:9.2f} ms", "",
             "per leaf type (rule calls per compute_lrp, ms per compute_lrp)"]
    for (kind, key), v in sorted(ms.items(), key=lambda kv: -kv[1]):
        if kind == "leaf":
            lines.append(f"  {key:<14} {cnt[(kind, key)] // a.iters:4d} calls {v:9.2f} ms")
    lines += ["", "conv engine launches (per distinct shape: launches per compute_lrp, ms per launch, flop as issued, achieved TFLOP/s, % of "
              f"{PEAK_TFLOPS:.0f})",
              f"  {'dir':<3} {'kernel':<6} {'stride':<6} {'map':<9} {'K':>5} {'n_oc':>5} {'launches':>8} {'ms':>8} {'GFLOP':>8} {'TFLOP/s':>8} {'%peak':>6}"]
    tot_ms = tot_fl = 0.0
    for (kind, key), v in sorted(ms.items(), key=lambda kv: -kv[1]):
        if kind != "launch":
            continue
        direction, geom, hw, k, n_oc, n, ohw = key
        c = cnt[(kind, key)] // a.iters
        per = v / c
        flop = 2.0 * n * ohw[0] * ohw[1] * geom[0] * geom[1] * k * n_oc
        tf = flop / (per * 1e-3) / 1e12
        tot_ms += v
        tot_fl += flop * c
        lines.append(f"  {'fwd' if direction == _lib.GEOM_FWD else 'bwd':<3} {geom[0]}x{geom[1]:<4} {geom[2]}x{geom[3]:<4} {hw[0]}x{hw[1]:<5} "
                     f"{k:5d} {n_oc:5d} {c:8d} {per:8.3f} {flop / 1e9:8.2f} {tf:8.2f} {100 * tf / PEAK_TFLOPS:6.1f}")
    if tot_ms:
        lines.append(f"  all conv engine launches: {tot_ms:.2f} ms, {tot_fl / 1e9:.1f} GFLOP, {tot_fl / (tot_ms * 1e-3) / 1e12:.2f} TFLOP/s")
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if a.out:
        with open(a.out, "w") as f:
            f.write(report)
    if a.engine:
        engine_leg(a, net, x)


def engine_leg(a, net, x):
    import torch
    from lrp_amd import _lib, ops
    g = torch.Generator().manual_seed(1)
    n_maps = a.batch * a.words
    map2img = torch.arange(n_maps, dtype=torch.int32).div(a.words, rounding_mode="floor").to(torch.int32).cuda()
    with torch.no_grad():
        feat_shape = tuple(net(x[:1]).shape[1:])
    targets = torch.randn((n_maps,) + feat_shape, generator=g).cuda()
    x_rep = x[map2img.long()].contiguous()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()                                      # warm-up
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters
    mode = 1 if a.conv_mode == "1" else 0
    generic_ms = float("nan") if a.engine_only else timed(lambda: net.compute_lrp(x_rep.clone(), target=targets))
    eng = ops.ResNetEncoder(net, conv_mode=mode)
    t_nhwc = ops.nchw_to_nhwc(targets)
    trace_ms = timed(lambda: eng.forward(x))
    rel_ms = timed(lambda: eng.relevance(t_nhwc, map2img))
    both_ms = timed(lambda: (eng.forward(x), eng.relevance(t_nhwc, map2img)))
    fwd_layers, rel_layers = {}, {}
    for _ in range(a.iters):
        eng.forward(x, layer_ms=fwd_layers)
        eng.relevance(t_nhwc, map2img, layer_ms=rel_layers)
    lines = [f"# tools/resnet_lrp_timing.py --engine --conv-mode {a.conv_mode} --batch {a.batch} --words {a.words} --iters {a.iters}"
             + (" --engine-only" if a.engine_only else ""),
             f"== bottleneck_net(base=64, blocks=[3,4,6,3]), {a.batch} images x {a.words} words = {n_maps} maps at 224 x 224, "
             f"{torch.cuda.get_device_name(0)}, engine conv mode {mode}",
             f"generic driver, compute_lrp on {n_maps} replicated images : {generic_ms:9.2f} ms" + ("  (skipped)" if a.engine_only else ""),
             f"engine, forward (trace of {a.batch} images)             : {trace_ms:9.2f} ms",
             f"engine, relevance ({n_maps} maps)                       : {rel_ms:9.2f} ms",
             f"engine, forward + relevance                          : {both_ms:9.2f} ms",
             f"trace memory                                         : {eng.trace_bytes(a.batch, 224, 224) / 2**20 / a.batch:9.1f} MiB per image",
             f"speed-up over the generic driver (same run)          : {generic_ms / both_ms:9.2f} x   (floor 2.00 x: "
             f"{'not run' if a.engine_only else 'met' if generic_ms / both_ms >= 2.0 else 'NOT met'})", "",
             "per layer, a pass with one HIP-event wait per layer (ms per call; trace = stacked forward conv + BN / coefficient pass, "
             f"relevance = transposed conv; flop as issued, % of {PEAK_TFLOPS:.0f} TFLOP/s)",
             f"  {'layer':<24} {'kernel':<6} {'stride':<6} {'map':<9} {'cin':>5} {'cout':>5} {'trace ms':>9} {'rel ms':>8} {'rel GFLOP':>9} {'TFLOP/s':>8} {'%peak':>6}"]
    tot_ms = tot_fl = 0.0
    for i, cv in enumerate(eng.plan.convs):
        kh, kw, sh, sw, _, _ = cv["geom"]
        hw, ohw = eng.dims[i]
        n_oc = eng.c2 if not cv["nonneg"] else cv["cin"]
        flop = 2.0 * n_maps * ohw[0] * ohw[1] * kh * kw * cv["cout"] * n_oc
        rms = rel_layers[cv["name"]] / a.iters
        tf = flop / (rms * 1e-3) / 1e12
        tot_ms += rms
        tot_fl += flop
        lines.append(f"  {cv['name']:<24} {kh}x{kw:<4} {sh}x{sw:<4} {hw[0]}x{hw[1]:<5} {cv['cin']:5d} {cv['cout']:5d} "
                     f"{fwd_layers[cv['name']] / a.iters:9.3f} {rms:8.3f} {flop / 1e9:9.2f} {tf:8.2f} {100 * tf / PEAK_TFLOPS:6.1f}")
    lines.append(f"  all transposed convs: {tot_ms:.2f} ms, {tot_fl / 1e9:.1f} GFLOP, {tot_fl / (tot_ms * 1e-3) / 1e12:.2f} TFLOP/s "
                 f"({100 * tot_fl / (tot_ms * 1e-3) / 1e12 / PEAK_TFLOPS:.1f} % of {PEAK_TFLOPS:.0f})")
    if a.conv_mode == "both":
        lines += [""] + mode_leg(a, net, x, t_nhwc, map2img, eng)
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if a.engine_out:
        with open(a.engine_out, "w") as f:
            f.write(report)


def pass_leg(a):
    """relevance and the gradient chain's passes on one trace per conv mode, alternating in this process"""
    import numpy as np
    import torch
    from lrp_amd import ops
    from lrp_amd.LRPtools import lrp_modules
    from make_golden_resnet import bottleneck_net
    blocks = [int(b) for b in a.blocks.split(",")]
    reps, n_maps = max(a.reps, 3), a.batch * a.words
    net = bottleneck_net(np.random.RandomState(0), lrp_modules.resAdd, 64, blocks).cuda()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.batch, 3, a.size, a.size, generator=g).cuda()
    map2img = torch.arange(n_maps, dtype=torch.int32).div(a.words, rounding_mode="floor").to(torch.int32).cuda()
    names = {"gradient": ["relevance", "gradient"], "guided": ["relevance", "guided stem", "guided all"],
             "all": ["relevance", "gradient", "guided stem", "guided all"]}[a.passes]
    lines = [f"# tools/resnet_lrp_timing.py --engine --pass {a.passes} --conv-mode {a.conv_mode} --batch {a.batch} --words {a.words} "
             f"--size {a.size} --blocks {a.blocks} --reps {reps}",
             f"== bottleneck_net(base=64, blocks={blocks}), {a.batch} images x {a.words} words = {n_maps} maps at {a.size} x {a.size}, "
             f"{torch.cuda.get_device_name(0)}; passes alternating, {reps} repetitions after one warm-up each, HIP events around each call"]
    for mode in ([0, 1] if a.conv_mode == "both" else [int(a.conv_mode)]):
        eng = ops.ResNetEncoder(net, conv_mode=mode)
        h, w, c = eng.feature_shape(a.size, a.size)
        d = torch.randn(n_maps, h * w, c, generator=g).cuda()
        out = torch.empty(n_maps, 3, a.size, a.size, device="cuda")
        eng.forward(x)
        fns = {"relevance": lambda: eng.relevance(d, map2img, out=out), "gradient": lambda: eng.gradient(d, map2img, out=out),
               "guided stem": lambda: eng.guided_backprop(d, map2img, out=out), "guided all": lambda: eng.guided_backprop(d, map2img, out=out, relus="all")}
        ms = {n: [] for n in names}
        for r in range(reps + 1):
            for n in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[n]()
                e1.record()
                e1.synchronize()
                if r:                              # repetition 0 warms up (and builds the gradient chain's packs)
                    ms[n].append(e0.elapsed_time(e1))
        med = {n: float(np.median(v)) for n, v in ms.items()}
        lines += ["", f"conv mode {mode}  (trace {eng.trace_bytes(a.batch, a.size, a.size) / 2**30:.2f} GiB, peak device memory "
                      f"{torch.cuda.max_memory_allocated() / 2**30:.1f} GiB)",
                  f"  {'pass':<14} {'median ms':>10} {'min':>9} {'max':>9} {'ms per map':>11} {'vs relevance':>13}"]
        for n in names:
            lines.append(f"  {n:<14} {med[n]:10.2f} {min(ms[n]):9.2f} {max(ms[n]):9.2f} {med[n] / n_maps:11.3f} {med[n] / med['relevance']:12.3f}x")
        del eng, d, out
        torch.cuda.empty_cache()
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    with open(a.engine_out or os.path.join(ROOT, "profiles", "resnet_grad_timing.txt"), "w") as f:
        f.write(report)


def mode_leg(a, net, x, t_nhwc, map2img, eng0):
    """conv mode 0 against conv mode 1 of the engine, alternating in this process; returns the report's lines"""
    import torch
    from lrp_amd import ops
    reps = max(5, a.reps)
    engs = {0: eng0, 1: ops.ResNetEncoder(net, conv_mode=1)}
    for e in engs.values():                       # warm-up: trace buffers, workspaces, every kernel loaded
        e.forward(x)
        e.relevance(t_nhwc, map2img)
    torch.cuda.synchronize()
    r0, r1 = engs[0].relevance(t_nhwc, map2img), engs[1].relevance(t_nhwc, map2img)
    dev = ((r1 - r0).abs().amax(dim=(1, 2, 3)) / r0.abs().amax(dim=(1, 2, 3))).max().item()

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    fwd, rel = {0: [], 1: []}, {0: [], 1: []}
    for _ in range(reps):
        for m in (0, 1):
            fwd[m].append(once(lambda: engs[m].forward(x)))
            rel[m].append(once(lambda: engs[m].relevance(t_nhwc, map2img)))
    fl, rl = {0: {}, 1: {}}, {0: {}, 1: {}}
    for _ in range(a.iters):
        for m in (0, 1):
            engs[m].forward(x, layer_ms=fl[m])
            engs[m].relevance(t_nhwc, map2img, layer_ms=rl[m])
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: max(v) - min(v)

    def verdict(t):
        d = med(t[0]) - med(t[1])
        if abs(d) <= spread(t[0]):
            return "no difference (inside mode 0's spread)"
        return f"mode 1 {'faster' if d > 0 else 'SLOWER'}: {med(t[0]) / med(t[1]):.2f} x"
    lines = [f"== conv mode 0 (fp32 MFMA) against conv mode 1 (bf16 split, six products), {reps} alternating repetitions each, ms per call",
             f"  largest difference of a mode-1 map from its mode-0 map: {dev:.2e} of the map's maximum",
             f"  {'':<10} {'mode 0 median':>13} {'min':>8} {'max':>8} {'mode 1 median':>13} {'min':>8} {'max':>8}   verdict"]
    for name, t in (("forward", fwd), ("relevance", rel)):
        lines.append(f"  {name:<10} {med(t[0]):13.3f} {min(t[0]):8.3f} {max(t[0]):8.3f} {med(t[1]):13.3f} {min(t[1]):8.3f} {max(t[1]):8.3f}   "
                     + verdict(t))
    lines += ["", f"per layer, one HIP-event wait per layer, mean of {a.iters} passes (ms; ratio = mode 0 / mode 1, above 1: mode 1 faster)",
              f"  {'layer':<24} {'kernel':<6} {'stride':<6} {'map':<9} {'cin':>5} {'cout':>5} {'trace m0':>9} {'trace m1':>9} {'ratio':>6} "
              f"{'rel m0':>8} {'rel m1':>8} {'ratio':>6}"]
    tot = {k: 0.0 for k in ("f0", "f1", "r0", "r1")}
    for i, cv in enumerate(eng0.plan.convs):
        kh, kw, sh, sw, _, _ = cv["geom"]
        hw = eng0.dims[i][0]
        f0, f1, q0, q1 = (d[cv["name"]] / a.iters for d in (fl[0], fl[1], rl[0], rl[1]))
        for k, v in zip(("f0", "f1", "r0", "r1"), (f0, f1, q0, q1)):
            tot[k] += v
        lines.append(f"  {cv['name']:<24} {kh}x{kw:<4} {sh}x{sw:<4} {hw[0]}x{hw[1]:<5} {cv['cin']:5d} {cv['cout']:5d} {f0:9.3f} {f1:9.3f} "
                     f"{f0 / f1:6.2f} {q0:8.3f} {q1:8.3f} {q0 / q1:6.2f}")
    lines.append(f"  {'all conv layers':<24} {'':<6} {'':<6} {'':<9} {'':>5} {'':>5} {tot['f0']:9.3f} {tot['f1']:9.3f} {tot['f0'] / tot['f1']:6.2f} "
                 f"{tot['r0']:8.3f} {tot['r1']:8.3f} {tot['r0'] / tot['r1']:6.2f}")
    return lines


def ab_leg(a, net, x):
    """the general alpha-beta rule on the engine against the preset on the same engine and against the generic driver under the same
    parameters, alternating in this process"""
    import torch
    from lrp_amd import _lib, ops
    from lrp_amd.LRPtools import lrp_wrapper
    g = torch.Generator().manual_seed(1)
    n_maps, reps, mode = a.batch * a.words, max(5, a.reps), int(a.conv_mode)
    map2img = torch.arange(n_maps, dtype=torch.int32).div(a.words, rounding_mode="floor").to(torch.int32).cuda()
    with torch.no_grad():
        feat_shape = tuple(net(x[:1]).shape[1:])
    targets = torch.randn((n_maps,) + feat_shape, generator=g).cuda() * 1e-8
    x_rep = x[map2img.long()].contiguous()
    lrp_wrapper.add_lrp(net, lrp_params={"alpha": a.alpha, "beta": a.beta})
    eng = ops.ResNetEncoder(net, conv_mode=mode)
    t_nhwc = ops.nchw_to_nhwc(targets)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    legs = {"ab": lambda: eng.relevance_alpha_beta(t_nhwc, map2img, a.alpha, a.beta), "preset": lambda: eng.relevance(t_nhwc, map2img),
            "first": lambda: (eng.forward(x), eng.relevance_alpha_beta(t_nhwc, map2img, a.alpha, a.beta))}
    generic_note = "skipped"
    if not a.engine_only:
        legs["generic"] = lambda: net.compute_lrp(x_rep.clone(), target=targets)
    eng.forward(x)
    try:
        for fn in legs.values():                  # warm-up: packs, qn, workspaces, every kernel loaded
            fn()
        generic_note = ""
    except _lib.LrpxError as err:                 # the generic driver's finite / non-zero check
        legs.pop("generic", None)
        generic_note = "refused its result: " + str(err)[:60]
    torch.cuda.synchronize()
    r_ab = legs["ab"]()
    finite = bool(torch.isfinite(r_ab).all())
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(once(fn))
    lay_ab, lay_pre = {}, {}
    for _ in range(a.iters):
        eng.relevance_alpha_beta(t_nhwc, map2img, a.alpha, a.beta, layer_ms=lay_ab)
        eng.relevance(t_nhwc, map2img, layer_ms=lay_pre)
    med = lambda v: sorted(v)[len(v) // 2]
    row = lambda name, v: f"  {name:<46} {med(v):10.3f} {min(v):10.3f} {max(v):10.3f} {max(v) - min(v):10.3f}"
    lines = [f"# tools/resnet_lrp_timing.py --engine --alpha {a.alpha:g} --beta {a.beta:g} --conv-mode {mode} --batch {a.batch} --words {a.words} "
             f"--reps {reps} --iters {a.iters}" + (" --engine-only" if a.engine_only else ""),
             f"== bottleneck_net(base=64, blocks=[3,4,6,3]), {a.batch} images x {a.words} words = {n_maps} maps at 224 x 224, "
             f"{torch.cuda.get_device_name(0)}, engine conv mode {mode}, alpha {a.alpha:g} beta {a.beta:g}; the alpha-beta maps are "
             f"{'finite' if finite else 'NOT finite'}",
             f"{reps} alternating repetitions, ms per call", f"  {'':<46} {'median':>10} {'min':>10} {'max':>10} {'spread':>10}",
             row(f"engine, alpha-beta map pass ({n_maps} maps)", ms["ab"]), row(f"engine, preset map pass ({n_maps} maps)", ms["preset"]),
             row("engine, forward + first alpha-beta call (qn)", ms["first"])]
    if "generic" in ms:
        lines.append(row(f"generic driver, {n_maps} replicated images", ms["generic"]))
    else:
        lines.append(f"  generic driver: {generic_note}")
    lines += ["", f"alpha-beta map pass / preset map pass      : {med(ms['ab']) / med(ms['preset']):6.2f} x   (2 x by flop count)"]
    if "generic" in ms:
        lines += [f"generic driver / alpha-beta map pass       : {med(ms['generic']) / med(ms['ab']):6.2f} x",
                  f"generic driver / (forward + first call)    : {med(ms['generic']) / med(ms['first']):6.2f} x"]
    lines += [f"trace memory with qn                       : {eng.trace_bytes(a.batch, 224, 224, alpha_beta=True) / 2**20 / a.batch:6.1f} MiB "
              f"per image ({eng.trace_bytes(a.batch, 224, 224) / 2**20 / a.batch:.1f} without)", "",
              f"per layer, one HIP-event wait per layer, mean of {a.iters} passes (ms; the transposed conv of each layer)",
              f"  {'layer':<24} {'kernel':<6} {'stride':<6} {'map':<9} {'cin':>5} {'cout':>5} {'preset':>8} {'alpha-beta':>10} {'ratio':>6}"]
    tot = [0.0, 0.0]
    for i, cv in enumerate(eng.plan.convs):
        kh, kw, sh, sw, _, _ = cv["geom"]
        hw = eng.dims[i][0]
        p, q = lay_pre[cv["name"]] / a.iters, lay_ab[cv["name"]] / a.iters
        tot[0] += p
        tot[1] += q
        lines.append(f"  {cv['name']:<24} {kh}x{kw:<4} {sh}x{sw:<4} {hw[0]}x{hw[1]:<5} {cv['cin']:5d} {cv['cout']:5d} {p:8.3f} {q:10.3f} {q / p:6.2f}")
    lines.append(f"  {'all conv layers':<24} {'':<6} {'':<6} {'':<9} {'':>5} {'':>5} {tot[0]:8.3f} {tot[1]:10.3f} {tot[1] / tot[0]:6.2f}")
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    with open(a.engine_out or os.path.join(ROOT, "profiles", "resnet_engine_ab_timing.txt"), "w") as f:
        f.write(report)


if __name__ == "__main__":
    main()
