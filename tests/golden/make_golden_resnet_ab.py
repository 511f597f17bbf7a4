#!/usr/bin/env python3
"""Golden vectors of the GENERAL alpha-beta rule through the bottleneck ResNet encoders (ops.ResNetEncoder.relevance_alpha_beta,
DESIGN.md 5.10): the nets, inputs and targets of tests/golden/resnet_engine.npz and resnet_tiny.npz at their stored seeds, run through
the REFERENCE implementation (LRPtools/lrp_wrapper.py add_lrp / compute_lrp with the preset's parameters replaced, the way
make_golden_alphabeta.py replaces them) on a fresh sample tensor per map, once in fp32 and once on .double() copies, for
(alpha, beta) = (2, 1) and (1.5, 0.5).  Writes tests/golden/resnet_ab.npz - outputs, parameters and e32 only; the two input files are
read, never rewritten.

    python tests/golden/make_golden_resnet_ab.py

Maps: the engine fixture's three targets on its map2img; the tiny fixture's target1 / target2 of image 0, then of image 1
(map2img = [0, 0, 1, 1]).  Every case must have the reference's fp32 within 1e-5 of its fp64.  Should the tiny fixture miss that under
a pair, seeds are searched with make_golden_resnet.gen_tiny's conditioning recipe and that case's inputs are stored under
`tiny_<pair>_x / _targets / _seed` in the new file (not needed for the pairs above).  Same harness shims as make_golden.py; run where
the reference is available only."""
import os

import numpy as np
import torch

from make_golden import install_stubs
from make_golden_resnet import TINY, bottleneck_net, conditioning
from make_golden_resnet_engine import ENGINE

HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = [(2., 1.), (1.5, .5)]
TINY_MAP2IMG = [0, 0, 1, 1]


def pair_tag(alpha, beta):
    return "a%g_b%g" % (alpha, beta)


def tiny_targets(t1, t2):
    return np.stack([t1[0], t2[0], t1[1], t2[1]])


def reference_maps(lrp_wrapper, rn, cfg, seed, x, targets, m2i):
    """{'r32', 'r64', 'e32'}: compute_lrp per map on a fresh sample tensor, under whatever lrp_wrapper.SequentialPresetA is now"""
    res = {}
    for dtype, tag in ((torch.float32, "r32"), (torch.float64, "r64")):
        net = bottleneck_net(np.random.RandomState(seed), rn.Add, cfg["base"], cfg["blocks"]).to(dtype)
        lrp_wrapper.add_lrp(net)
        rows = []
        for m, img in enumerate(m2i):
            xs = torch.from_numpy(x[img:img + 1].copy()).to(dtype)
            rows.append(net.compute_lrp(xs, target=torch.from_numpy(targets[m:m + 1].copy()).to(dtype)).numpy()[0])
        res[tag] = np.stack(rows)
    res["e32"] = np.float64(max(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max() for a, b in zip(res["r32"], res["r64"])))
    return res


def search_tiny(lrp_wrapper, rn):
    """gen_tiny's recipe under the current parameters: (seed, x, targets, maps) of the first seed that meets it"""
    for seed in range(31, 4096):
        rs = np.random.RandomState(seed)
        x = rs.standard_normal(TINY["shape"]).astype(np.float32)
        make = lambda: bottleneck_net(np.random.RandomState(seed), rn.Add, TINY["base"], TINY["blocks"])
        add_min, pool_min = conditioning(make().double(), torch.from_numpy(x).double())
        if add_min < 0.1 or pool_min < 1e-3:
            continue
        with torch.no_grad():
            oshape = tuple(make()(torch.from_numpy(x)).shape)
        targets = tiny_targets(rs.standard_normal(oshape).astype(np.float32), rs.standard_normal(oshape).astype(np.float32))
        res = reference_maps(lrp_wrapper, rn, TINY, seed, x, targets, TINY_MAP2IMG)
        print("  seed %d: e32 %.2e" % (seed, res["e32"]))
        if res["e32"] < 1e-5:
            return seed, x, targets, res
    raise SystemExit("no seed met the conditioning recipe")


def main():
    install_stubs()
    from LRPtools import lrp_wrapper
    import models.resnet as rn

    def preset(alpha, beta):
        class Preset(object):
            def __init__(self):
                self.lrp_params = {"alpha": alpha, "beta": beta, "ignore_bias": True}
        return Preset
    E, T = np.load(os.path.join(HERE, "resnet_engine.npz")), np.load(os.path.join(HERE, "resnet_tiny.npz"))
    g = {"pairs": np.asarray(PAIRS, dtype=np.float64), "tiny_map2img": np.asarray(TINY_MAP2IMG, dtype=np.int32)}
    default_preset = lrp_wrapper.SequentialPresetA
    try:
        for alpha, beta in PAIRS:
            lrp_wrapper.SequentialPresetA = preset(alpha, beta)
            tag = pair_tag(alpha, beta)
            res = reference_maps(lrp_wrapper, rn, ENGINE, int(E["seed"]), E["x"], E["targets"], list(E["map2img"]))
            print("engine %s: e32 %.2e" % (tag, res["e32"]))
            assert res["e32"] < 1e-5, ("engine", tag, res["e32"])
            g.update({"engine_%s_%s" % (tag, k): v for k, v in res.items()})
            res = reference_maps(lrp_wrapper, rn, TINY, int(T["seed"]), T["x"], tiny_targets(T["target1"], T["target2"]), TINY_MAP2IMG)
            print("tiny %s: e32 %.2e" % (tag, res["e32"]))
            if not res["e32"] < 1e-5:
                seed, x, targets, res = search_tiny(lrp_wrapper, rn)
                g.update({"tiny_%s_x" % tag: x, "tiny_%s_targets" % tag: targets, "tiny_%s_seed" % tag: np.int64(seed)})
            assert res["e32"] < 1e-5, ("tiny", tag, res["e32"])
            g.update({"tiny_%s_%s" % (tag, k): v for k, v in res.items()})
    finally:
        lrp_wrapper.SequentialPresetA = default_preset
    np.savez_compressed(os.path.join(HERE, "resnet_ab.npz"), **g)
    print("resnet_ab.npz:", sum(np.asarray(v).nbytes for v in g.values()), "bytes;", {k: np.asarray(v).shape for k, v in g.items()})


if __name__ == "__main__":
    main()
