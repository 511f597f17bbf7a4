#!/usr/bin/env python3
"""Golden vectors for the batched bottleneck-ResNet encoder engine (ops.ResNetEncoder): a second small net beside resnet_tiny.npz whose
every tile is ragged - base 12, blocks [1, 2, 1] (three stages, an identity block right after a strided one, channel counts 12 / 24 /
48 / 96 / 192: multiples of 4, not of 8 or 32), input 2 x 3 x 45 x 51 - with three targets on the images [1, 0, 1].  Runs the REFERENCE
implementation (LRPtools/lrp_wrapper.py add_lrp / compute_lrp) on a fresh sample tensor per map, once in fp32 and once on .double()
copies, and writes tests/golden/resnet_engine.npz - arrays only, no intermediate activations.

    python tests/golden/make_golden_resnet_engine.py

Seeds are searched with the conditioning recipe of make_golden_resnet.gen_tiny (Add ratio >= 0.1, pool lead >= 1e-3, the reference's
fp32 within 1e-5 of its fp64); the chosen seed is stored.  With two strided stages the recipe is rare at this size (the shortcut's and
the branch's BatchNorm outputs both spread around +2.5, and 45 x 51 pixels hold many pool windows): the forward-only conditioning is
therefore checked first, the two LRP passes run for seeds that meet it.  Seeds 71 .. 164 000 hold none (about 11 ms each);
--first-seed defaults to where that search stopped.  Same harness shims as make_golden.py; run where the reference is available
only."""
import argparse
import os

import numpy as np
import torch

from make_golden import install_stubs
from make_golden_resnet import bottleneck_net, conditioning

HERE = os.path.dirname(os.path.abspath(__file__))
ENGINE = dict(base=12, blocks=[1, 2, 1], shape=(2, 3, 45, 51), map2img=[1, 0, 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-seed", type=int, default=164000, help="71 repeats the whole search")
    first = ap.parse_args().first_seed
    install_stubs()
    from LRPtools import lrp_wrapper
    import models.resnet as rn
    make = lambda seed: bottleneck_net(np.random.RandomState(seed), rn.Add, ENGINE["base"], ENGINE["blocks"])
    m2i = ENGINE["map2img"]
    for seed in range(first, first + 2000000):
        rs = np.random.RandomState(seed)
        x = rs.standard_normal(ENGINE["shape"]).astype(np.float32)
        add_min, pool_min = conditioning(make(seed).double(), torch.from_numpy(x).double())
        if add_min < 0.1 or pool_min < 1e-3:
            continue
        with torch.no_grad():
            oshape = tuple(make(seed)(torch.from_numpy(x)).shape)
        targets = rs.standard_normal((len(m2i),) + oshape[1:]).astype(np.float32)
        res = {}
        for dtype, tag in ((torch.float32, "r32"), (torch.float64, "r64")):
            net = make(seed).to(dtype)
            lrp_wrapper.add_lrp(net)
            rows = []
            for m, img in enumerate(m2i):
                xs = torch.from_numpy(x[img:img + 1].copy()).to(dtype)        # a fresh sample tensor: no .grad running sum
                rows.append(net.compute_lrp(xs, target=torch.from_numpy(targets[m:m + 1].copy()).to(dtype)).numpy()[0])
            res[tag] = np.stack(rows)
        e32 = max(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max() for a, b in zip(res["r32"], res["r64"]))
        print("seed %d: min |x1+x2|/(|x1|+|x2|) %.3f, min pool lead %.2e, e32 %.2e" % (seed, add_min, pool_min, e32))
        if add_min >= 0.1 and pool_min >= 1e-3 and e32 < 1e-5:
            g = dict(x=x, targets=targets, map2img=np.asarray(m2i, dtype=np.int32), seed=np.int64(seed), e32=np.float64(e32), **res)
            np.savez_compressed(os.path.join(HERE, "resnet_engine.npz"), **g)
            print("resnet_engine.npz:", sum(np.asarray(v).nbytes for v in g.values()), "bytes;", {k: np.asarray(v).shape for k, v in g.items()})
            return
    raise SystemExit("no seed met the conditioning recipe")


if __name__ == "__main__":
    main()
