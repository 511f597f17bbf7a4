#!/usr/bin/env python3
"""Golden vectors of the gradient chain through the reference's bottleneck ResNet encoders (ops.ResNetEncoder.gradient /
guided_backprop): two small nets in the shapes of make_golden_resnet.TINY and make_golden_resnet_engine.ENGINE, and for
each the image gradients of a few feature-map gradients in three passes, once in fp32 and once on .double() copies:
    plain   autograd, as ExplainGridTDGradient.explain_cnn runs it (models/gridTDmodel.py:1510-1521)
    stem    the reference's guided backprop: ExplainiGridTDGuidedGradient.register_hooks (:1677-1691) called on a deep copy, as its
            explain_cnn does.  It hooks the DIRECT children of the encoder: on a ResNet the stem's ReLU alone.
    all     max(g, 0) at every ReLU output (canonical guided backprop), which the reference does not have: the autograd restatement
            `chain` below.  The same restatement with the stem's ReLU alone is asserted to be within 1e-5 of the hook path.
Writes tests/golden/resnet_grad.npz - arrays only: per net x, d_feat, map2img, seed, the fp64 maps of the three passes, the fp32 maps
of the two the reference runs itself (plain32, stem32), e32_rows (pass, map) = the fp32 maps' distance from fp64 as a fraction of each
map's maximum, and the margins.

    python tests/golden/make_golden_resnet_grad.py

The nets are `bottleneck_net` with the BatchNorms that feed an Add redrawn like the others (gamma U[0.5, 1.5], beta N(0, 0.2)): with the
stock builder both summands of every Add are positive and no Add ReLU ever cuts (`grad_net`, imported by the tests; it needs no
reference).

Conditioning, a condition on the fixture and not a tolerance: a ReLU mask or a pool winner that differs between two forward passes is
a discontinuity of the gradient.  Seeds are searched until, in fp64, every ReLU input z (every Add sum included) has |z| >= 1e-5 of
its tensor's max |z|, every pool window with a positive maximum leads its runner-up by >= 1e-5 of the tensor's maximum, and the
reference's fp32 is within 1e-5 of its fp64 in every pass.  The margins are stored.  Same harness shims as make_golden.py; run where
the reference is available only."""
import copy
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from make_golden import install_stubs
from make_golden_resnet import TINY, bottleneck_net
from make_golden_resnet_engine import ENGINE

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-5
NETS = {"tiny": dict(TINY, map2img=[1, 0]), "engine": dict(ENGINE)}
PASSES = ("plain", "stem", "all")


def grad_net(seed, add_cls, cfg):
    """bottleneck_net(seed) of cfg's base / blocks with the BatchNorms that feed an Add (bn3, the shortcut's) redrawn from
    RandomState(seed + 1) like the other BatchNorms, in module order"""
    net = bottleneck_net(np.random.RandomState(int(seed)), add_cls, cfg["base"], cfg["blocks"])
    rs = np.random.RandomState(int(seed) + 1)
    for blk in net.layers:
        for bn in [blk.bn3] + ([blk.downsample[1]] if blk.downsample is not None else []):
            c = bn.num_features
            bn.weight.data = torch.from_numpy(rs.uniform(0.5, 1.5, c).astype(np.float32))
            bn.bias.data = torch.from_numpy((rs.standard_normal(c) * 0.2).astype(np.float32))
    return net


class _GuidedReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = x.clamp(min=0)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return g.clamp(min=0) * (y > 0).to(g.dtype)


def chain(net, x, d_feat, relus):
    """the image gradient of one forward written out module by module; relus None: plain autograd, 'stem': max(g, 0) at the stem
    ReLU's output, 'all': at every ReLU's output"""
    relu = lambda t, guided: _GuidedReLU.apply(t) if guided else F.relu(t)
    x = x.clone().requires_grad_(True)
    with torch.enable_grad():
        a = net.maxpool(relu(net.bn1(net.conv1(x)), relus is not None))
        for blk in net.layers:
            o = relu(blk.bn1(blk.conv1(a)), relus == "all")
            o = relu(blk.bn2(blk.conv2(o)), relus == "all")
            o = blk.bn3(blk.conv3(o))
            a = relu(o + (a if blk.downsample is None else blk.downsample(a)), relus == "all")
        a.backward(d_feat)
    return x.grad.detach().clone()


def margins(net64, x64):
    """(min |z| / max |z| over every ReLU input tensor, min lead / max x over every pool window with a positive maximum) of one fp64
    forward"""
    seen = {"relu": np.inf, "pool": np.inf}
    hooks = []

    def relu_hook(m, inp):
        z = inp[0].detach()
        seen["relu"] = min(seen["relu"], (z.abs().min() / z.abs().max()).item())

    def pool_hook(m, inp):
        k, s, p = m.kernel_size, m.stride, m.padding
        xin = inp[0].detach()
        xp = F.pad(xin, (p, p, p, p), value=float("-inf"))
        win = xp.unfold(2, k, s).unfold(3, k, s).reshape(xp.shape[0], xp.shape[1], -1, k * k)
        top = win.topk(2, dim=-1).values
        live = top[..., 0] > 0
        seen["pool"] = min(seen["pool"], ((top[..., 0] - top[..., 1])[live].min() / xin.max()).item())
    for m in net64.modules():
        if isinstance(m, nn.ReLU):
            hooks.append(m.register_forward_pre_hook(relu_hook))
        if isinstance(m, nn.MaxPool2d):
            hooks.append(m.register_forward_pre_hook(pool_hook))
    with torch.no_grad():
        net64(x64)
    for h in hooks:
        h.remove()
    return seen["relu"], seen["pool"]


def passes(net, x, d_feat, m2i, hooked_cls):
    """{pass: (n_maps, cin, H, W)} in the net's dtype, one fresh sample tensor per map, and the deviation of the stem-only
    restatement from the reference's hook path"""
    res = {k: [] for k in PASSES}
    dev = 0.
    for m, img in enumerate(m2i):
        xs, g = x[img:img + 1], d_feat[m:m + 1]
        res["plain"].append(chain(net, xs, g, None)[0])
        res["all"].append(chain(net, xs, g, "all")[0])
        enc = copy.deepcopy(net)                                   # explain_cnn, models/gridTDmodel.py:1705-1716
        enc.zero_grad()
        hooked_cls.register_hooks(None, enc)
        sample = xs.clone()
        sample.requires_grad = True
        with torch.enable_grad():
            enc(sample).backward(g.clone(), retain_graph=True)
        ref = sample.grad.detach().clone()
        res["stem"].append(ref[0])
        dev = max(dev, ((chain(net, xs, g, "stem") - ref).abs().max() / ref.abs().max()).item())
        auto = copy.deepcopy(net)                                   # the plain pass is autograd itself
        sample = xs.clone().requires_grad_(True)
        with torch.enable_grad():
            auto(sample).backward(g.clone())
        assert torch.equal(sample.grad, res["plain"][-1][None]) or \
            ((sample.grad - res["plain"][-1][None]).abs().max() / sample.grad.abs().max()).item() < 1e-6
    return {k: torch.stack(v).numpy() for k, v in res.items()}, dev


def gen(name, cfg, rn, hooked_cls, first_seed):
    m2i = cfg["map2img"]
    for seed in range(first_seed, first_seed + 100000):
        rs = np.random.RandomState(seed)
        x = rs.standard_normal(cfg["shape"]).astype(np.float32)
        relu_m, pool_m = margins(grad_net(seed, rn.Add, cfg).double(), torch.from_numpy(x).double())
        if relu_m < MARGIN or pool_m < MARGIN:
            continue
        with torch.no_grad():
            oshape = tuple(grad_net(seed, rn.Add, cfg)(torch.from_numpy(x)).shape)
        d_feat = rs.standard_normal((len(m2i),) + oshape[1:]).astype(np.float32)
        out, e32 = {}, 0.
        for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
            net = grad_net(seed, rn.Add, cfg).to(dtype)
            res, dev = passes(net, torch.from_numpy(x).to(dtype), torch.from_numpy(d_feat).to(dtype), m2i, hooked_cls)
            assert dev < 1e-5, ("the stem-only restatement left the reference's hook path", dtype, dev)
            for k, v in res.items():
                out[k + tag] = v
        rows = np.array([[np.abs(a.astype(np.float64) - b).max() / np.abs(b).max() for a, b in zip(out[k + "32"], out[k + "64"])]
                         for k in PASSES])
        e32 = rows.max()
        del out["all32"]          # the restatement's fp32 maps: their e32 is kept in e32_rows, the file stays under the size limit
        cut = cut_fraction(grad_net(seed, rn.Add, cfg).double(), torch.from_numpy(x).double())
        print("%s seed %d: relu margin %.2e, pool margin %.2e, e32 %.2e, stem restatement %.1e, Add outputs cut %.0f%% .. %.0f%%"
              % (name, seed, relu_m, pool_m, e32, dev, 100 * min(cut), 100 * max(cut)))
        if e32 < 1e-5:
            g = dict(x=x, d_feat=d_feat, map2img=np.asarray(m2i, dtype=np.int32), seed=np.int64(seed), e32=np.float64(e32), e32_rows=rows,
                     relu_margin=np.float64(relu_m), pool_margin=np.float64(pool_m), **out)
            return {name + "_" + k: v for k, v in g.items()}
    raise SystemExit("no seed met the conditioning recipe")


def cut_fraction(net64, x64):
    """fraction of zero outputs of each block (the Add's ReLU cut them)"""
    with torch.no_grad():
        a = net64.maxpool(net64.relu(net64.bn1(net64.conv1(x64))))
        cut = []
        for blk in net64.layers:
            a = blk(a)
            cut.append((a == 0).double().mean().item())
    return cut


def main():
    install_stubs()
    import models.resnet as rn
    from models.gridTDmodel import ExplainiGridTDGuidedGradient
    g = {}
    for name, cfg in NETS.items():
        g.update(gen(name, cfg, rn, ExplainiGridTDGuidedGradient, 1))
    path = os.path.join(HERE, "resnet_grad.npz")
    np.savez_compressed(path, **g)
    print("resnet_grad.npz:", os.path.getsize(path), "bytes on disk;", {k: np.asarray(v).shape for k, v in g.items()})


if __name__ == "__main__":
    main()
