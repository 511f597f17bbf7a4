#!/usr/bin/env python3
"""Golden vectors of LRP through the reference's bottleneck ResNet encoders (models/resnet.py resnet50 / resnet101): the Conv2d rule
at the geometries only a ResNet has (7x7 s2 p3, 1x1, 1x1 s2, 3x3 s2 p1, a rectangular kernel), the MaxPool2d rule at the stem's
MaxPool2d(3, 2, 1) and other windows, and add_lrp / compute_lrp on a small bottleneck net.  Runs the REFERENCE implementation
(LRPtools/lrp_modules.py, LRPtools/lrp_wrapper.py) on seeded synthetic inputs, once in fp32 and once on .double() copies, and writes
tests/golden/resnet_rules.npz and tests/golden/resnet_tiny.npz - arrays only.

    python tests/golden/make_golden_resnet.py

Same harness shims as make_golden.py (install_stubs); run where the reference is available only.  `bottleneck_net` is imported by the
tests (it needs no reference)."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from make_golden import install_stubs

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (kernel, stride, padding, cin, cout, (H, W), input kind)
CONV_CASES = {
    "stem7": ((7, 7), (2, 2), (3, 3), 3, 24, (37, 33), "signed"),
    "pw": ((1, 1), (1, 1), (0, 0), 48, 80, (7, 7), "relu_zero"),
    "pw_s2": ((1, 1), (2, 2), (0, 0), 48, 80, (9, 8), "relu"),
    "c3_s2": ((3, 3), (2, 2), (1, 1), 40, 72, (9, 8), "relu"),
    "c3_s2_signed": ((3, 3), (2, 2), (1, 1), 40, 72, (9, 8), "signed"),
    "rect": ((1, 3), (1, 2), (0, 1), 16, 24, (6, 9), "relu"),
}
SHARED_WEIGHTS = {"c3_s2_signed": "c3_s2"}      # the same layer on another input: its _w / _b arrays are stored once
# (conv case, alpha, beta, ignore_bias) of the general rule
GENERAL_CASES = [("c3_s2", 2., 1., True), ("pw", 2., 1., False), ("pw", 1., 0., False)]
# name: (kernel, stride, padding, ceil_mode, (C, H, W), input kind)
POOL_CASES = {
    "mp321_signed": (3, 2, 1, False, (5, 9, 8), "special"),
    "mp321_relu": (3, 2, 1, False, (5, 9, 8), "relu"),
    "mp311": (3, 1, 1, False, (4, 7, 6), "signed"),
    "mp320_ceil": (3, 2, 0, True, (4, 8, 8), "signed"),
    "mp22_odd": (2, 2, 0, False, (4, 7, 7), "signed"),
}
TINY = dict(base=8, blocks=[2, 1], shape=(2, 3, 38, 34))


def general_tag(name, alpha, beta, ignore_bias):
    return "%s_a%g_b%g_%s" % (name, alpha, beta, "nobias" if ignore_bias else "bias")


def bottleneck_net(rs, add_cls, base, blocks, head=True):
    """A bottleneck ResNet in the layout of models/resnet.py (ResNet + Bottleneck, :93-140, :143-236), weights drawn from the numpy
    RandomState `rs`: 7x7 s2 p3 stem conv, BN, ONE in-place ReLU per container called for every activation in it, MaxPool2d(3, 2, 1);
    blocks of 1x1 / 3x3 (stride) / 1x1 convs with BNs, a 1x1 (stride) + BN shortcut where the shapes change and an explicit `add_cls()`
    member; with `head` the AdaptiveAvgPool2d + Linear leaves the reference's class carries and its forward never calls.
    base=64, blocks=[3, 4, 6, 3] is the ResNet-50 shape.  Convs are He-scaled.  The BNs that feed an Add have gamma in [0.1, 0.2] and
    beta in [2, 3]: both summands of every Add are then positive, away from the x1 + x2 ~ 0 pole of the Add rule where fp32 itself is
    2e-4 from fp64 (two CPU conv back-ends differ by 3.5e-4 there)."""
    def conv(cin, cout, k, stride=1, padding=0):
        m = nn.Conv2d(cin, cout, k, stride=stride, padding=padding, bias=False)
        m.weight.data = torch.from_numpy((rs.standard_normal(m.weight.shape) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32))
        return m

    def bn(c, feeds_add=False):
        m = nn.BatchNorm2d(c)
        if feeds_add:
            g, b = rs.uniform(0.1, 0.2, c), rs.uniform(2.0, 3.0, c)
        else:
            g, b = rs.uniform(0.5, 1.5, c), rs.standard_normal(c) * 0.2
        m.weight.data, m.bias.data = torch.from_numpy(g.astype(np.float32)), torch.from_numpy(b.astype(np.float32))
        m.running_mean = torch.from_numpy((rs.standard_normal(c) * 0.2).astype(np.float32))
        m.running_var = torch.from_numpy(rs.uniform(0.5, 1.5, c).astype(np.float32))
        return m

    class Block(nn.Module):
        def __init__(self, cin, planes, stride):
            super().__init__()
            self.conv1, self.bn1 = conv(cin, planes, 1), bn(planes)
            self.conv2, self.bn2 = conv(planes, planes, 3, stride, 1), bn(planes)
            self.conv3, self.bn3 = conv(planes, 4 * planes, 1), bn(4 * planes, True)
            self.relu = nn.ReLU(inplace=True)
            self.downsample = None
            if stride != 1 or cin != 4 * planes:
                self.downsample = nn.Sequential(conv(cin, 4 * planes, 1, stride), bn(4 * planes, True))
            self.add = add_cls()

        def forward(self, x):
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
            identity = x if self.downsample is None else self.downsample(x)
            return self.relu(self.add(out, identity))

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1 = conv(3, base, 7, 2, 3), bn(base)
            self.relu = nn.ReLU(inplace=True)
            self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
            layers, cin = [], base
            for i, nb in enumerate(blocks):
                planes = base << i
                for b in range(nb):
                    layers.append(Block(cin, planes, 2 if (b == 0 and i > 0) else 1))
                    cin = 4 * planes
            self.layers = nn.Sequential(*layers)
            if head:
                self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
                self.fc = nn.Linear(cin, 10)
                self.fc.weight.data = torch.from_numpy((rs.standard_normal(self.fc.weight.shape) * 0.1).astype(np.float32))
                self.fc.bias.data = torch.from_numpy((rs.standard_normal(self.fc.bias.shape) * 0.1).astype(np.float32))

        def forward(self, x):
            return self.layers(self.maxpool(self.relu(self.bn1(self.conv1(x)))))

    return Net().eval()


def leaf_signature(model):
    """{(type name, kernel, stride, padding)} over the leaf modules"""
    pair = lambda v: None if v is None else (tuple(v) if isinstance(v, (tuple, list)) else (v, v))
    return {(type(m).__name__,) + tuple(pair(getattr(m, a, None)) for a in ("kernel_size", "stride", "padding"))
            for m in model.modules() if len(list(m.children())) == 0}


def conv_case_arrays(rs, name):
    (kh, kw), _, _, cin, cout, (h, w), kind = CONV_CASES[name]
    wt = (rs.standard_normal((cout, cin, kh, kw)) * np.sqrt(2.0 / (cin * kh * kw))).astype(np.float32)
    b = (rs.standard_normal((cout,)) * 0.03).astype(np.float32)
    x = rs.standard_normal((2, cin, h, w)).astype(np.float32)
    if kind != "signed":
        x = np.maximum(x, 0.0)
    if kind == "relu_zero":
        x[0, :, :2] = 0.0          # Z == 0 there without bias: the safe_divide path
    return wt, b, x


def make_conv(name, wt, b):
    k, s, p, cin, cout, _, _ = CONV_CASES[name]
    conv = nn.Conv2d(cin, cout, k, stride=s, padding=p)
    conv.weight.data, conv.bias.data = torch.from_numpy(wt.copy()), torch.from_numpy(b.copy())
    return conv


def pool_input(rs, name):
    _, _, _, _, (c, h, w), kind = POOL_CASES[name]
    x = rs.standard_normal((2, c, h, w)).astype(np.float32)
    if kind == "relu":
        x = np.maximum(x, 0.0)
    if kind == "special":
        x[0, 0, :4, :4] = 0.0              # an all-zero region: Z == 0, safe_divide
        x[0, 1, :7] = np.minimum(x[0, 1, :7], 1.0)
        x[0, 1, 2:5, 3:6] = 1.75           # a 3 x 3 block of one repeated value above everything near it: first-maximum order
        x[1, 2, 3:7, 3:7] = -np.abs(x[1, 2, 3:7, 3:7]) - 0.1     # holds whole windows of negative values (window rows 3..5 / 5..7)
    return x


def gen_rules(lrp_modules):
    g = {}
    rs = np.random.RandomState(4101)
    params = {"alpha": 1., "beta": 0., "ignore_bias": True}

    def conv_rule(conv, x, r_out, p, dtype):
        conv = conv.to(dtype)
        xin = torch.from_numpy(x.copy()).to(dtype)
        conv.input = (xin,)
        r = lrp_modules.Conv2d().propagate_relevance(conv, (xin, conv.weight), (torch.from_numpy(r_out.copy()).to(dtype),),
                                                     'alpha_beta', p)[0]
        return r.detach().numpy()

    store = {}
    for name in CONV_CASES:
        wt, b, x = conv_case_arrays(rs, name)
        if name in SHARED_WEIGHTS:
            wt, b = store[SHARED_WEIGHTS[name]][:2]
        conv = make_conv(name, wt, b)
        with torch.no_grad():
            oshape = conv(torch.from_numpy(x)).shape
        r_out = rs.standard_normal(tuple(oshape)).astype(np.float32)
        store[name] = (wt, b, x, r_out)
        g[name + "_x"], g[name + "_rout"] = x, r_out
        if name not in SHARED_WEIGHTS:
            g[name + "_w"], g[name + "_b"] = wt, b
        g[name + "_rin"] = conv_rule(make_conv(name, wt, b), x, r_out, params, torch.float32)
        g[name + "_rin64"] = conv_rule(make_conv(name, wt, b), x, r_out, params, torch.float64)
    for name, alpha, beta, ignore_bias in GENERAL_CASES:
        wt, b, x, r_out = store[name]
        p = {"alpha": alpha, "beta": beta, "ignore_bias": ignore_bias}
        tag = general_tag(name, alpha, beta, ignore_bias)
        g[tag + "_rin"] = conv_rule(make_conv(name, wt, b), x, r_out, p, torch.float32)
        g[tag + "_rin64"] = conv_rule(make_conv(name, wt, b), x, r_out, p, torch.float64)
    for name, (k, s, p, ceil_mode, _, _) in POOL_CASES.items():
        x = pool_input(rs, name)
        pool = nn.MaxPool2d(k, s, p, ceil_mode=ceil_mode)
        r_out = rs.standard_normal(tuple(pool(torch.from_numpy(x)).shape)).astype(np.float32)
        g[name + "_x"], g[name + "_rout"] = x, r_out
        for dtype, key in ((torch.float32, "_rin"), (torch.float64, "_rin64")):
            pool.input = (torch.from_numpy(x.copy()).to(dtype),)
            g[name + key] = lrp_modules.Pool2d().propagate_relevance(pool, None, (torch.from_numpy(r_out.copy()).to(dtype),),
                                                                     'alpha_beta', params)[0].detach().numpy()
    np.savez_compressed(os.path.join(HERE, "resnet_rules.npz"), **g)
    print("resnet_rules.npz:", sum(v.nbytes for v in g.values()), "bytes,", len(g), "arrays")
    for name in list(CONV_CASES) + [general_tag(*c) for c in GENERAL_CASES] + list(POOL_CASES):
        a, b = g[name + "_rin"].astype(np.float64), g[name + "_rin64"]
        print("  %-24s e32 = %.2e" % (name, np.abs(a - b).max() / np.abs(b).max()))


def conditioning(net64, x64):
    """(min |x1 + x2| / (|x1| + |x2|) over every Add, min relative lead of a pool window's winner over its runner-up) of one fp64
    forward; windows whose two largest values are both zero do not count"""
    seen = {"add": np.inf, "pool": np.inf}
    hooks = []

    def add_hook(m, inp, out):
        a, b = inp
        den = a.abs() + b.abs()
        seen["add"] = min(seen["add"], ((a + b).abs() / den)[den > 0].min().item())

    def pool_hook(m, inp, out):
        k, s, p = m.kernel_size, m.stride, m.padding
        xp = F.pad(inp[0], (p, p, p, p), value=float("-inf"))
        win = xp.unfold(2, k, s).unfold(3, k, s).reshape(xp.shape[0], xp.shape[1], -1, k * k)
        top = win.topk(2, dim=-1).values
        live = ~((top[..., 0] == 0) & (top[..., 1] == 0))
        lead = (top[..., 0] - top[..., 1]) / top[..., 0].abs()
        seen["pool"] = min(seen["pool"], lead[live].min().item())
    for m in net64.modules():
        if type(m).__name__ == "Add":
            hooks.append(m.register_forward_hook(add_hook))
        if isinstance(m, nn.MaxPool2d):
            hooks.append(m.register_forward_hook(pool_hook))
    with torch.no_grad():
        net64(x64)
    for h in hooks:
        h.remove()
    return seen["add"], seen["pool"]


def gen_tiny(lrp_wrapper, rn):
    for seed in range(31, 63):
        rs = np.random.RandomState(seed)
        x = rs.standard_normal(TINY["shape"]).astype(np.float32)
        net = bottleneck_net(np.random.RandomState(seed), rn.Add, TINY["base"], TINY["blocks"])
        with torch.no_grad():
            oshape = tuple(net(torch.from_numpy(x)).shape)
        t1, t2 = rs.standard_normal(oshape).astype(np.float32), rs.standard_normal(oshape).astype(np.float32)
        add_min, pool_min = conditioning(bottleneck_net(np.random.RandomState(seed), rn.Add, TINY["base"], TINY["blocks"]).double(),
                                         torch.from_numpy(x).double())
        res = {}
        for dtype, tag in ((torch.float32, ""), (torch.float64, "64")):
            net = bottleneck_net(np.random.RandomState(seed), rn.Add, TINY["base"], TINY["blocks"]).to(dtype)
            lrp_wrapper.add_lrp(net)
            xs = torch.from_numpy(x.copy()).to(dtype)
            res["r1" + tag] = net.compute_lrp(xs, target=torch.from_numpy(t1.copy()).to(dtype)).numpy()
            res["r2" + tag] = net.compute_lrp(xs, target=torch.from_numpy(t2.copy()).to(dtype)).numpy()     # the .grad running sum
        e32 = max(np.abs(res[k] - res[k + "64"]).max() / np.abs(res[k + "64"]).max() for k in ("r1", "r2"))
        print("seed %d: min |x1+x2|/(|x1|+|x2|) %.3f, min pool lead %.2e, e32 %.2e" % (seed, add_min, pool_min, e32))
        if add_min >= 0.1 and pool_min >= 1e-3 and e32 < 1e-5:
            g = dict(x=x, target1=t1, target2=t2, seed=np.int64(seed), e32=np.float64(e32), **res)
            np.savez_compressed(os.path.join(HERE, "resnet_tiny.npz"), **g)
            print("resnet_tiny.npz:", sum(np.asarray(v).nbytes for v in g.values()), "bytes;", {k: np.asarray(v).shape for k, v in g.items()})
            return
    raise SystemExit("no seed met the conditioning recipe")


def main():
    install_stubs()
    from LRPtools import lrp_modules, lrp_wrapper
    import models.resnet as rn
    want = leaf_signature(rn.resnet50(pretrained=False))      # (its default loads a checkpoint file)
    got = leaf_signature(bottleneck_net(np.random.RandomState(0), rn.Add, 64, [3, 4, 6, 3], head=True))
    assert want == got, (sorted(want - got, key=str), sorted(got - want, key=str))
    print("leaf (type, kernel, stride, padding) set of models.resnet.resnet50() == bottleneck_net(64, [3,4,6,3]):", len(got), "entries")
    gen_rules(lrp_modules)
    gen_tiny(lrp_wrapper, rn)


if __name__ == "__main__":
    main()
