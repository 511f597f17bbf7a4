#!/usr/bin/env python3
"""Golden vectors of the GENERAL alpha-beta Conv2d rule (beta != 0, with bias): runs the REFERENCE implementation
(LRPtools/lrp_modules.py:124-150 and, for whole nets, add_lrp / compute_lrp of LRPtools/lrp_wrapper.py with the preset's
parameters replaced) on seeded synthetic inputs and writes tests/golden/alphabeta.npz - arrays only.

    python tests/golden/make_golden_alphabeta.py

Same harness shims as make_golden.py (install_stubs); run where the reference is available only."""
import os

import numpy as np
import torch
import torch.nn as nn

from make_golden import install_stubs, toy_resnet

HERE = os.path.dirname(os.path.abspath(__file__))

# (alpha, beta, ignore_bias) of the single-rule fixtures
RULE_CASES = [(2., 1., True), (1.5, .5, True), (2., 1., False), (1., 0., False), (3., 0., True)]


def case_tag(alpha, beta, ignore_bias):
    return "a%g_b%g_%s" % (alpha, beta, "nobias" if ignore_bias else "bias")


def rule_inputs(rs):
    """{name: (weight, bias, x, r_out)}: `signed` = 4 -> 6 channels at 6 x 6, signed input with a zero region (Z == 0 there without
    bias: the safe_divide path); `relu` = 16 -> 32 channels at 14 x 14 on a post-ReLU input.  |b| ~ 0.1 against |Z| ~ 1."""
    c = {}
    w = rs.standard_normal((6, 4, 3, 3)).astype(np.float32) * 0.3
    b = rs.standard_normal((6,)).astype(np.float32) * 0.1
    x = rs.standard_normal((2, 4, 6, 6)).astype(np.float32)
    x[0, :, :2] = 0.0
    c["signed"] = (w, b, x, rs.standard_normal((2, 6, 6, 6)).astype(np.float32))
    w = rs.standard_normal((32, 16, 3, 3)).astype(np.float32) * 0.15
    b = rs.standard_normal((32,)).astype(np.float32) * 0.1
    x = np.maximum(rs.standard_normal((2, 16, 14, 14)).astype(np.float32), 0.0)
    c["relu"] = (w, b, x, rs.standard_normal((2, 32, 14, 14)).astype(np.float32))
    return c


def mini_net(rs):
    """the Conv-ReLU-Conv-ReLU-MaxPool-Conv-ReLU net of make_golden.gen_layers"""
    net = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(inplace=True),
                        nn.Conv2d(8, 8, 3, padding=1), nn.ReLU(inplace=True),
                        nn.MaxPool2d(2, 2),
                        nn.Conv2d(8, 16, 3, padding=1), nn.ReLU(inplace=True))
    for m in net:
        if isinstance(m, nn.Conv2d):
            m.weight.data = torch.from_numpy(rs.standard_normal(m.weight.shape).astype(np.float32) * 0.2)
            m.bias.data = torch.from_numpy(rs.standard_normal(m.bias.shape).astype(np.float32) * 0.1)
    return net.eval()


def main():
    install_stubs()
    from LRPtools import lrp_modules, lrp_wrapper
    import models.resnet as rn
    g = {}
    rs = np.random.RandomState(2024)
    for name, (w, b, x, r_out) in rule_inputs(rs).items():
        conv = nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1)
        conv.weight.data, conv.bias.data = torch.from_numpy(w.copy()), torch.from_numpy(b.copy())
        g[name + "_w"], g[name + "_b"], g[name + "_x"], g[name + "_rout"] = w, b, x, r_out
        for alpha, beta, ignore_bias in RULE_CASES:
            xin = torch.from_numpy(x.copy())
            conv.input = (xin,)
            params = {"alpha": alpha, "beta": beta, "ignore_bias": ignore_bias}
            rin = lrp_modules.Conv2d().propagate_relevance(conv, (xin, conv.weight), (torch.from_numpy(r_out.copy()),),
                                                           'alpha_beta', params)[0]
            g[name + "_rin_" + case_tag(alpha, beta, ignore_bias)] = rin.detach().numpy()

    def preset(ignore_bias):
        class Preset(object):
            def __init__(self):
                self.lrp_params = {"alpha": 2., "beta": 1., "ignore_bias": ignore_bias}
        return Preset

    default_preset = lrp_wrapper.SequentialPresetA
    try:
        rs = np.random.RandomState(2025)
        x = rs.standard_normal((1, 3, 16, 16)).astype(np.float32)
        x[0, :, 3, 4] = 0.0
        target = rs.standard_normal((1, 16, 8, 8)).astype(np.float32)
        target[0, 2] = 0.0
        g["mini_x"], g["mini_target"], g["mini_seed"] = x, target, np.int64(77)
        for ignore_bias in (True, False):
            lrp_wrapper.SequentialPresetA = preset(ignore_bias)
            net = mini_net(np.random.RandomState(77))
            lrp_wrapper.add_lrp(net)
            r = net.compute_lrp(torch.from_numpy(x.copy()), target=torch.from_numpy(target.copy()))
            g["mini_r_" + case_tag(2., 1., ignore_bias)] = r.numpy()
        # the toy residual net: conv2 has NO bias, so with ignore_bias=False the reference's clones keep the random bias
        # nn.Conv2d() gave them (lrp_modules.py:73-76): noise, not a fixture.  ignore_bias=True only.
        rs = np.random.RandomState(5)
        lrp_wrapper.SequentialPresetA = preset(True)
        net = toy_resnet(rs, rn.Add, rn.Flatten)
        lrp_wrapper.add_lrp(net)
        x = rs.standard_normal((2, 3, 14, 14)).astype(np.float32)
        x[1, :, 5, 6] = 0.0
        target = rs.standard_normal((2, 10)).astype(np.float32)
        target2 = rs.standard_normal((2, 10)).astype(np.float32)
        xs = torch.from_numpy(x.copy())
        r1 = net.compute_lrp(xs, target=torch.from_numpy(target.copy()))
        r2 = net.compute_lrp(xs, target=torch.from_numpy(target2.copy()))
        g.update(toy_x=x, toy_target=target, toy_target2=target2, toy_r1=r1.numpy(), toy_r2=r2.numpy(), toy_seed=np.int64(5))
    finally:
        lrp_wrapper.SequentialPresetA = default_preset
    np.savez(os.path.join(HERE, "alphabeta.npz"), **g)
    print("alphabeta.npz:", sum(v.nbytes for v in g.values()), "bytes;", {k: getattr(v, "shape", ()) for k, v in g.items()})


if __name__ == "__main__":
    main()
