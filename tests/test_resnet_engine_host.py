"""Host-side logic of the batched bottleneck-ResNet encoder engine (no GPU): the structure matcher and its layer plan, the new
entry points of the C ABI, and - in plain torch fp64 - the COEFFICIENT FORMULATION the kernels rely on: per image, precompute for
every conv q = BN-rule fraction / safe(Z+) and for every Add its two split coefficients; per map, run transposed convs only.  It must
reproduce the reference's own fp64 result on tests/golden/resnet_tiny.npz."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import lrp_amd  # noqa: F401
from lrp_amd import _lib, ops
from lrp_amd.LRPtools import lrp_modules

from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet import TINY, bottleneck_net  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lrpx_conv_geom_ex", "lrpx_resnet_bn_act_coef", "lrpx_resnet_add_relu_coef", "lrpx_resnet_maxpool_fwd",
               "lrpx_resnet_maxpool_rel", "lrpx_resnet_add_split", "lrpx_resnet_stem_fold")


def _net(base, blocks, seed=3, **kw):
    return bottleneck_net(np.random.RandomState(seed), lrp_modules.resAdd, base, blocks, **kw)


# ---- matcher ------------------------------------------------------------------------------------------------------------------------------
class _LayeredNet(nn.Module):
    """the reference's layout: layer1 .. layer4 containers and the unused head (models/resnet.py:164-177)"""

    def __init__(self):
        super().__init__()
        src = _net(8, [1, 1, 1, 1])
        self.conv1, self.bn1, self.relu, self.maxpool = src.conv1, src.bn1, src.relu, src.maxpool
        for i in range(4):
            setattr(self, "layer%d" % (i + 1), nn.Sequential(src.layers[i]))
        self.avgpool, self.fc = src.avgpool, src.fc


class _BasicBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(c, c, 3, padding=1, bias=False), nn.BatchNorm2d(c)
        self.relu = nn.ReLU(inplace=True)
        self.conv2, self.bn2 = nn.Conv2d(c, c, 3, padding=1, bias=False), nn.BatchNorm2d(c)
        self.downsample = None


def _basic_net():
    net = _net(8, [1])
    net.layers = nn.Sequential(_BasicBlock(8))
    return net.eval()


def _vgg16():
    layers, cin = [], 3
    for v in [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512]:
        if v == 'M':
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers).eval()


def _with_conv2(**kw):
    net = _net(8, [1])
    net.layers[0].conv2 = nn.Conv2d(8, 8, 3, **kw)
    return net


@pytest.mark.parametrize("make", [lambda: _net(8, [2, 1]), lambda: _net(64, [3, 4, 6, 3]), _LayeredNet],
                         ids=["tiny", "resnet50_shape", "layer1_to_layer4"])
def test_matcher_accepts_bottleneck_resnets(make):
    net = make()
    plan = ops.match_bottleneck_resnet(net)
    n_blocks = sum(1 for m in net.modules() if hasattr(m, "conv3"))
    assert len(plan.blocks) == n_blocks
    assert len(plan.convs) == 1 + 3 * n_blocks + sum(1 for b in plan.blocks if b["downsample"] is not None)


@pytest.mark.parametrize("make,cause", [
    (_basic_net, "BasicBlock"),
    (_vgg16, "stem"),
    (lambda: _net(8, [2, 1]).train(), "training mode"),
    (lambda: _with_conv2(padding=2, dilation=2, bias=False), "dilation"),
    (lambda: _with_conv2(padding=1, groups=2, bias=False), "groups"),
    (lambda: _with_conv2(padding=1, bias=True), "bias"),
], ids=["basic_block", "vgg16", "train", "dilation", "groups", "bias"])
def test_matcher_refuses_and_names_the_cause(make, cause):
    with pytest.raises(ValueError, match=cause):
        ops.match_bottleneck_resnet(make())


def test_encoder_refuses_a_model_that_is_not_on_the_gpu():
    with pytest.raises(ValueError, match="GPU"):
        ops.ResNetEncoder(_net(8, [2, 1]))


def test_layer_plan_of_the_tiny_net():
    plan = ops.match_bottleneck_resnet(_net(TINY["base"], TINY["blocks"]))
    pw, c3, c3s2, pws2 = (1, 1, 1, 1, 0, 0), (3, 3, 1, 1, 1, 1), (3, 3, 2, 2, 1, 1), (1, 1, 2, 2, 0, 0)
    want = [("conv1", 3, 8, (7, 7, 2, 2, 3, 3), "image"),
            ("layers.0.conv1", 8, 8, pw, "maxpool(relu)"), ("layers.0.conv2", 8, 8, c3, "relu"), ("layers.0.conv3", 8, 32, pw, "relu"),
            ("layers.0.downsample.0", 8, 32, pw, "maxpool(relu)"),
            ("layers.1.conv1", 32, 8, pw, "relu"), ("layers.1.conv2", 8, 8, c3, "relu"), ("layers.1.conv3", 8, 32, pw, "relu"),
            ("layers.2.conv1", 32, 16, pw, "relu"), ("layers.2.conv2", 16, 16, c3s2, "relu"), ("layers.2.conv3", 16, 64, pw, "relu"),
            ("layers.2.downsample.0", 32, 64, pws2, "relu")]
    got = [(c["name"], c["cin"], c["cout"], c["geom"], c["producer"]) for c in plan.convs]
    assert got == want
    # non-negative inputs by structure: every conv but the stem
    assert [c["nonneg"] for c in plan.convs] == [False] + [True] * 11
    assert [(b["name"], b["downsample"] is not None) for b in plan.blocks] == [("layers.0", True), ("layers.1", False), ("layers.2", True)]
    assert [(b["conv1"], b["conv2"], b["conv3"], b["downsample"]) for b in plan.blocks] == [(1, 2, 3, 4), (5, 6, 7, None), (8, 9, 10, 11)]
    assert plan.pool == (3, 3, 2, 2, 1, 1)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lrpx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lrpx_[a-z0-9_]+)\s*\(", src))
    for s in NEW_SYMBOLS:
        assert s in declared, s + " is not declared in include/lrpx.h"
        assert s in _lib.SIGNATURES, s + " is not bound in _lib.py"
    assert "lrpx_conv_geom_ex_desc" in src
    assert os.path.exists(_lib.LIB_PATH), "liblrpx.so not built (run __graft_entry__.build())"
    lib = _lib.load()
    assert lib.lrpx_version() == 101            # the capability is detected by the symbols, not by the number
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)


def test_new_entry_points_validate_on_the_host():
    assert os.path.exists(_lib.LIB_PATH), "liblrpx.so not built (run __graft_entry__.build())"
    lib = _lib.load()
    assert lib.lrpx_conv_geom_ex(None, None) == _lib.EINVAL
    assert b"null" in lib.lrpx_last_error_string()
    assert lib.lrpx_conv_geom_ex(C.byref(_lib.ConvGeomExDesc()), None) == _lib.EINVAL
    assert lib.lrpx_resnet_bn_act_coef(None, 8, None, None, None, None, 4, 4, 1, None) == _lib.EINVAL
    assert lib.lrpx_resnet_add_relu_coef(None, None, None, None, None, 4, None) == _lib.EINVAL
    assert lib.lrpx_resnet_maxpool_fwd(None, None, 1, 8, 8, 4, 4, 4, 3, 3, 2, 2, 1, 1, None) == _lib.EINVAL
    assert lib.lrpx_resnet_maxpool_rel(None, None, None, None, 1, 1, 8, 8, 4, 4, 4, 3, 3, 2, 2, 1, 1, None) == _lib.EINVAL
    assert lib.lrpx_resnet_add_split(None, None, None, None, None, None, 1, 1, 4, None) == _lib.EINVAL
    assert lib.lrpx_resnet_stem_fold(None, None, 1, 3, 3, 8, 4, None) == _lib.EINVAL
    assert b"null" in lib.lrpx_last_error_string()


# ---- the coefficient formulation in fp64 --------------------------------------------------------------------------------------------------
def _safe(z):
    return z + 1e-7 * (z == 0).to(z.dtype)


def coefficient_trace(plan, x):
    """per IMAGE: activations, q per conv, (c1, c2) per Add.  NCHW fp64."""
    act, q = {}, {}

    def conv(i, inp, relu):
        cv = plan.convs[i]
        kh, kw, sh, sw, ph, pw = cv["geom"]
        wt, bn = cv["module"].weight.detach(), cv["bn"]
        wp, wn = wt.clamp(min=0), wt.clamp(max=0)
        kw_ = dict(stride=(sh, sw), padding=(ph, pw))
        y = F.conv2d(inp, wt, **kw_)
        if cv["nonneg"]:
            z = F.conv2d(inp, wp, **kw_)
        else:
            z = F.conv2d(inp.clamp(min=0), wp, **kw_) + F.conv2d(inp.clamp(max=0), wn, **kw_)
        sd = torch.sqrt(bn.running_var + bn.eps)
        w = (bn.weight.detach() / sd)[:, None, None]
        b = (bn.bias.detach() - (bn.running_mean * bn.weight.detach()) / sd)[:, None, None]
        xw = (y * w).abs()
        q[i] = xw / _safe(xw + b.abs()) / _safe(z)
        a = y * w + b
        act[i] = a.clamp(min=0) if relu else a
        return act[i]
    pk = plan.pool
    a0 = conv(0, x, True)
    pooled, pool_idx = F.max_pool2d(a0, pk[:2], pk[2:4], pk[4:], return_indices=True)
    outs, coef = [], []
    cur = pooled
    for blk in plan.blocks:
        y3 = conv(blk["conv3"], conv(blk["conv2"], conv(blk["conv1"], cur, True), True), False)
        short = conv(blk["downsample"], cur, False) if blk["downsample"] is not None else cur
        s = y3 + short
        half = 0.5 * (s == 0).to(s.dtype)
        den = s + 0.01 * s.sign()
        coef.append((torch.nan_to_num(y3 / den, nan=0.0) + half, torch.nan_to_num(short / den, nan=0.0) + half))
        cur = s.clamp(min=0)
        outs.append(cur)
    return dict(x=x, act=act, q=q, pooled=pooled, pool_idx=pool_idx, outs=outs, coef=coef)


def coefficient_relevance(plan, tr, r, img):
    """per MAP: multiplications by the image's coefficients and transposed convs only"""
    sel = lambda t: t[img:img + 1]

    def convT(i, r_out, x_in, signed=False):
        cv = plan.convs[i]
        kh, kw, sh, sw, ph, pw = cv["geom"]
        wt = cv["module"].weight.detach()
        s = r_out * sel(tr["q"][i])
        back = lambda w_: torch.nn.grad.conv2d_input(x_in.shape, w_, s, stride=(sh, sw), padding=(ph, pw))
        if signed:
            return x_in.clamp(min=0) * back(wt.clamp(min=0)) + x_in.clamp(max=0) * back(wt.clamp(max=0))
        return x_in * back(wt.clamp(min=0))
    for bi in range(len(plan.blocks) - 1, -1, -1):
        blk = plan.blocks[bi]
        x_in = sel(tr["outs"][bi - 1] if bi > 0 else tr["pooled"])
        c1, c2 = tr["coef"][bi]
        r1, r2 = r * sel(c1), r * sel(c2)
        rb = convT(blk["conv2"], convT(blk["conv3"], r1, sel(tr["act"][blk["conv2"]])), sel(tr["act"][blk["conv1"]]))
        if blk["downsample"] is not None:
            r2 = convT(blk["downsample"], r2, x_in)
        r = convT(blk["conv1"], rb, x_in) + r2
    a0 = sel(tr["act"][0])
    s = r / _safe(sel(tr["pooled"]))
    grad = torch.zeros_like(a0).flatten(2).scatter_add_(2, sel(tr["pool_idx"]).flatten(2), s.flatten(2)).view(a0.shape)
    return convT(0, a0 * grad, sel(tr["x"]), signed=True)


def test_coefficient_formulation_reproduces_the_reference_in_fp64():
    T = dict(np.load(os.path.join(GOLDEN, "resnet_tiny.npz")))
    net = _net(TINY["base"], TINY["blocks"], seed=int(T["seed"])).double()
    plan = ops.match_bottleneck_resnet(net)
    with torch.no_grad():
        tr = coefficient_trace(plan, torch.from_numpy(T["x"]).double())
        assert torch.allclose(tr["outs"][-1], net(torch.from_numpy(T["x"]).double()), rtol=0, atol=1e-12)
        for key, want in (("target1", T["r164"]), ("target2", T["r264"] - T["r164"])):
            t = torch.from_numpy(T[key]).double()
            for img in range(t.shape[0]):
                got = coefficient_relevance(plan, tr, t[img:img + 1], img)[0]
                e = (got - torch.from_numpy(want[img])).abs().max().item() / np.abs(want[img]).max()
                print(f"coefficient formulation {key} image {img}: {e:.2e} of the map's maximum")
                assert e < 1e-9, (key, img, e)
