"""LRP through the reference's bottleneck ResNet encoders on the GPU: the Conv2d rule on the runtime-geometry engine
(csrc/conv_geom.hip), the MaxPool2d rule at any window (csrc/lrpx_rules.hip) and add_lrp / compute_lrp on a bottleneck net, against
the reference's own results (tests/golden/resnet_rules.npz, resnet_tiny.npz: make_golden_resnet.py) and - at production shapes -
against the rule's formula in fp64.

Conv criterion (tests/fp64_anchor.py): rel_err(got, fp64) <= C * max(rel_err(fp32 reference, fp64), FLOOR) with the project's measured
grade of fp32-MFMA relevance kernels, C = 6, FLOOR = 1e-7.  Pool criterion: C * FLOOR, exact zeros where the reference has exact
zeros and the same set of non-zero positions (a winner mistake is an O(1) error)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import lrp_amd  # noqa: F401
from conftest import GOLDEN, rel_err
from fp64_anchor import C, FLOOR

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet import (CONV_CASES, GENERAL_CASES, POOL_CASES, SHARED_WEIGHTS, TINY, bottleneck_net,  # noqa: E402
                                general_tag)

_G = {}


def golden(name):
    if name not in _G:
        _G[name] = dict(np.load(os.path.join(GOLDEN, name)))
    return _G[name]


def _modules():
    from lrp_amd.LRPtools import lrp_modules, lrp_wrapper
    return lrp_modules, lrp_wrapper


def run_conv_rule(w, b, x, r_out, stride, padding, params):
    lrp_modules, _ = _modules()
    cout, cin, kh, kw = w.shape
    conv = nn.Conv2d(cin, cout, (kh, kw), stride=stride, padding=padding, bias=b is not None)
    conv.weight.data = torch.as_tensor(w).clone()
    if b is not None:
        conv.bias.data = torch.as_tensor(b).clone()
    conv = conv.cuda()
    conv.input = (torch.as_tensor(x).cuda(),)
    r = lrp_modules.Conv2d().propagate_relevance(conv, None, (torch.as_tensor(r_out).cuda(),), "alpha_beta", params)[0]
    torch.cuda.synchronize()
    return r.cpu()


def run_pool_rule(pool, x, r_out):
    lrp_modules, _ = _modules()
    pool.input = (torch.as_tensor(x).cuda(),)
    r = lrp_modules.Pool2d().propagate_relevance(pool, None, (torch.as_tensor(r_out).cuda(),), "alpha_beta", None)[0]
    torch.cuda.synchronize()
    return r.cpu()


def assert_fp32_grade(got, ref64, ref32, what):
    e, e32 = rel_err(got, ref64), rel_err(ref32, ref64)
    bound = C * max(e32, FLOOR)
    print(f"resnet conv {what}: e {e:.2e}  e32 {e32:.2e}  e/max(e32,FLOOR) {e / max(e32, FLOOR):.2f}  bound {bound:.2e}")
    assert e <= bound, f"{what}: rel_err vs fp64 {e:.3e} > {C} x max(fp32's {e32:.3e}, {FLOOR:.0e})"


def assert_pool_grade(got, ref64, what):
    ref64 = torch.as_tensor(ref64)
    e = rel_err(got, ref64)
    print(f"resnet pool {what}: e {e:.2e}  e/FLOOR {e / FLOOR:.2f}  bound {C * FLOOR:.1e}")
    assert e <= C * FLOOR, f"{what}: rel_err vs fp64 {e:.3e} > {C} x {FLOOR:.0e}"
    assert torch.equal(got != 0, ref64 != 0), f"{what}: the non-zero positions differ from the reference's"


# ---- 1. every rule fixture through the rule classes ---------------------------------------------------------------------------------
_PRESET = {"alpha": 1., "beta": 0., "ignore_bias": True}
_CONV_IDS = [(name, 1., 0., True) for name in CONV_CASES] + list(GENERAL_CASES)


@pytest.mark.parametrize("name,alpha,beta,ignore_bias", _CONV_IDS, ids=[general_tag(*c) for c in _CONV_IDS])
def test_conv_rule_fixtures(name, alpha, beta, ignore_bias):
    G = golden("resnet_rules.npz")
    _, stride, padding = CONV_CASES[name][:3]
    wname = SHARED_WEIGHTS.get(name, name)
    tag = name if (alpha, beta, ignore_bias) == (1., 0., True) else general_tag(name, alpha, beta, ignore_bias)
    got = run_conv_rule(G[wname + "_w"], G[wname + "_b"], G[name + "_x"], G[name + "_rout"], stride, padding,
                        {"alpha": alpha, "beta": beta, "ignore_bias": ignore_bias})
    assert_fp32_grade(got, G[tag + "_rin64"], G[tag + "_rin"], tag)
    if name == "pw_s2":       # rows / columns no 1x1 s2 window covers: exact zeros
        assert (got[:, :, 1::2, :] == 0).all() and (got[:, :, :, 1::2] == 0).all()
        assert (got[:, :, ::2, ::2] != 0).any()


@pytest.mark.parametrize("name", list(POOL_CASES))
def test_maxpool_rule_fixtures(name):
    G = golden("resnet_rules.npz")
    k, s, p, ceil_mode = POOL_CASES[name][:4]
    got = run_pool_rule(nn.MaxPool2d(k, s, p, ceil_mode=ceil_mode), G[name + "_x"], G[name + "_rout"])
    assert_pool_grade(got, G[name + "_rin64"], name)
    assert torch.equal(got == 0, torch.as_tensor(G[name + "_rin"]) == 0)


# ---- 2. long-K and production-tile launches: the rule's formula in fp64 on the CPU ------------------------------------------------------
def conv_rule_cpu(x, w, r, stride, padding, dtype):
    """alpha 1 / beta 0 without bias (lrp_modules.py:124-150): Z = conv(x+, W+) + conv(x-, W-), R = x+ convT(S, W+) + x- convT(S, W-)"""
    x, w, r = x.to(dtype), w.to(dtype), r.to(dtype)
    xp, xn, wp, wn = x.clamp(min=0), x.clamp(max=0), w.clamp(min=0), w.clamp(max=0)
    z = F.conv2d(xp, wp, stride=stride, padding=padding) + F.conv2d(xn, wn, stride=stride, padding=padding)
    s = r / (z + 1e-7 * (z == 0).to(dtype))
    back = lambda wt: torch.nn.grad.conv2d_input(x.shape, wt, s, stride=stride, padding=padding)
    return xp * back(wp) + xn * back(wn)


@pytest.mark.parametrize("k,stride,padding,cin,cout,hw,signed", [
    (1, 1, 0, 2048, 512, 7, False), (3, 2, 1, 512, 512, 14, False), (1, 2, 0, 256, 512, 56, False), (7, 2, 3, 3, 64, 224, True),
    (1, 1, 0, 256, 64, 56, False)], ids=["pw_2048_512_7", "c3s2_512_14", "pws2_256_512_56", "stem7_224", "pw_256_64_56"])
def test_conv_rule_production_shapes(k, stride, padding, cin, cout, hw, signed):
    g = torch.Generator().manual_seed(100 + k + cin)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    x = torch.randn(1, cin, hw, hw, generator=g)
    if not signed:
        x = x.clamp(min=0)
    ohw = (hw + 2 * padding - k) // stride + 1
    r = torch.randn(1, cout, ohw, ohw, generator=g)
    got = run_conv_rule(w, None, x, r, stride, padding, _PRESET)
    ref64 = conv_rule_cpu(x, w, r, stride, padding, torch.float64)
    ref32 = conv_rule_cpu(x, w, r, stride, padding, torch.float32)
    assert_fp32_grade(got, ref64, ref32, f"{k}x{k} s{stride} {cin}->{cout} at {hw}x{hw}")


def test_maxpool_rule_production_shape():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 64, 112, 112, generator=g)
    r = torch.randn(1, 64, 56, 56, generator=g)
    got = run_pool_rule(nn.MaxPool2d(3, 2, 1), x, r)
    xd = x.double().requires_grad_(True)
    z = F.max_pool2d(xd, 3, 2, 1)
    z.backward(r.double() / (z.detach() + 1e-7 * (z.detach() == 0)))
    assert_pool_grade(got, (xd * xd.grad).detach(), "MaxPool2d(3,2,1) 64 x 112 x 112")


# ---- 3. the bottleneck net through add_lrp / compute_lrp --------------------------------------------------------------------------------
def _tiny_net(T):
    lrp_modules, _ = _modules()
    return bottleneck_net(np.random.RandomState(int(T["seed"])), lrp_modules.resAdd, TINY["base"], TINY["blocks"]).cuda()


def test_bottleneck_net_compute_lrp_vs_reference():
    """both calls on one sample tensor (the second carries the running sum) within the end-to-end criterion of SURVEY 8(d), 1e-4 of the
    map's maximum, against the reference's fp64 result; the reference's own fp32 result sits at e32 (stored, < 1e-5)"""
    _, lrp_wrapper = _modules()
    T = golden("resnet_tiny.npz")
    net = _tiny_net(T)
    lrp_wrapper.add_lrp(net)
    lrp_wrapper.add_lrp(net)                       # idempotent: never two hooks per leaf
    leaves = [m for m in net.modules() if len(list(m.children())) == 0]
    assert len(net._lrpx_hooks) == len(leaves) and all(len(m._forward_hooks) == 1 for m in leaves)
    xs = torch.from_numpy(T["x"].copy()).cuda()
    r1 = net.compute_lrp(xs, target=torch.from_numpy(T["target1"]).cuda()).cpu()
    r2 = net.compute_lrp(xs, target=torch.from_numpy(T["target2"]).cuda()).cpu()
    for got, key in ((r1, "r1"), (r2, "r2")):
        e, e32 = rel_err(got, T[key + "64"]), rel_err(T[key], T[key + "64"])
        print(f"resnet tiny net {key}: e {e:.2e}  e32 {e32:.2e}  e/e32 {e / e32:.2f}  bound 1.0e-04")
        assert e < 1e-4, (key, e)


def test_bottleneck_net_alpha2_beta1_overlay():
    _, lrp_wrapper = _modules()
    T = golden("resnet_tiny.npz")
    net = _tiny_net(T)
    target = torch.from_numpy(T["target1"]).cuda()
    lrp_wrapper.add_lrp(net)
    r_preset = net.compute_lrp(torch.from_numpy(T["x"].copy()).cuda(), target=target).cpu()
    lrp_wrapper.add_lrp(net, lrp_params={"alpha": 2., "beta": 1.})
    r_ab = net.compute_lrp(torch.from_numpy(T["x"].copy()).cuda(), target=target).cpu()
    assert torch.isfinite(r_ab).all() and r_ab.shape == r_preset.shape
    d = rel_err(r_ab, r_preset)
    print(f"resnet tiny net alpha 2 / beta 1 against the preset: {d:.2e} of the maximum")
    assert d > 1e-2


def test_a_forward_that_reaches_the_deferred_leaf_is_refused():
    _, lrp_wrapper = _modules()
    net = nn.Sequential(nn.Conv2d(3, 8, 1), nn.AdaptiveAvgPool2d(1)).cuda()
    lrp_wrapper.add_lrp(net)                       # accepted: the reference's encoders carry one and never call it
    with pytest.raises(ValueError, match="not known"):
        net.compute_lrp(torch.randn(1, 3, 6, 6).cuda(), target=torch.randn(1, 8, 1, 1).cuda())


# ---- 4. guard bands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(3, 3, 2, 2, 1, 1), (1, 1, 2, 2, 0, 0), (7, 7, 2, 2, 3, 3), (1, 3, 1, 2, 0, 1)],
                         ids=["c3s2", "pws2", "stem7", "rect"])
def test_conv_geom_never_writes_past_its_output(geom):
    """both directions write into a buffer with a sentinel band behind it, at pixel and channel counts that are no multiple of the
    64 x 64 tile; the inputs sit at the END of their allocations.  Every element of the output is written, the band stays."""
    from lrp_amd import _lib, ops
    kh, kw, sh, sw, ph, pw = geom
    g = torch.Generator().manual_seed(23)
    n, h, w, k, n_oc = 3, 11, 9, 20, 37
    oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    guard = 64 * 64
    pad = 4096

    def at_end(t):
        buf = torch.zeros(pad + t.numel(), device="cuda")
        buf[pad:] = t.flatten().cuda()
        return buf[pad:].view(t.shape)
    wt = torch.randn(n_oc, k, kh, kw, generator=g)
    pf = ops.conv_geom_pack(wt.cuda(), _lib.GEOM_FWD)
    xin = at_end(torch.randn(n, h * w, k, generator=g))
    n_out = n * oh * ow * n_oc
    buf = torch.full((n_out + guard,), 12345.0, device="cuda")
    out = buf[:n_out].view(n, oh * ow, n_oc)
    ops.conv_geom(xin, pf, _lib.GEOM_FWD, n, (h, w), (oh, ow), geom, k, n_oc, out=out)
    torch.cuda.synchronize()
    assert (buf[n_out:] == 12345.0).all() and (out != 12345.0).all() and torch.isfinite(out).all()
    want = F.conv2d(xin.view(n, h, w, k).permute(0, 3, 1, 2).cpu().double(), wt.double(), stride=(sh, sw), padding=(ph, pw))
    # (a layout check: a misplaced element is an O(1) error; fp32 chains of <= 40 * 49 terms of N(0,1) products stay below 1e-5 of the maximum)
    assert rel_err(out.view(n, oh, ow, n_oc).permute(0, 3, 1, 2).cpu(), want) < 1e-5
    # transposed: S (n, oh ow, n_oc) -> (n, h w, k), weights (cout = n_oc, cin = k)
    s_in = at_end(torch.randn(n, oh * ow, n_oc + 3, generator=g))       # K = 40: two chunks, the second partial
    wt2 = torch.randn(n_oc + 3, k, kh, kw, generator=g)
    pb = ops.conv_geom_pack(wt2.cuda(), _lib.GEOM_BWD)
    xm = at_end(torch.rand(n, h * w, k, generator=g) + 0.5)
    n_out = n * h * w * k
    buf = torch.full((n_out + guard,), 12345.0, device="cuda")
    out = buf[:n_out].view(n, h * w, k)
    ops.conv_geom(s_in, pb, _lib.GEOM_BWD, n, (h, w), (oh, ow), geom, n_oc + 3, k, x=xm, out=out)
    torch.cuda.synchronize()
    assert (buf[n_out:] == 12345.0).all() and (out != 12345.0).all() and torch.isfinite(out).all()
    s_nchw = s_in.view(n, oh, ow, n_oc + 3).permute(0, 3, 1, 2).cpu().double()
    want = torch.nn.grad.conv2d_input((n, k, h, w), wt2.double(), s_nchw, stride=(sh, sw), padding=(ph, pw))
    want = want * xm.view(n, h, w, k).permute(0, 3, 1, 2).cpu().double()
    assert rel_err(out.view(n, h, w, k).permute(0, 3, 1, 2).cpu(), want) < 1e-5
