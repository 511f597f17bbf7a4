"""The rule classes lrp_modules.Conv2d and Pool2d on the GPU on real modules at geometries outside ResNet-50's: nn.Conv2d(5, 6, ...) -
an odd cin exercises the half padding of the split input [x+ | x-], cout % 4 != 0 the padded relevance channels - at four geometries of
tests/conv_geom_offgeom_cases.py, under the preset and under alpha 2 / beta 1 with the bias; a 3x3 / s1 / p1 conv on a 226 x 5 map (the
branch that leaves the VGG16 kernels for the runtime-geometry engine); and a rectangular MaxPool2d through Pool2d.

Conv criterion (tests/fp64_anchor.py): rel_err(got, fp64) <= C * max(rel_err(fp32 CPU, fp64), FLOOR) against the docstring's formula in
torch fp64.  The inputs are conditioned on the CPU first, as tests/test_gpu_alphabeta.py conditions its production inputs: the first
seed at which the fp32 CPU evaluation is within 1e-6 of fp64 (with 5 input channels a Z is a sum of few terms; a bias that happens to
cancel one is a pole of R / Z, where two fp32 evaluations differ by more than any grade).  Pool criterion: assert_pool_grade."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import lrp_amd  # noqa: F401
from conftest import rel_err
from conv_geom_offgeom_cases import GEOMS
from test_gpu_resnet import assert_fp32_grade, assert_pool_grade, conv_rule_cpu, run_conv_rule, run_pool_rule

pytestmark = pytest.mark.gpu

CIN, COUT, N = 5, 6, 2
RULE_GEOMS = ["rect", "k2s2", "k5s3p2", "k1p1"]
PRESET = {"alpha": 1., "beta": 0., "ignore_bias": True}
GENERAL = {"alpha": 2., "beta": 1., "ignore_bias": False}


def general_rule_cpu(x, w, b, r, stride, padding, alpha, beta, dtype):
    """lrp_modules.Conv2d's docstring at any geometry, with bias: Z+ = conv(x+, W+) + conv(x-, W-) + b, Z- = conv(x-, W+) + conv(x+, W-) + b,
    S+- = R / safe(Z+-), R_in = alpha (x+ convT(S+, W+) + x- convT(S+, W-)) - beta (x- convT(S-, W+) + x+ convT(S-, W-))"""
    x, w, b, r = (t.to(dtype) for t in (x, w, b, r))
    xp, xn, wp, wn = x.clamp(min=0), x.clamp(max=0), w.clamp(min=0), w.clamp(max=0)
    conv = lambda a, k: F.conv2d(a, k, stride=stride, padding=padding)
    back = lambda s, k: torch.nn.grad.conv2d_input(x.shape, k, s, stride=stride, padding=padding)
    bb = b.view(1, -1, 1, 1)
    zp, zn = conv(xp, wp) + conv(xn, wn) + bb, conv(xn, wp) + conv(xp, wn) + bb
    sp, sn = r / (zp + 1e-7 * (zp == 0).to(dtype)), r / (zn + 1e-7 * (zn == 0).to(dtype))
    return alpha * (xp * back(sp, wp) + xn * back(sp, wn)) - beta * (xn * back(sn, wp) + xp * back(sn, wn))


def conditioned(geom, hw, general, base_seed):
    """(w, b, x, r, fp64, fp32) at the first seed whose fp32 CPU evaluation is within 1e-6 of fp64"""
    kh, kw, sh, sw, ph, pw = geom
    h, w_ = hw
    oh, ow = (h + 2 * ph - kh) // sh + 1, (w_ + 2 * pw - kw) // sw + 1
    for seed in range(base_seed, base_seed + 64):
        g = torch.Generator().manual_seed(seed)
        w = torch.randn(COUT, CIN, kh, kw, generator=g) * (2.0 / (CIN * kh * kw)) ** 0.5
        b = torch.randn(COUT, generator=g) * 0.03
        x = torch.randn(N, CIN, h, w_, generator=g)
        r = torch.randn(N, COUT, oh, ow, generator=g)
        if general:
            refs = [general_rule_cpu(x, w, b, r, (sh, sw), (ph, pw), GENERAL["alpha"], GENERAL["beta"], dt) for dt in (torch.float64, torch.float32)]
        else:
            refs = [conv_rule_cpu(x, w, r, (sh, sw), (ph, pw), dt) for dt in (torch.float64, torch.float32)]
        if rel_err(refs[1], refs[0]) < 1e-6:
            return w, b, x, r, refs[0], refs[1]
    raise AssertionError("no conditioned seed")


@pytest.mark.parametrize("general", [False, True], ids=["preset", "a2_b1_bias"])
@pytest.mark.parametrize("gid", RULE_GEOMS)
def test_conv_rule_on_a_real_module(gid, general):
    geom, hw = GEOMS[gid]
    w, b, x, r, ref64, ref32 = conditioned(geom, hw, general, 6100 + 64 * RULE_GEOMS.index(gid))
    got = run_conv_rule(w, b, x, r, geom[2:4], geom[4:], GENERAL if general else PRESET)
    assert got.shape == x.shape and torch.isfinite(got).all()
    assert_fp32_grade(got, ref64, ref32, f"Conv2d({CIN}, {COUT}) {gid} {'alpha 2 beta 1 with bias' if general else 'preset'}")


def test_a_3x3_conv_on_a_map_above_224_pixels_runs_on_the_engine():
    """3x3 / s1 / p1 is the VGG16 kernels' geometry; at max(H, W) > 224 the rule leaves them for lrpx_conv_geom: one forward and one
    transposed launch, counted by ops.LAUNCHES"""
    from lrp_amd import _lib, ops
    geom, hw = (3, 3, 1, 1, 1, 1), (226, 5)
    w, b, x, r, ref64, ref32 = conditioned(geom, hw, False, 6500)
    before = dict(ops.LAUNCHES)
    got = run_conv_rule(w, None, x, r, 1, 1, PRESET)
    delta = {k: v - before.get(k, 0) for k, v in ops.LAUNCHES.items() if v != before.get(k, 0)}
    assert delta == {("conv_geom", _lib.GEOM_FWD): 1, ("conv_geom", _lib.GEOM_BWD): 1}, delta
    assert_fp32_grade(got, ref64, ref32, f"Conv2d({CIN}, {COUT}, 3, padding=1) at 226 x 5")


def test_pool_rule_on_a_rectangular_maxpool():
    g = torch.Generator().manual_seed(6600)
    x = torch.randn(3, 6, 11, 13, generator=g)
    x[0, :, :5, :6] = 0.0
    x[1, 1, 3:7, 4:9] = 1.75
    pool = nn.MaxPool2d((2, 3), (2, 1), (0, 1))
    z, idx = F.max_pool2d(x.double(), (2, 3), (2, 1), (0, 1), return_indices=True)
    r = torch.randn(z.shape, generator=g)
    got = run_pool_rule(pool, x, r)
    s = r.double() / (z + 1e-7 * (z == 0).double())
    want = x.double() * torch.zeros(3, 6, 11 * 13, dtype=torch.float64).scatter_add_(2, idx.flatten(2), s.flatten(2)).view(3, 6, 11, 13)
    assert_pool_grade(got, want, "Pool2d on MaxPool2d((2, 3), (2, 1), (0, 1))")
