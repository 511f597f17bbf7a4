"""Host side of the off-geometry tests of the runtime-geometry contraction engine (tests/conv_geom_offgeom_cases.py; no GPU): the
geometry table against `conv_geom_check`'s output-size rule, the unreached-pixel masks against conv2d_input of an all-ones tensor, the
decision that every conv mode 1 case is fit for the criterion of tests/fp64_anchor.py on exactly the tensors the GPU test builds, and
the off-geometry net of tests/golden/make_golden_resnet_offgeom.py: what the engine's matcher finds in it, the stored seeds against their
recipes, and the dual-coefficient formulation of tests/resnet_ab_cases.py in fp64 against the reference's fp64 maps."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from lrp_amd import _lib, ops
from lrp_amd.LRPtools import lrp_modules

from conftest import GOLDEN, rel_err
from conv_geom_offgeom_cases import (AB_CHANNELS, AB_ENTRIES, CHANNELS, ENTRIES, GEOMS, REDRAW, UNREACHED, ab_case, case, fit, maps_of,
                                     out_hw, unreached)
from resnet_ab_cases import ab_relevance, ab_trace

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet_offgeom import (AB_PAIR, GRAD_MARGIN, GRAD_SEED, OFFGEOM, conditioning_rect, grad_inputs, margins_rect,  # noqa: E402
                                        offgeom_grad_net, offgeom_net)


# ---- the geometry table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", list(GEOMS))
def test_the_table_satisfies_the_output_size_rule(gid):
    """the table's output map is the one torch's own conv produces and the rule's other clauses hold; the entry refuses its two
    neighbours by name (made-up, aligned pointers: a refused descriptor is never dereferenced)"""
    assert os.path.exists(_lib.LIB_PATH), "liblrpx.so not built (run __graft_entry__.build())"
    lib = _lib.load()
    geom, (h, w) = GEOMS[gid]
    kh, kw, sh, sw, ph, pw = geom
    oh, ow = out_hw(gid)
    assert h + 2 * ph >= kh and w + 2 * pw >= kw and oh > 0 and ow > 0 and kh * kw <= 1024 and sh * sw < 65536
    assert tuple(torch.nn.functional.conv2d(torch.zeros(1, 1, h, w), torch.zeros(1, 1, kh, kw), stride=(sh, sw), padding=(ph, pw)).shape[2:]) \
        == (oh, ow)
    n_img, m2i = maps_of(gid)
    assert len(m2i) > n_img and sorted(set(m2i)) == list(range(n_img)) and m2i != sorted(m2i)      # repeated and unsorted
    for d_oh, d_ow in ((1, 0), (0, -1)):
        bad = _lib.ConvGeomExDesc(in_=0x10000, wpacked=0x20000, bias=None, x=0x30000, q=None, addend=None, map2img=None, out=0x50000,
                                  dir=_lib.GEOM_BWD, n=1, n_img=1, h=h, w=w, oh=oh + d_oh, ow=ow + d_ow, kh=kh, kw=kw, sh=sh, sw=sw, ph=ph,
                                  pw=pw, k=4, n_oc=3)
        assert lib.lrpx_conv_geom_ex(C.byref(bad), None) == _lib.EINVAL
        msg = lib.lrpx_last_error_string()
        assert (b"output %dx%d is not what input %dx%d gives" % (oh + d_oh, ow + d_ow, h, w) in msg) or (ow + d_ow == 0 and b"bad sizes" in msg), msg


def test_the_table_reaches_what_it_claims():
    """the edges the table is there for, from the index arithmetic of the transposed direction (csrc/conv_geom_kernel.h): taps per class
    and axis, empty classes, the idle wave"""
    def taps(gid):       # {(class row, class column): (taps along h, taps along w)} of the classes that hold pixels
        (kh, kw, sh, sw, ph, pw), (h, w) = GEOMS[gid]
        per = lambda c, p, s, k: len(range((c + p) % s, k, s))
        return {(ch, cw): (per(ch, ph, sh, kh), per(cw, pw, sw, kw)) for ch in range(min(sh, h)) for cw in range(min(sw, w))}
    assert set(taps("k4s4").values()) == {(1, 1)} and len(taps("k4s4")) == 16
    assert {t for pair in taps("k5s3p2").values() for t in pair} == {1, 2}
    assert {t for pair in taps("rect").values() for t in pair} == {1, 2}
    assert len(taps("gap")) == 2 * 2 and GEOMS["gap"][0][2] == 3           # class row 2 of 3 holds no pixel: H = 2 < sh
    assert 0 in {t for pair in taps("gap").values() for t in pair}        # and a class with pixels that no tap reaches
    assert max(a * b for a, b in taps("k11s4").values()) == 9 and GEOMS["k11s4"][0][0] * GEOMS["k11s4"][0][1] == 121
    assert all(o > i for o, i in zip(out_hw("k1p1"), GEOMS["k1p1"][1]))
    (h, w), (n_img, m2i) = GEOMS["rect_5x3"][1], maps_of("rect_5x3")
    assert len(m2i) * -(-h // 2) * -(-w // 3) <= 64 and len(m2i) >= 4     # one 64-pixel tile of the largest class spans every map
    assert any(-(-n_oc // 32) % 2 == 1 and n_oc > 64 for _, n_oc in CHANNELS)      # 72: the fourth 32-column block is an idle wave


@pytest.mark.parametrize("gid", list(GEOMS))
def test_unreached_masks_are_what_conv2d_input_of_ones_gives(gid):
    (kh, kw, sh, sw, ph, pw), (h, w) = GEOMS[gid]
    oh, ow = out_hw(gid)
    cover = torch.nn.grad.conv2d_input((1, 1, h, w), torch.ones(1, 1, kh, kw, dtype=torch.float64), torch.ones(1, 1, oh, ow, dtype=torch.float64),
                                       stride=(sh, sw), padding=(ph, pw))[0, 0]
    assert torch.equal(unreached(gid), cover == 0)
    assert bool(unreached(gid).any()) == (gid in UNREACHED)
    if gid == "k2s2":
        assert unreached(gid)[-1].all() and unreached(gid)[:, -1].all() and int(unreached(gid).sum()) == h + w - 1
    if gid == "k4s4":
        assert unreached(gid)[-3:].all() and not unreached(gid)[:-3, :-1].any()


# ---- the conv mode 1 cases are fit for the bound -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", list(GEOMS))
def test_the_b6_cases_are_fit_for_the_fp32_grade_bound(gid):
    """on the GPU test's own tensors: the six plane products of conv mode 1, summed in fp64, pass e <= C max(e32, FLOOR) at every entry
    that has a _b6 form - a conv mode 1 failure on the GPU is then the kernel's"""
    worst = {}
    for k, n_oc in CHANNELS:
        for entry in (e for e, b6 in ENTRIES.items() if b6):
            worst[entry] = max(worst.get(entry, 0.), fit(entry, case(gid, k, n_oc)))
    for kr, n_oc in AB_CHANNELS:
        for entry in AB_ENTRIES:
            worst[entry] = max(worst.get(entry, 0.), fit(entry, ab_case(gid, kr, n_oc)))
    print(f"off-geometry b6 inputs {gid}: six-product emulation error / bound, worst per entry: " +
          "  ".join(f"{e} {v:.3f}" for e, v in worst.items()))
    assert all(v <= 1 for v in worst.values()), (gid, worst)


def test_the_redraw_table_names_cases():
    names = {"%s_%d_%d" % (gid, kr, n_oc) for gid in GEOMS for kr, n_oc in AB_CHANNELS}
    assert set(REDRAW) <= names


# ---- the off-geometry net ------------------------------------------------------------------------------------------------------------------
def test_the_matcher_finds_the_off_geometry_net():
    net = offgeom_net(np.random.RandomState(3), lrp_modules.resAdd)
    plan = ops.match_bottleneck_resnet(net)
    flat = lambda t: tuple(t[0]) + tuple(t[1]) + tuple(t[2])
    assert plan.pool == flat(OFFGEOM["pool"])
    assert plan.convs[0]["geom"] == flat(OFFGEOM["stem"])
    strided = plan.blocks[1]
    assert plan.convs[strided["conv2"]]["geom"] == flat(OFFGEOM["conv2"])
    assert plan.convs[strided["downsample"]]["geom"] == flat(OFFGEOM["shortcut"])
    resnet50 = {(1, 1, 1, 1, 0, 0), (1, 1, 2, 2, 0, 0), (3, 3, 1, 1, 1, 1), (3, 3, 2, 2, 1, 1), (7, 7, 2, 2, 3, 3)}
    assert len({cv["geom"] for cv in plan.convs} - resnet50) == 3
    with torch.no_grad():
        assert tuple(net(torch.zeros(OFFGEOM["shape"])).shape) == (OFFGEOM["shape"][0],) + OFFGEOM["feat"]


def test_the_stored_seeds_meet_their_recipes():
    G = dict(np.load(os.path.join(GOLDEN, "resnet_offgeom.npz")))
    assert list(G["map2img"]) == OFFGEOM["map2img"] and tuple(G["ab_pair"]) == AB_PAIR
    add_min, pool_min = conditioning_rect(offgeom_net(np.random.RandomState(int(G["seed"])), lrp_modules.resAdd).double(),
                                          torch.from_numpy(G["x"]).double())
    e32 = max(rel_err(a, b) for a, b in zip(G["r32"], G["r64"]))
    print(f"resnet_offgeom.npz seed {int(G['seed'])}: Add ratio {add_min:.3f}  pool lead {pool_min:.2e}  e32 {e32:.2e}  "
          f"alpha {AB_PAIR[0]:g} beta {AB_PAIR[1]:g} e32 {float(G['ab_e32']):.2e}")
    assert add_min >= 0.1 and pool_min >= 1e-3 and e32 < 1e-5 and float(G["ab_e32"]) < 1e-5
    x, _ = grad_inputs(GRAD_SEED)
    relu_m, pool_m = margins_rect(offgeom_grad_net(GRAD_SEED, lrp_modules.resAdd).double(), torch.from_numpy(x).double())
    print(f"off-geometry gradient net seed {GRAD_SEED}: relu margin {relu_m:.2e}  pool margin {pool_m:.2e}")
    assert relu_m >= GRAD_MARGIN and pool_m >= GRAD_MARGIN


@pytest.mark.parametrize("alpha,beta,key", [(1., 0., "r64"), AB_PAIR + ("ab_r64",)], ids=["a1_b0", "a2_b1"])
def test_dual_coefficient_formulation_reproduces_the_reference_in_fp64(alpha, beta, key):
    G = dict(np.load(os.path.join(GOLDEN, "resnet_offgeom.npz")))
    net = offgeom_net(np.random.RandomState(int(G["seed"])), lrp_modules.resAdd).double()
    plan = ops.match_bottleneck_resnet(net)
    with torch.no_grad():
        tr = ab_trace(plan, torch.from_numpy(G["x"]).double())
        for m, img in enumerate(G["map2img"]):
            got = ab_relevance(plan, tr, torch.from_numpy(G["targets"][m:m + 1]).double(), int(img), alpha, beta)[0]
            e = rel_err(got, G[key][m])
            print(f"dual-coefficient formulation, off-geometry net, alpha {alpha:g} beta {beta:g} map {m} (image {img}): {e:.2e} of the map's maximum")
            assert e < 1e-9, (alpha, beta, m, e)
