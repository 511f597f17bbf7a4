"""The batched bottleneck-ResNet encoder engine (ops.ResNetEncoder) end to end on the GPU on a net that none of ResNet-50's geometries
describes (tests/golden/make_golden_resnet_offgeom.py: stem conv (5, 4) / (3, 2) / (1, 2), MaxPool2d((2, 3), (2, 1), (0, 1)), a strided
block with a (3, 5) / (2, 3) / (1, 2) conv2 and a (1, 3) / (2, 3) / (0, 1) shortcut; 2 x 3 x 47 x 52 -> 4 x 9 x 64, three maps on the
images [1, 0, 1]), all five passes in both conv modes.

Relevance and relevance_alpha_beta(2, 1): against the reference's own fp64 maps (tests/golden/resnet_offgeom.npz), < 1e-4 of each map's
maximum (the bound of every engine test); the byte equalities of the batched contract; agreement with the generic
add_lrp / compute_lrp driver on the same net.  Gradient, guided "stem", guided "all": against make_golden_resnet_grad.chain in fp64 at
test time, under the same bound, after the fixture's condition (no ReLU mask of the engine's trace differs from the fp64 forward's)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lrp_amd  # noqa: F401
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet_grad import PASSES, chain  # noqa: E402
from make_golden_resnet_offgeom import AB_PAIR, GRAD_SEED, OFFGEOM, grad_inputs, offgeom_grad_net, offgeom_net  # noqa: E402

MODES = pytest.mark.parametrize("mode", [0, 1])
_CACHE = {}


def _mods():
    from lrp_amd import _lib, ops
    from lrp_amd.LRPtools import lrp_modules, lrp_wrapper
    return _lib, ops, lrp_modules, lrp_wrapper


def _i32(v):
    return torch.tensor([int(a) for a in v], dtype=torch.int32, device="cuda")


def _rows(t_nchw):
    n, c, h, w = t_nchw.shape
    return t_nchw.permute(0, 2, 3, 1).reshape(n, h * w, c).float().contiguous().cuda()


def golden():
    if "G" not in _CACHE:
        _CACHE["G"] = dict(np.load(os.path.join(GOLDEN, "resnet_offgeom.npz")))
    return _CACHE["G"]


def fixture():
    """(golden arrays, net, inputs on the device, {mode: traced engine}, {mode: (relevance, alpha-beta relevance)}), built once and
    shared read-only; the tests never call forward() on these engines"""
    if "fx" not in _CACHE:
        _, ops, lrp_modules, _ = _mods()
        G = golden()
        net = offgeom_net(np.random.RandomState(int(G["seed"])), lrp_modules.resAdd).cuda()
        x, targets = torch.from_numpy(G["x"]).cuda(), torch.from_numpy(G["targets"]).cuda()
        t, m2i = ops.nchw_to_nhwc(targets), _i32(G["map2img"])
        engines, maps = {}, {}
        for mode in (0, 1):
            eng = ops.ResNetEncoder(net, conv_mode=mode)
            feats = eng.forward(x)
            assert tuple(feats.shape) == (2, OFFGEOM["feat"][1] * OFFGEOM["feat"][2], OFFGEOM["feat"][0])
            engines[mode] = eng
            maps[mode] = (eng.relevance(t, m2i).clone(), eng.relevance_alpha_beta(t, m2i, *AB_PAIR).clone())
        torch.cuda.synchronize()
        _CACHE["fx"] = (G, net, dict(x=x, targets=targets, t=t, m2i=m2i), engines, maps)
    return _CACHE["fx"]


# ---- 1. relevance against the reference ------------------------------------------------------------------------------------------------------
@MODES
def test_relevance_against_the_reference(mode):
    G, _, _, _, maps = fixture()
    r = maps[mode][0].cpu()
    assert tuple(r.shape) == G["r64"].shape
    for row, img in enumerate(G["map2img"]):
        e, e32 = rel_err(r[row], G["r64"][row]), rel_err(G["r32"][row], G["r64"][row])
        print(f"off-geometry engine relevance mode {mode} row {row} (image {img}): e {e:.2e}  reference's e32 {e32:.2e}  bound 1.0e-04")
        assert e < 1e-4, (row, e)


@MODES
def test_alpha_beta_against_the_reference(mode):
    G, _, _, _, maps = fixture()
    r = maps[mode][1].cpu()
    assert tuple(r.shape) == G["ab_r64"].shape
    for row, img in enumerate(G["map2img"]):
        e = rel_err(r[row], G["ab_r64"][row])
        print(f"off-geometry engine alpha {AB_PAIR[0]:g} beta {AB_PAIR[1]:g} mode {mode} row {row} (image {img}): e {e:.2e}  "
              f"reference's e32 {float(G['ab_e32_rows'][row]):.2e}  bound 1.0e-04")
        assert e < 1e-4, (row, e)
    assert rel_err(r, maps[mode][0].cpu()) > 1e-2           # another rule, not the preset again


@MODES
@pytest.mark.parametrize("rule", ["preset", "alpha_beta"])
def test_a_map_does_not_depend_on_the_other_maps_of_the_call(rule, mode):
    G, _, d, engines, maps = fixture()
    eng, t, m2i = engines[mode], d["t"], [int(i) for i in G["map2img"]]
    call = (lambda tt, mm: eng.relevance(tt, mm)) if rule == "preset" else (lambda tt, mm: eng.relevance_alpha_beta(tt, mm, *AB_PAIR))
    r = maps[mode][0 if rule == "preset" else 1]
    perm = [1, 0, 2]
    rp = call(t[perm].contiguous(), _i32([m2i[p] for p in perm])).clone()
    for new, old in enumerate(perm):
        assert torch.equal(rp[new], r[old]), f"row {old} changed when the call's rows were permuted"
    for row in range(3):
        alone = call(t[row:row + 1].contiguous(), _i32([m2i[row]]))
        assert torch.equal(alone[0], r[row]), f"row {row} alone differs from row {row} in the call of three"
    ident = call(t[:2].contiguous(), None).clone()
    assert torch.equal(ident, call(t[:2].contiguous(), _i32([0, 1])))


@MODES
def test_the_engine_agrees_with_the_generic_driver(mode):
    _, _, _, lrp_wrapper = _mods()
    G, net, d, _, maps = fixture()
    m2i = [int(i) for i in G["map2img"]]
    try:
        for what, params, want in (("preset", None, maps[mode][0]), ("alpha-beta", {"alpha": AB_PAIR[0], "beta": AB_PAIR[1]}, maps[mode][1])):
            lrp_wrapper.add_lrp(net) if params is None else lrp_wrapper.add_lrp(net, lrp_params=params)
            for row, img in enumerate(m2i):
                generic = net.compute_lrp(d["x"][img:img + 1].clone(), target=d["targets"][row:row + 1])[0]     # a fresh sample tensor
                eg = rel_err(want[row].cpu(), generic.cpu())
                print(f"off-geometry engine {what} mode {mode} row {row} against the generic driver: {eg:.2e} of the map's maximum  bound 1.0e-04")
                assert eg < 1e-4, (what, row, eg)
            batched = net.compute_lrp_maps if params is None else net.compute_lrp_maps_ab
            assert torch.equal(batched(d["x"], d["targets"], d["m2i"], conv_mode=mode), want), what + ": the hook API differs from the engine"
    finally:
        lrp_wrapper.add_lrp(net)


# ---- 2. the gradient passes against fp64 at test time ----------------------------------------------------------------------------------------
def grad_reference():
    """{pass: (n_maps, 3, H, W) fp64} by make_golden_resnet_grad.chain on the CPU, one sample tensor per map; computed once"""
    if "g64" not in _CACHE:
        _, _, lrp_modules, _ = _mods()
        x, d_feat = grad_inputs(GRAD_SEED)
        net = offgeom_grad_net(GRAD_SEED, lrp_modules.resAdd).double()
        x64, d64 = torch.from_numpy(x).double(), torch.from_numpy(d_feat).double()
        relus = {"plain": None, "stem": "stem", "all": "all"}
        _CACHE["g64"] = {k: torch.stack([chain(net, x64[img:img + 1], d64[m:m + 1], relus[k])[0] for m, img in enumerate(OFFGEOM["map2img"])])
                         for k in PASSES}
    return _CACHE["g64"]


def grad_fixture(mode):
    """(engine with the trace of x, feature-map gradients NHWC, map2img, {pass: maps}), computed once per mode and shared read-only"""
    key = ("gfx", mode)
    if key not in _CACHE:
        _, ops, lrp_modules, _ = _mods()
        x, d_feat = grad_inputs(GRAD_SEED)
        net = offgeom_grad_net(GRAD_SEED, lrp_modules.resAdd).cuda()
        eng = ops.ResNetEncoder(net, conv_mode=mode)
        eng.forward(torch.from_numpy(x).cuda())
        d, m2i = _rows(torch.from_numpy(d_feat)), _i32(OFFGEOM["map2img"])
        maps = {"plain": eng.gradient(d, m2i).clone(), "stem": eng.guided_backprop(d, m2i).clone(),
                "all": eng.guided_backprop(d, m2i, relus="all").clone()}
        torch.cuda.synchronize()
        _CACHE[key] = (eng, d, m2i, maps)
    return _CACHE[key]


@MODES
def test_the_fixture_condition_holds_on_the_engines_trace(mode):
    """every ReLU mask of the engine's trace against the fp64 forward on the CPU.  A flip is a discontinuity of the gradient: the
    comparisons below would then say nothing about the kernels."""
    _, _, lrp_modules, _ = _mods()
    eng = grad_fixture(mode)[0]
    net = offgeom_grad_net(GRAD_SEED, lrp_modules.resAdd).double()
    masks = {}
    with torch.no_grad():
        a = F.relu(net.bn1(net.conv1(torch.from_numpy(grad_inputs(GRAD_SEED)[0]).double())))
        masks["act", 0] = a > 0
        a = net.maxpool(a)
        for bi, (blk, pb) in enumerate(zip(net.layers, eng.plan.blocks)):
            o = F.relu(blk.bn1(blk.conv1(a)))
            masks["act", pb["conv1"]] = o > 0
            o = F.relu(blk.bn2(blk.conv2(o)))
            masks["act", pb["conv2"]] = o > 0
            a = F.relu(blk.bn3(blk.conv3(o)) + blk.downsample(a))
            masks["out", bi] = a > 0
    flips = 0
    for (kind, i), want in masks.items():
        got = eng.trace[kind][i] > 0
        flips += int((got.cpu() != want.permute(0, 2, 3, 1).reshape(got.shape)).sum())
    assert flips == 0, (f"the fixture's condition is broken: {flips} ReLU mask(s) of the engine's trace differ from the fp64 forward; "
                        f"nothing is known about the kernels from this fixture")


@pytest.mark.parametrize("which", PASSES)
@MODES
def test_gradient_passes_against_fp64(mode, which):
    got = grad_fixture(mode)[3][which].cpu()
    want = grad_reference()[which]
    assert tuple(got.shape) == tuple(want.shape)
    other = grad_fixture(1 - mode)[3][which].cpu()
    for row, img in enumerate(OFFGEOM["map2img"]):
        e = rel_err(got[row], want[row])
        print(f"off-geometry engine {which} mode {mode} row {row} (image {img}): e {e:.2e}  mode {mode} against mode {1 - mode} "
              f"{rel_err(got[row], other[row]):.2e}  bound 1.0e-04")
        assert e < 1e-4, (which, row, e)


@MODES
def test_gradient_maps_do_not_depend_on_the_other_maps_of_the_call(mode):
    eng, d, _, maps = grad_fixture(mode)
    calls = {"plain": lambda *a: eng.gradient(*a), "stem": lambda *a: eng.guided_backprop(*a),
             "all": lambda *a: eng.guided_backprop(*a, relus="all")}
    for which, call in calls.items():
        for row, img in enumerate(OFFGEOM["map2img"]):
            assert torch.equal(call(d[row:row + 1].contiguous(), _i32([img]))[0], maps[which][row]), (which, row, "alone")
