"""The gradient chain of the batched ResNet encoder engine on the GPU (ops.ResNetEncoder.gradient / guided_backprop).

Contraction level: lrpx_conv_geom_grad / _grad_b6 against the formula in fp64 on the CPU at the five geometries of
make_golden_conv_geom_bytes.GEOMS, every combination of mask / scale / addend / clamp; criterion of tests/fp64_anchor.py:
rel_err(got, fp64) <= C * max(rel_err(fp32 CPU, fp64), FLOOR), C = 6, FLOOR = 1e-7.  Byte anchor: with an all-positive mask, no scale
and no clamp the result is lrpx_conv_geom_ex's (_ex_b6's) with q = 1 and x = 1.  The two elementwise kernels are exact against torch.

Engine level, both conv modes, both nets of tests/golden/resnet_grad.npz: the fixture's condition first (no ReLU mask of the engine's
trace differs from the fp64 forward's), then plain / guided "stem" / guided "all" < 1e-4 of each map's maximum against fp64 (SURVEY
8(d), the bound of every ResNet engine test), then the byte equalities of the batched contract."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lrp_amd  # noqa: F401
from conftest import GOLDEN, rel_err
from fp64_anchor import C, FLOOR

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_conv_geom_bytes import GEOMS  # noqa: E402
from make_golden_resnet_grad import NETS, PASSES, grad_net  # noqa: E402

HW, N_IMG, MAP2IMG = (11, 13), 2, [1, 0, 1]
_CACHE = {}


def _mods():
    from lrp_amd import _lib, ops
    from lrp_amd.LRPtools import lrp_modules
    return _lib, ops, lrp_modules


def _i32(v):
    return torch.tensor([int(a) for a in v], dtype=torch.int32, device="cuda")


def _rows(t_nchw):
    """(n, c, h, w) on the CPU -> (n, h w, c) on the device"""
    n, c, h, w = t_nchw.shape
    return t_nchw.permute(0, 2, 3, 1).reshape(n, h * w, c).float().contiguous().cuda()


def _nchw(rows, h, w):
    return rows.cpu().view(rows.shape[0], h, w, -1).permute(0, 3, 1, 2)


# ---- 1. the contraction against its formula ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b6", [False, True], ids=["fp32", "b6"])
@pytest.mark.parametrize("gname", list(GEOMS))
def test_conv_geom_grad_against_the_formula(gname, b6):
    _lib, ops, _ = _mods()
    ksz, s, p = GEOMS[gname]
    (h, w), geom = HW, (ksz, ksz, s, s, p, p)
    oh, ow = (h + 2 * p - ksz) // s + 1, (w + 2 * p - ksz) // s + 1
    m2i, n = _i32(MAP2IMG), len(MAP2IMG)
    gen = torch.Generator().manual_seed(500 + 7 * ksz + s)
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    for k in (12, 36):
        for n_oc in (3, 40):
            wt, g, mask, scale, addend = rn(k, n_oc, ksz, ksz), rn(n, k, oh, ow), rn(N_IMG, k, oh, ow), rn(k), rn(n, n_oc, h, w)
            pack = (ops.conv_geom_pack_bf16x3 if b6 else ops.conv_geom_pack)(wt.cuda(), _lib.GEOM_BWD)
            d = dict(g=_rows(g), mask=_rows(mask), scale=scale.cuda(), addend=_rows(addend))
            worst = 0.
            for case in range(16):
                use_mask, use_scale, use_add, clamp = case & 1, case & 2, case & 4, case & 8
                got = ops.conv_geom_grad(d["g"], pack, n, (h, w), (oh, ow), geom, k, n_oc, mask=d["mask"] if use_mask else None,
                                         scale=d["scale"] if use_scale else None, clamp=bool(clamp), addend=d["addend"] if use_add else None,
                                         map2img=m2i, n_img=N_IMG, b6=b6)
                refs = []
                for dtype in (torch.float64, torch.float32):
                    a = g.to(dtype)
                    if clamp:
                        a = a.clamp(min=0)
                    if use_mask:
                        a = a * (mask[MAP2IMG] > 0).to(dtype)
                    if use_scale:
                        a = a * scale.to(dtype)[None, :, None, None]
                    ref = torch.nn.grad.conv2d_input((n, n_oc, h, w), wt.to(dtype), a, stride=s, padding=p)
                    refs.append(ref + addend.to(dtype) if use_add else ref)
                e, e32 = rel_err(_nchw(got, h, w), refs[0]), rel_err(refs[1], refs[0])
                worst = max(worst, e / max(e32, FLOOR))
                assert e <= C * max(e32, FLOOR), (f"{gname} k {k} n_oc {n_oc} mask {bool(use_mask)} scale {bool(use_scale)} addend {bool(use_add)} "
                                                  f"clamp {bool(clamp)}: rel_err vs fp64 {e:.3e} > {C} x max(fp32's {e32:.3e}, {FLOOR:.0e})")
                if s == 2 and ksz == 1 and not use_add:            # rows / columns of odd index: no tap reaches their class
                    o = _nchw(got, h, w)
                    assert not o[:, :, 1::2, :].any() and not o[:, :, :, 1::2].any()
            print(f"conv_geom_grad{'_b6' if b6 else ''} {gname} {k}->{n_oc} at {h}x{w}, 16 operand combinations: worst e / max(e32, FLOOR) "
                  f"{worst:.2f}  bound {C:.0f}")
            # byte anchor
            ones_q = torch.ones(N_IMG, oh * ow, k, device="cuda")
            ones_x = torch.ones(N_IMG, h * w, n_oc, device="cuda")
            for add in (None, d["addend"]):
                want = ops.conv_geom_ex(d["g"], pack, _lib.GEOM_BWD, n, (h, w), (oh, ow), geom, k, n_oc, x=ones_x, q=ones_q, addend=add,
                                        map2img=m2i, n_img=N_IMG, b6=b6)
                got = ops.conv_geom_grad(d["g"], pack, n, (h, w), (oh, ow), geom, k, n_oc, mask=ones_q, addend=add, map2img=m2i, n_img=N_IMG,
                                         b6=b6)
                assert torch.equal(got, want), f"{gname} {k}->{n_oc}: not the bytes of conv_geom_ex with q = 1, x = 1"


def test_launches_are_counted():
    _lib, ops, _ = _mods()
    before = dict(ops.LAUNCHES)
    pack = ops.conv_geom_pack(torch.randn(12, 3, 1, 1).cuda(), _lib.GEOM_BWD)
    pack6 = ops.conv_geom_pack_bf16x3(torch.randn(12, 3, 1, 1).cuda(), _lib.GEOM_BWD)
    g = torch.randn(2, 20, 12).cuda()
    ops.conv_geom_grad(g, pack, 2, (4, 5), (4, 5), (1, 1, 1, 1, 0, 0), 12, 3)
    ops.conv_geom_grad_b6(g, pack6, 2, (4, 5), (4, 5), (1, 1, 1, 1, 0, 0), 12, 3)
    ops.resnet_relu_grad(g, g, None, torch.empty_like(g), 2, 2, False)
    for key in (("conv_geom_grad", _lib.GEOM_BWD), ("conv_geom_grad_b6", _lib.GEOM_BWD), ("resnet_relu_grad", None)):
        assert ops.LAUNCHES.get(key, 0) == before.get(key, 0) + 1, key


# ---- 2. the elementwise kernels, exactly -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [False, True])
def test_relu_grad_is_exact(clamp):
    _, ops, _ = _mods()
    gen = torch.Generator().manual_seed(77)
    g, act = torch.randn(3, 143, 20, generator=gen), torch.randn(2, 143, 20, generator=gen).clamp(min=0)
    act[0, :5] = -0.0
    out = torch.full_like(g, float("nan")).cuda()
    ops.resnet_relu_grad(g.cuda(), act.cuda(), _i32(MAP2IMG), out, 3, 2, clamp)
    want = torch.where(act[MAP2IMG] > 0, g.clamp(min=0) if clamp else g, torch.zeros(()))
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("win", [(3, 3, 2, 2, 1, 1), (2, 2, 2, 2, 0, 0), (3, 3, 1, 1, 1, 1)], ids=["k3s2p1", "k2s2", "k3s1p1"])
def test_maxpool_grad_is_exact(win):
    """x >= 0 with a plateau of ties, an all-zero region (every window of it ties at zero: the first element wins) and, per
    channel, distinct values elsewhere; g_out in eighths, so the sum of the windows an element wins is exact in any order"""
    _, ops, _ = _mods()
    kh, kw, sh, sw, ph, pw = win
    h, w, c = 11, 13, 6
    oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    gen = torch.Generator().manual_seed(78)
    x = torch.rand(2, c, h, w, generator=gen) + 0.25
    x[0, :, :5, :6] = 0.0
    x[1, 1, 3:7, 4:9] = 1.75
    g_out = torch.randint(-40, 41, (3, c, oh, ow), generator=gen).float() / 8
    got = torch.full((3, h * w, c), float("nan")).cuda()
    ops.resnet_maxpool_grad(_rows(x), _rows(g_out), _i32(MAP2IMG), got, 3, 2, (h, w), (oh, ow), c, win)
    _, idx = F.max_pool2d(x[MAP2IMG], (kh, kw), (sh, sw), (ph, pw), return_indices=True)
    want = torch.zeros(3, c, h * w).scatter_add_(2, idx.flatten(2), g_out.flatten(2)).view(3, c, h, w)
    assert torch.equal(_nchw(got, h, w), want)


# ---- 3. the engine on resnet_grad.npz ----------------------------------------------------------------------------------------------------
def golden():
    if "G" not in _CACHE:
        _CACHE["G"] = dict(np.load(os.path.join(GOLDEN, "resnet_grad.npz")))
    return _CACHE["G"]


def fixture(name, mode):
    """(arrays of the net, engine with the trace of x, feature-map gradients NHWC, map2img, {pass: maps}) computed once and shared
    read-only"""
    key = ("fx", name, mode)
    if key not in _CACHE:
        _, ops, lrp_modules = _mods()
        G = {k[len(name) + 1:]: v for k, v in golden().items() if k.startswith(name + "_")}
        net = grad_net(G["seed"], lrp_modules.resAdd, NETS[name]).cuda()
        eng = ops.ResNetEncoder(net, conv_mode=mode)
        eng.forward(torch.from_numpy(G["x"]).cuda())
        d, m2i = _rows(torch.from_numpy(G["d_feat"])), _i32(G["map2img"])
        maps = {"plain": eng.gradient(d, m2i).clone(), "stem": eng.guided_backprop(d, m2i).clone(),
                "all": eng.guided_backprop(d, m2i, relus="all").clone()}
        torch.cuda.synchronize()
        _CACHE[key] = (G, eng, d, m2i, maps)
    return _CACHE[key]


CASES = [(name, mode) for name in NETS for mode in (0, 1)]
IDS = ["%s-mode%d" % c for c in CASES]


@pytest.mark.parametrize("name,mode", CASES, ids=IDS)
def test_the_fixture_condition_holds_on_the_engines_trace(name, mode):
    """every ReLU mask of the engine's trace against the fp64 forward on the CPU.  A flip is a discontinuity of the gradient: the
    comparisons below would then say nothing about the kernels."""
    _, ops, lrp_modules = _mods()
    G, eng, _, _, _ = fixture(name, mode)
    net = grad_net(G["seed"], lrp_modules.resAdd, NETS[name]).double()
    masks = {}
    with torch.no_grad():
        a = F.relu(net.bn1(net.conv1(torch.from_numpy(G["x"]).double())))
        masks["act", 0] = a > 0
        a = net.maxpool(a)
        for bi, (blk, pb) in enumerate(zip(net.layers, eng.plan.blocks)):
            o = F.relu(blk.bn1(blk.conv1(a)))
            masks["act", pb["conv1"]] = o > 0
            o = F.relu(blk.bn2(blk.conv2(o)))
            masks["act", pb["conv2"]] = o > 0
            a = F.relu(blk.bn3(blk.conv3(o)) + (a if blk.downsample is None else blk.downsample(a)))
            masks["out", bi] = a > 0
    flips = 0
    for (kind, i), want in masks.items():
        got = eng.trace[kind][i] > 0
        flips += int((got.cpu() != want.permute(0, 2, 3, 1).reshape(got.shape)).sum())
    assert flips == 0, (f"the fixture's condition is broken: {flips} ReLU mask(s) of the engine's trace differ from the fp64 forward "
                        f"(stored margin {float(G['relu_margin']):.1e}); nothing is known about the kernels from this fixture")


@pytest.mark.parametrize("which", PASSES)
@pytest.mark.parametrize("name,mode", CASES, ids=IDS)
def test_engine_against_fp64(name, mode, which):
    G, _, _, _, maps = fixture(name, mode)
    got = maps[which].cpu()
    assert tuple(got.shape) == tuple(G[which + "64"].shape)
    other = fixture(name, 1 - mode)[4][which].cpu()
    for row in range(got.shape[0]):
        e, e32 = rel_err(got[row], G[which + "64"][row]), float(G["e32_rows"][PASSES.index(which), row])
        print(f"resnet {which} {name} mode {mode} row {row} (image {G['map2img'][row]}): e {e:.2e}  reference's e32 {e32:.2e}  "
              f"mode {mode} against mode {1 - mode} {rel_err(got[row], other[row]):.2e}  bound 1.0e-04")
        assert e < 1e-4, (which, row, e)


@pytest.mark.parametrize("name,mode", CASES, ids=IDS)
def test_byte_equalities_of_the_batched_contract(name, mode):
    G, eng, d, m2i, maps = fixture(name, mode)
    x = torch.from_numpy(G["x"]).cuda()
    calls = {"plain": lambda e, *a, **k: e.gradient(*a, **k), "stem": lambda e, *a, **k: e.guided_backprop(*a, **k),
             "all": lambda e, *a, **k: e.guided_backprop(*a, relus="all", **k)}
    rel_before = eng.relevance(d.abs(), m2i).clone()
    rep = eng.replica()
    rep.forward(x)
    for which, call in calls.items():
        want = maps[which]
        for row, img in enumerate(G["map2img"]):                 # one map at a time, on the repeated / unsorted map2img
            assert torch.equal(call(eng, d[row:row + 1].contiguous(), _i32([img]))[0], want[row]), (which, row, "alone")
        out = torch.full_like(want, float("nan"))
        assert call(eng, d, m2i, out=out) is out and torch.equal(out, want), (which, "out=")
        assert torch.equal(call(rep, d, m2i), want), (which, "replica")
    assert rep._grad_packs is eng._grad_packs
    assert torch.equal(eng.relevance(d.abs(), m2i), rel_before), "a gradient call changed the trace: relevance differs after it"
    solo = eng.replica()                                         # an image alone against the same image inside the batch
    for img in sorted(set(int(i) for i in G["map2img"])):
        solo.forward(x[img:img + 1].contiguous())
        rows = [r for r, i in enumerate(G["map2img"]) if int(i) == img]
        for which, call in calls.items():
            got = call(solo, d[rows].contiguous(), _i32([0] * len(rows)))
            assert torch.equal(got, maps[which][rows]), (which, img, "image alone")


def test_argument_checks_on_a_live_engine():
    _lib, ops, _ = _mods()
    G, eng, d, m2i, _ = fixture("tiny", 0)
    with pytest.raises(ValueError, match="relus must be"):
        eng.guided_backprop(d, m2i, relus="block")
    for fn in (eng.gradient, eng.guided_backprop):
        with pytest.raises(ValueError, match="must be float32"):
            fn(d[:, :-1].contiguous(), m2i)
        with pytest.raises(ValueError, match="must be float32"):
            fn(d.double(), m2i)
        with pytest.raises(ValueError, match="out must be contiguous"):
            fn(d, m2i, out=torch.empty(1, 3, 38, 34, device="cuda"))
        with pytest.raises(_lib.LrpxError, match="outside"):
            fn(d, _i32([0, 2]))
    with pytest.raises(ValueError, match="no trace"):
        eng.replica().gradient(d, m2i)
