"""The batched bottleneck-ResNet encoder engine on the GPU (ops.ResNetEncoder, model.compute_lrp_maps): one trace per
image, one relevance map per (target, map2img) row, against the reference's own fp64 results (tests/golden/resnet_tiny.npz,
resnet_engine.npz), against the generic leaf driver, and - for the extended conv entry at production widths - against the rule's
formula in fp64 on the CPU.

End-to-end criterion (the one tests/test_gpu_resnet.py uses on resnet_tiny.npz): < 1e-4 of the map's maximum.
Conv criterion (tests/fp64_anchor.py): rel_err(got, fp64) <= C * max(rel_err(fp32 CPU, fp64), FLOOR), C = 6, FLOOR = 1e-7."""
import os
import sys

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN, rel_err
from fp64_anchor import C, FLOOR

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet import TINY, bottleneck_net  # noqa: E402
from make_golden_resnet_engine import ENGINE  # noqa: E402

_CACHE = {}


def golden(name):
    if name not in _CACHE:
        _CACHE[name] = dict(np.load(os.path.join(GOLDEN, name)))
    return _CACHE[name]


def _mods():
    from lrp_amd import _lib, ops
    from lrp_amd.LRPtools import lrp_modules, lrp_wrapper
    return _lib, ops, lrp_modules, lrp_wrapper


def _net(cfg, seed):
    _, _, lrp_modules, _ = _mods()
    return bottleneck_net(np.random.RandomState(int(seed)), lrp_modules.resAdd, cfg["base"], cfg["blocks"]).cuda()


def _nhwc(t_nchw):
    _, ops, _, _ = _mods()
    return ops.nchw_to_nhwc(torch.as_tensor(t_nchw).cuda())


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def fixture2():
    """the engine on resnet_engine.npz, computed once and shared (read-only) by the tests that need it"""
    if "fx2" not in _CACHE:
        _, ops, _, _ = _mods()
        G = golden("resnet_engine.npz")
        net = _net(ENGINE, G["seed"])
        eng = ops.ResNetEncoder(net)
        eng.forward(torch.from_numpy(G["x"]).cuda())
        r = eng.relevance(_nhwc(G["targets"]), _i32(G["map2img"]))
        torch.cuda.synchronize()
        _CACHE["fx2"] = (G, net, eng, r.clone())
    return _CACHE["fx2"]


# ---- 1. reference parity on resnet_tiny.npz ----------------------------------------------------------------------------------------------
def test_engine_vs_reference_on_the_tiny_fixture():
    """B = 2, four maps on map2img = [0, 0, 1, 1]: rows 0 / 2 against r1, rows 1 / 3 against r2 - r1 (the stored second call carries the
    running sum of .grad), the reference's fp64 results"""
    _, ops, _, _ = _mods()
    T = golden("resnet_tiny.npz")
    eng = ops.ResNetEncoder(_net(TINY, T["seed"]))
    feats = eng.forward(torch.from_numpy(T["x"]).cuda())
    assert tuple(feats.shape) == (2, 5 * 5, 64)
    t1, t2 = T["target1"], T["target2"]
    r = eng.relevance(_nhwc(np.stack([t1[0], t2[0], t1[1], t2[1]])), _i32([0, 0, 1, 1])).cpu()
    assert tuple(r.shape) == (4, 3, 38, 34)
    d64, d32 = T["r264"] - T["r164"], T["r2"].astype(np.float64) - T["r1"]
    for row, (want64, want32) in enumerate([(T["r164"][0], T["r1"][0]), (d64[0], d32[0]), (T["r164"][1], T["r1"][1]), (d64[1], d32[1])]):
        e, e32 = rel_err(r[row], want64), rel_err(want32, want64)
        print(f"resnet engine tiny fixture row {row}: e {e:.2e}  e32 {e32:.2e}  e/e32 {e / e32:.2f}  bound 1.0e-04")
        assert e < 1e-4, (row, e)


# ---- 2. the second fixture: ragged tiles, unsorted map2img -------------------------------------------------------------------------------
def test_engine_vs_reference_on_the_ragged_fixture():
    G, _, _, r = fixture2()
    assert tuple(r.shape) == (3,) + tuple(G["x"].shape[1:])
    for row in range(3):
        e, e32 = rel_err(r[row].cpu(), G["r64"][row]), rel_err(G["r32"][row], G["r64"][row])
        print(f"resnet engine ragged fixture row {row} (image {G['map2img'][row]}): e {e:.2e}  e32 {e32:.2e}  e/e32 {e / e32:.2f}  bound 1.0e-04")
        assert e < 1e-4, (row, e)


# ---- 3. the hook API agrees with the generic driver --------------------------------------------------------------------------------------
def test_compute_lrp_maps_agrees_with_the_generic_driver():
    _, _, _, lrp_wrapper = _mods()
    G, net, _, _ = fixture2()
    lrp_wrapper.add_lrp(net)
    leaves = [m for m in net.modules() if len(list(m.children())) == 0]
    assert len(net._lrpx_hooks) == len(leaves) and all(len(m._forward_hooks) == 1 for m in leaves)     # what add_lrp did before
    x, targets, m2i = torch.from_numpy(G["x"]).cuda(), torch.from_numpy(G["targets"]).cuda(), G["map2img"]
    maps = net.compute_lrp_maps(x, targets, _i32(m2i))
    assert x.grad is None and not x.requires_grad
    for row, img in enumerate(m2i):
        sample = x[img:img + 1].clone()                                  # a fresh sample tensor per map: no running sum
        want = net.compute_lrp(sample, target=targets[row:row + 1])[0]
        e = rel_err(maps[row].cpu(), want.cpu())
        print(f"compute_lrp_maps row {row} against compute_lrp (generic driver): {e:.2e} of the map's maximum  bound 1.0e-04")
        assert e < 1e-4, (row, e)
    lrp_wrapper.add_lrp(net, lrp_params={"alpha": 2., "beta": 1.})
    assert not hasattr(net, "compute_lrp_maps")                          # the engine runs the preset only
    lrp_wrapper.add_lrp(net)
    assert hasattr(net, "compute_lrp_maps")


# ---- 4. map independence, bitwise --------------------------------------------------------------------------------------------------------
def test_a_map_does_not_depend_on_the_other_maps_of_the_call():
    G, _, eng, r = fixture2()                                             # r: map2img = [1, 0, 1]
    t = _nhwc(G["targets"])
    perm = [1, 0, 2]                                                      # rows permuted: map2img = [0, 1, 1]
    rp = eng.relevance(t[perm].contiguous(), _i32([G["map2img"][p] for p in perm]))
    for new, old in enumerate(perm):
        assert torch.equal(rp[new], r[old]), f"row {old} changed when the call's rows were permuted"
    for row in range(3):
        alone = eng.relevance(t[row:row + 1].contiguous(), _i32([G["map2img"][row]]))
        assert torch.equal(alone[0], r[row]), f"row {row} alone differs from row {row} in the call of three"
    ident = eng.relevance(t[:2].contiguous(), None)
    explicit = eng.relevance(t[:2].contiguous(), _i32([0, 1]))
    assert torch.equal(ident, explicit)


# ---- 5. the trace is computed once -------------------------------------------------------------------------------------------------------
def test_relevance_launches_no_forward_work():
    _lib, ops, _, _ = _mods()
    G, net, _, _ = fixture2()
    x, t = torch.from_numpy(G["x"]).cuda(), _nhwc(G["targets"])
    ta, tb = t[:2].contiguous(), t[1:3].contiguous()
    eng = ops.ResNetEncoder(net)
    eng.forward(x)
    n_convs = len(eng.plan.convs)
    trace_names = ("resnet_bn_act_coef", "resnet_add_relu_coef", "resnet_maxpool_fwd")
    before = dict(ops.LAUNCHES)
    ra, rb = eng.relevance(ta).clone(), eng.relevance(tb).clone()
    delta = {k: v - before.get(k, 0) for k, v in ops.LAUNCHES.items() if v != before.get(k, 0)}
    assert delta.get(("conv_geom_ex", _lib.GEOM_FWD), 0) == 0, delta      # the stem's Z belongs to the trace too
    assert all(delta.get((n, None), 0) == 0 for n in trace_names), delta
    assert delta[("conv_geom_ex", _lib.GEOM_BWD)] == 2 * n_convs, delta   # one transposed conv per conv and call
    assert delta[("resnet_add_split", None)] == 2 * len(eng.plan.blocks) and delta[("resnet_maxpool_rel", None)] == 2
    for tt, got in ((ta, ra), (tb, rb)):
        fresh = ops.ResNetEncoder(net)
        fresh.forward(x)
        assert torch.equal(fresh.relevance(tt), got)
    rep = eng.replica()
    assert rep.trace is None and rep.packs is eng.packs
    rep.forward(x)
    assert torch.equal(rep.relevance(ta), ra)


# ---- 6. the extended conv entry at production widths -------------------------------------------------------------------------------------
def _conv_ex_reference(x, q, r, addend, w, stride, padding, signed, dtype):
    """out[m] = x * convT(r[m] * q, W+) + addend[m]  (signed input: [x+ convT(., W+) | x- convT(., W-)] halves); NCHW on the CPU"""
    x, q, r, addend, w = (t.to(dtype) for t in (x, q, r, addend, w))
    s = r * q
    back = lambda wt: torch.nn.grad.conv2d_input((r.shape[0],) + tuple(x.shape[1:]), wt, s, stride=stride, padding=padding)
    if signed:
        return torch.cat([x.clamp(min=0) * back(w.clamp(min=0)), x.clamp(max=0) * back(w.clamp(max=0))], 1) + addend
    return x * back(w.clamp(min=0)) + addend


@pytest.mark.parametrize("k,stride,padding,cin,cout,hw,signed", [
    (1, 1, 0, 2048, 512, 7, False), (3, 2, 1, 512, 512, 14, False), (1, 2, 0, 256, 512, 14, False), (7, 2, 3, 3, 64, 32, True)],
    ids=["pw_2048_512_7", "c3s2_512_14", "pws2_256_512_14", "stem7_32"])
def test_conv_geom_ex_production_widths(k, stride, padding, cin, cout, hw, signed):
    """n_img = 1, three maps on map2img = [0, 0, 0], with an input multiplier and an addend"""
    _lib, ops, _, _ = _mods()
    g = torch.Generator().manual_seed(300 + k + cin)
    n_maps = 3
    ohw = (hw + 2 * padding - k) // stride + 1
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    x = torch.randn(1, cin, hw, hw, generator=g)
    if not signed:
        x = x.clamp(min=0)
    q = torch.rand(1, cout, ohw, ohw, generator=g) + 0.5
    r = torch.randn(n_maps, cout, ohw, ohw, generator=g)
    n_oc = 8 if signed else cin
    addend = torch.randn(n_maps, n_oc, hw, hw, generator=g) * 0.1
    to_nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).contiguous().cuda()
    if signed:          # the split image [x+ | x- | 0 0] and the weight rows [W+ | W- | 0 0]
        pad = torch.zeros(1, 8 - 2 * cin, hw, hw)
        xs = to_nhwc(torch.cat([x.clamp(min=0), x.clamp(max=0), pad], 1))
        wb = torch.cat([w.clamp(min=0), w.clamp(max=0), torch.zeros(cout, 8 - 2 * cin, k, k)], 1)
    else:
        xs, wb = to_nhwc(x), w.clamp(min=0)
    pb = ops.conv_geom_pack(wb.cuda(), _lib.GEOM_BWD)
    got = ops.conv_geom_ex(to_nhwc(r), pb, _lib.GEOM_BWD, n_maps, (hw, hw), (ohw, ohw), (k, k, stride, stride, padding, padding), cout, n_oc,
                           x=xs, q=to_nhwc(q), addend=to_nhwc(addend), map2img=_i32([0, 0, 0]), n_img=1)
    torch.cuda.synchronize()
    got = got.view(n_maps, hw, hw, n_oc).permute(0, 3, 1, 2).cpu()
    refs = []
    for dtype in (torch.float64, torch.float32):
        ref = _conv_ex_reference(x, q, r, addend[:, :2 * cin] if signed else addend, w, stride, padding, signed, dtype)
        if signed:      # the two zero columns behind the halves carry the addend alone
            ref = torch.cat([ref, addend[:, 2 * cin:].to(dtype)], 1)
        refs.append(ref)
    e, e32 = rel_err(got, refs[0]), rel_err(refs[1], refs[0])
    bound = C * max(e32, FLOOR)
    print(f"conv_geom_ex {k}x{k} s{stride} {cin}->{cout} at {hw}x{hw}: e {e:.2e}  e32 {e32:.2e}  e/max(e32,FLOOR) {e / max(e32, FLOOR):.2f}  bound {bound:.2e}")
    assert e <= bound, f"rel_err vs fp64 {e:.3e} > {C} x max(fp32's {e32:.3e}, {FLOOR:.0e})"


# ---- 7. guard bands ----------------------------------------------------------------------------------------------------------------------
SENTINEL = 12345.0
GUARD = 4096


class Guarded:
    """an output of `shape` embedded in a larger allocation filled with a sentinel"""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
        self.view = self.buf[GUARD:GUARD + n].view(*shape)

    def check(self, what):
        torch.cuda.synchronize()
        assert (self.buf[:GUARD] == SENTINEL).all(), what + ": wrote before its output"
        assert (self.buf[-GUARD:] == SENTINEL).all(), what + ": wrote past its output"
        assert (self.view != SENTINEL).all() and torch.isfinite(self.view).all(), what + ": left part of its output unwritten"


def test_new_kernels_never_write_outside_their_outputs():
    """every new kernel that writes a caller's buffer, at pixel and channel counts that are no multiple of a 64 x 64 tile or a 256-thread
    block: 3 maps on 2 images, 11 x 9 pixels, 20 / 36 channels"""
    _lib, ops, _, _ = _mods()
    g = torch.Generator().manual_seed(29)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()
    n_img, n_maps, h, w, c, co = 2, 3, 11, 9, 20, 36
    m2i = _i32([1, 0, 1])
    for geom in [(3, 3, 2, 2, 1, 1), (1, 1, 2, 2, 0, 0), (7, 7, 2, 2, 3, 3), (1, 1, 1, 1, 0, 0)]:
        kh, kw, sh, sw, ph, pw = geom
        oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
        wt = torch.randn(co, c, kh, kw, generator=g)
        out = Guarded(n_img, oh * ow, co)
        ops.conv_geom_ex(rnd(n_img, h * w, c), ops.conv_geom_pack(wt.cuda(), _lib.GEOM_FWD), _lib.GEOM_FWD, n_img, (h, w), (oh, ow), geom, c, co,
                         out=out.view)
        out.check(f"conv_geom_ex FWD {geom}")
        out = Guarded(n_maps, h * w, c)
        ops.conv_geom_ex(rnd(n_maps, oh * ow, co), ops.conv_geom_pack(wt.cuda(), _lib.GEOM_BWD), _lib.GEOM_BWD, n_maps, (h, w), (oh, ow), geom,
                         co, c, x=rnd(n_img, h * w, c).abs() + 0.5, q=rnd(n_img, oh * ow, co).abs() + 0.5, addend=rnd(n_maps, h * w, c),
                         map2img=m2i, n_img=n_img, out=out.view)
        out.check(f"conv_geom_ex BWD {geom}")
    act, q = Guarded(n_img, h * w, c), Guarded(n_img, h * w, c)
    ops.resnet_bn_act_coef(rnd(n_img, h * w, 2 * c), rnd(c), rnd(c), act.view, q.view, True)
    act.check("resnet_bn_act_coef act")
    q.check("resnet_bn_act_coef q")
    o, c1, c2 = Guarded(n_img, h * w, c), Guarded(n_img, h * w, c), Guarded(n_img, h * w, c)
    ops.resnet_add_relu_coef(rnd(n_img, h * w, c), rnd(n_img, h * w, c), o.view, c1.view, c2.view)
    for t, name in ((o, "out"), (c1, "c1"), (c2, "c2")):
        t.check("resnet_add_relu_coef " + name)
    win, (oh, ow) = (3, 3, 2, 2, 1, 1), (6, 5)
    x = rnd(n_img, h * w, c)
    y = Guarded(n_img, oh * ow, c)
    ops.resnet_maxpool_fwd(x, y.view, n_img, (h, w), (oh, ow), c, win)
    y.check("resnet_maxpool_fwd")
    want = torch.nn.functional.max_pool2d(x.view(n_img, h, w, c).permute(0, 3, 1, 2), 3, 2, 1)
    assert torch.equal(y.view.view(n_img, oh, ow, c).permute(0, 3, 1, 2), want)
    r_in = Guarded(n_maps, h * w, c)
    ops.resnet_maxpool_rel(x, rnd(n_maps, oh * ow, c), m2i, r_in.view, n_maps, n_img, (h, w), (oh, ow), c, win)
    r_in.check("resnet_maxpool_rel")
    r1, r2 = Guarded(n_maps, h * w, c), Guarded(n_maps, h * w, c)
    ops.resnet_add_split(rnd(n_maps, h * w, c), rnd(n_img, h * w, c), rnd(n_img, h * w, c), m2i, r1.view, r2.view, n_maps, n_img)
    r1.check("resnet_add_split r1")
    r2.check("resnet_add_split r2")
    out = Guarded(n_maps, 3, h, w)
    ops.resnet_stem_fold(rnd(n_maps, h * w, 8), out.view, n_maps, 3, 3, 8, h * w)
    out.check("resnet_stem_fold")


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    _lib, ops, _, _ = _mods()
    G, net, _, _ = fixture2()
    t = _nhwc(G["targets"])
    eng = ops.ResNetEncoder(net)
    with pytest.raises(ValueError, match="forward"):
        eng.relevance(t)                                                  # no trace yet
    eng.forward(torch.from_numpy(G["x"]).cuda())
    before = dict(ops.LAUNCHES)
    for bad in ([0, 2, 1], [0, -1, 1]):
        with pytest.raises((_lib.LrpxError, ValueError), match="map2img"):
            eng.relevance(t, _i32(bad))
    with pytest.raises((_lib.LrpxError, ValueError), match="map2img"):
        eng.relevance(t, torch.tensor([0, 1, 1], dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        eng.relevance(t[:, :-1].contiguous(), _i32([0, 1, 1]))            # wrong shape
    with pytest.raises(ValueError):
        eng.relevance(t)                                                  # three maps, two images, no map2img
    assert ops.LAUNCHES == before, "a refused call launched a kernel"
    with pytest.raises((_lib.LrpxError, ValueError), match="map2img"):
        ops.conv_geom_ex(torch.zeros(2, 4, 4, device="cuda"), torch.zeros(1024, device="cuda"), _lib.GEOM_BWD, 2, (2, 2), (2, 2),
                         (1, 1, 1, 1, 0, 0), 4, 4, x=torch.zeros(1, 4, 4, device="cuda"), map2img=_i32([0, 1]), n_img=1)
    assert ops.LAUNCHES == before
