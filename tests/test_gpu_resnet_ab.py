"""The general alpha-beta rule on the batched bottleneck-ResNet encoder engine, on the GPU (ops.ResNetEncoder.relevance_alpha_beta,
model.compute_lrp_maps_ab, lrpx_conv_geom_ab / lrpx_conv_geom_ab_b6), in both conv modes.

Kernel criterion (tests/fp64_anchor.py): e = rel_err(got, fp64) <= C max(rel_err(fp32 CPU, fp64), FLOOR), C = 6, FLOOR = 1e-7, on the
tensors of tests/resnet_ab_cases.py, which tests/test_resnet_ab_host.py has found fit for it on the CPU; conv mode 1 must also leave
the three-product witness WITNESS_MARGIN above the bound.  End-to-end criterion: < 1e-4 of the map's maximum against
the reference's own fp64 results (tests/golden/resnet_ab.npz) and against the generic leaf driver under the same lrp_params."""
import os
import sys

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN, rel_err
from fp64_anchor import THREE, fp32_grade
from resnet_ab_cases import ALPHA, BETA, EDGE_CASES, MAP2IMG, N_MAPS, PROD_CASES, cached, case, reference

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet import TINY, bottleneck_net  # noqa: E402
from make_golden_resnet_engine import ENGINE  # noqa: E402

_CACHE = {}
SENTINEL = 12345.0
GUARD = 4096


def _mods():
    from lrp_amd import _lib, ops
    from lrp_amd.LRPtools import lrp_modules, lrp_wrapper
    return _lib, ops, lrp_modules, lrp_wrapper


def golden(name):
    if name not in _CACHE:
        _CACHE[name] = dict(np.load(os.path.join(GOLDEN, name)))
    return _CACHE[name]


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def to_nhwc(t):
    """CPU NCHW -> device (n, H W, c)"""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).contiguous().cuda()


def to_nchw(t, h, w):
    return t.view(t.shape[0], h, w, -1).permute(0, 3, 1, 2).cpu()


def fixture(name):
    """(inputs, net, {mode: traced engine}) of a golden fixture, built once and shared; the tests never call forward() on these engines"""
    if ("fx", name) not in _CACHE:
        _, ops, lrp_modules, _ = _mods()
        if name == "engine":
            G = golden("resnet_engine.npz")
            cfg, targets, m2i = ENGINE, G["targets"], list(G["map2img"])
        else:
            G = golden("resnet_tiny.npz")
            cfg, targets = TINY, np.stack([G["target1"][0], G["target2"][0], G["target1"][1], G["target2"][1]])
            m2i = list(golden("resnet_ab.npz")["tiny_map2img"])
        net = bottleneck_net(np.random.RandomState(int(G["seed"])), lrp_modules.resAdd, cfg["base"], cfg["blocks"]).cuda()
        x, t = torch.from_numpy(G["x"]).cuda(), torch.from_numpy(targets).cuda()
        engines = {}
        for mode in (0, 1):
            engines[mode] = ops.ResNetEncoder(net, conv_mode=mode)
            engines[mode].forward(x)
        torch.cuda.synchronize()
        _CACHE[("fx", name)] = (dict(x=x, targets=t, t_nhwc=ops.nchw_to_nhwc(t), m2i=m2i), net, engines)
    return _CACHE[("fx", name)]


def _delta(ops, before):
    return {k: v - before.get(k, 0) for k, v in ops.LAUNCHES.items() if v != before.get(k, 0)}


FORWARD_WORK = ("resnet_bn_act_coef", "resnet_coef_neg", "resnet_add_relu_coef", "resnet_maxpool_fwd")


def _no_forward_work(_lib, d):
    assert not any(k[1] == _lib.GEOM_FWD or k[0] in FORWARD_WORK for k in d), d


# ---- 1. the kernels at the edges ---------------------------------------------------------------------------------------------------------
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
        assert (self.view != SENTINEL).all(), what + ": left part of its output unwritten"
        assert torch.isfinite(self.view).all(), what + ": read beyond an operand (NaN surroundings)"


def in_nans(t):
    """the tensor on the device inside a NaN-filled allocation: a read beyond it poisons the result"""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), device="cuda")
    view = buf[GUARD:GUARD + t.numel()].view(*t.shape)
    view.copy_(t)
    return view


def _run_case(name, b6, addend, guarded):
    """the case on the device: (result NCHW on the CPU, fp64, fp32, three-product witness)"""
    _lib, ops, _, _ = _mods()
    c = case(name)
    wrap = in_nans if guarded else (lambda t: t)
    dev = cached(c, "dev", lambda: {k: to_nhwc(c[k]) for k in ("r", "xs", "qp", "qn", "addend")})
    pack = ops.conv_geom_pack_bf16x3 if b6 else ops.conv_geom_pack
    h, w = c["hw"]
    out = Guarded(N_MAPS, h * w, c["n_oc"]) if guarded else None
    got = ops.conv_geom_ab(wrap(dev["r"]), pack(c["rows"].cuda(), _lib.GEOM_BWD), N_MAPS, c["hw"], c["ohw"], c["geom"], c["kr"], c["n_oc"],
                           wrap(dev["xs"]), wrap(dev["qp"]), q2=wrap(dev["qn"]), scale=ALPHA, scale2=-BETA,
                           addend=wrap(dev["addend"]) if addend else None, map2img=_i32(MAP2IMG), n_img=2,
                           out=out.view if guarded else None, b6=b6)
    if guarded:
        out.check(f"conv_geom_ab b6={b6} {name} addend={addend}")
    torch.cuda.synchronize()
    refs = [cached(c, (what, addend), fn) for what, fn in (
        ("ref64", lambda: reference(c, torch.float64, addend=addend)), ("ref32", lambda: reference(c, torch.float32, addend=addend)),
        ("three", lambda: reference(c, torch.float64, THREE, addend=addend)))]
    return [to_nchw(got, h, w)] + refs


@pytest.mark.parametrize("b6", [False, True], ids=["mode0", "mode1"])
@pytest.mark.parametrize("group", ["pw", "pws2", "c3", "c3s2", "stem7"])
def test_kernel_edges(group, b6):
    """kr in {4, 20, 36, 52} (the half boundary inside a 32-channel chunk, the last chunk a quarter full) x n_oc in {4, 8, 20, 36, 52}
    (the stem: 8) at 11 x 9 pixels, three maps on two images [1, 0, 1], with and without addend: nothing written outside the output,
    everything inside written, no read outside an operand, fp32 grade against the fp64 formula"""
    for spec in EDGE_CASES:
        if not spec[0].startswith(group + "_"):
            continue
        for addend in (True, False):
            got, ref64, ref32, three = _run_case(spec[0], b6, addend, True)
            fp32_grade(got, ref64, ref32, three, f"conv_geom_ab{'_b6' if b6 else ''} {spec[0]} addend={addend}", margin_min=None if b6 else 0)
            if group == "pws2":             # rows / columns of odd index: no tap reaches their class
                want = case(spec[0])["addend"] if addend else torch.zeros_like(got)
                assert torch.equal(got[:, :, 1::2, :], want[:, :, 1::2, :]) and torch.equal(got[:, :, :, 1::2], want[:, :, :, 1::2])


@pytest.mark.parametrize("b6", [False, True], ids=["mode0", "mode1"])
@pytest.mark.parametrize("name", [c[0] for c in PROD_CASES])
def test_kernel_production_widths(name, b6):
    """kr = 2048 -> 512 at 7 x 7 (K = 4096) and 3x3 s2 512 -> 512 at 14 x 14; mode 1 with the witness margin"""
    got, ref64, ref32, three = _run_case(name, b6, True, False)
    fp32_grade(got, ref64, ref32, three, f"conv_geom_ab{'_b6' if b6 else ''} {name}", margin_min=None if b6 else 0)


# ---- 2. reduction to the preset ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["engine", "tiny"])
def test_alpha_1_beta_0_is_the_preset_bit_for_bit(name, mode):
    _lib, ops, _, _ = _mods()
    fx, _, engines = fixture(name)
    eng, m2i = engines[mode], _i32(fx["m2i"])
    want = eng.relevance(fx["t_nhwc"], m2i).clone()
    assert torch.equal(eng.relevance_alpha_beta(fx["t_nhwc"], m2i, alpha=1., beta=0.), want)
    before = dict(ops.LAUNCHES)
    r3 = eng.relevance_alpha_beta(fx["t_nhwc"], m2i, alpha=3., beta=0.)
    d = _delta(ops, before)
    single = "conv_geom_ab" + ("_b6" if mode else "")
    assert d.pop((single, _lib.GEOM_BWD)) == len(eng.plan.convs), d          # K = cout launches only: no W- half
    assert not any(k[0].startswith("conv_geom") for k in d), d
    _no_forward_work(_lib, d)
    assert torch.isfinite(r3).all() and not torch.equal(r3, want)


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pair", [(2., 1.), (1.5, .5)], ids=["a2_b1", "a1.5_b0.5"])
@pytest.mark.parametrize("name", ["engine", "tiny"])
def test_end_to_end(name, pair, mode):
    _, _, _, lrp_wrapper = _mods()
    AB = golden("resnet_ab.npz")
    fx, net, engines = fixture(name)
    alpha, beta = pair
    m2i = _i32(fx["m2i"])
    r = engines[mode].relevance_alpha_beta(fx["t_nhwc"], m2i, alpha, beta).clone()
    tag = "%s_a%g_b%g" % (name, alpha, beta)
    want64, want32 = AB[tag + "_r64"], AB[tag + "_r32"]
    assert tuple(r.shape) == want64.shape
    try:
        lrp_wrapper.add_lrp(net, lrp_params={"alpha": alpha, "beta": beta})
        for row, img in enumerate(fx["m2i"]):
            e, e32 = rel_err(r[row].cpu(), want64[row]), rel_err(want32[row], want64[row])
            generic = net.compute_lrp(fx["x"][img:img + 1].clone(), target=fx["targets"][row:row + 1])[0]      # a fresh sample tensor
            eg = rel_err(r[row].cpu(), generic.cpu())
            print(f"alpha-beta engine {tag} mode {mode} row {row} (image {img}): e {e:.2e}  e32 {e32:.2e}  e/e32 {e / e32:.2f}  "
                  f"against the generic driver {eg:.2e}  bound 1.0e-04")
            assert e < 1e-4, (row, e)
            assert eg < 1e-4, (row, eg)
        maps = net.compute_lrp_maps_ab(fx["x"], fx["targets"], m2i, conv_mode=mode)
        assert fx["x"].grad is None and not fx["x"].requires_grad
        assert torch.equal(maps, r), "compute_lrp_maps_ab differs from the engine"
    finally:
        lrp_wrapper.add_lrp(net)


# ---- 4. map independence and trace reuse -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_a_map_does_not_depend_on_the_other_maps_of_the_call(mode):
    fx, _, engines = fixture("engine")
    eng, t, m2i = engines[mode], fx["t_nhwc"], fx["m2i"]                   # m2i = [1, 0, 1]
    r = eng.relevance_alpha_beta(t, _i32(m2i)).clone()
    perm = [1, 0, 2]
    rp = eng.relevance_alpha_beta(t[perm].contiguous(), _i32([m2i[p] for p in perm]))
    for new, old in enumerate(perm):
        assert torch.equal(rp[new], r[old]), f"row {old} changed when the call's rows were permuted"
    for row in range(3):
        alone = eng.relevance_alpha_beta(t[row:row + 1].contiguous(), _i32([m2i[row]]))
        assert torch.equal(alone[0], r[row]), f"row {row} alone differs from row {row} in the call of three"
    ident = eng.relevance_alpha_beta(t[:2].contiguous(), None).clone()
    assert torch.equal(ident, eng.relevance_alpha_beta(t[:2].contiguous(), _i32([0, 1])))


@pytest.mark.parametrize("mode", [0, 1])
def test_the_trace_is_reused(mode):
    """qn is made at the first alpha-beta call after a forward and kept: the second call and a call with another (alpha, beta) launch
    no forward work; forward itself launches what it launched before this rule existed; a replica shares the dual packs"""
    _lib, ops, _, _ = _mods()
    fx, net, engines = fixture("engine")
    t, m2i = fx["t_nhwc"], _i32(fx["m2i"])
    eng = ops.ResNetEncoder(net, conv_mode=mode)
    n_convs, n_blocks = len(eng.plan.convs), len(eng.plan.blocks)
    ex, dual = ("conv_geom_ex_b6", "conv_geom_ab_dual_b6") if mode else ("conv_geom_ex", "conv_geom_ab_dual")
    with pytest.raises(ValueError, match="forward"):
        eng.relevance_alpha_beta(t, m2i)
    before = dict(ops.LAUNCHES)
    eng.forward(fx["x"])
    assert _delta(ops, before) == {(ex, _lib.GEOM_FWD): n_convs, ("resnet_bn_act_coef", None): n_convs,
                                   ("resnet_add_relu_coef", None): n_blocks, ("resnet_maxpool_fwd", None): 1}
    before = dict(ops.LAUNCHES)
    r1 = eng.relevance_alpha_beta(t, m2i, 2., 1.).clone()
    d = _delta(ops, before)
    assert d[(ex, _lib.GEOM_FWD)] == n_convs and d[("resnet_coef_neg", None)] == n_convs and d[(dual, _lib.GEOM_BWD)] == n_convs, d
    before = dict(ops.LAUNCHES)
    r2 = eng.relevance_alpha_beta(t, m2i, 2., 1.).clone()
    r3 = eng.relevance_alpha_beta(t, m2i, 1.5, .5).clone()
    d = _delta(ops, before)
    _no_forward_work(_lib, d)
    assert d == {(dual, _lib.GEOM_BWD): 2 * n_convs, ("resnet_add_split", None): 2 * n_blocks, ("resnet_maxpool_rel", None): 2,
                 ("resnet_stem_fold", None): 2}, d
    assert torch.equal(r1, r2) and not torch.equal(r1, r3)
    assert torch.equal(r1, engines[mode].relevance_alpha_beta(t, m2i, 2., 1.))
    rep = eng.replica()
    assert rep.trace is None and rep._ab_packs is eng._ab_packs and len(rep._ab_packs) == n_convs
    rep.forward(fx["x"])
    assert torch.equal(rep.relevance_alpha_beta(t, m2i, 2., 1.), r1)
    eng.forward(fx["x"])                                                   # a new trace: qn is made again
    before = dict(ops.LAUNCHES)
    assert torch.equal(eng.relevance_alpha_beta(t, m2i, 2., 1.), r1)
    assert _delta(ops, before)[("resnet_coef_neg", None)] == n_convs
    assert eng.trace_bytes(2, 45, 51, alpha_beta=True) - eng.trace_bytes(2, 45, 51) == sum(4 * q.numel() for q in eng.trace["q"])


def test_refusals():
    _lib, ops, _, _ = _mods()
    fx, _, engines = fixture("engine")
    eng, t = engines[0], fx["t_nhwc"]
    before = dict(ops.LAUNCHES)
    for bad in ((float("nan"), 1.), (2., float("-inf"))):
        with pytest.raises(ValueError, match="finite"):
            eng.relevance_alpha_beta(t, _i32(fx["m2i"]), *bad)
    with pytest.raises((_lib.LrpxError, ValueError), match="map2img"):
        eng.relevance_alpha_beta(t, _i32([0, 2, 1]))
    with pytest.raises(ValueError):
        eng.relevance_alpha_beta(t)                                        # three maps, two images, no map2img
    with pytest.raises(ValueError):
        eng.relevance_alpha_beta(t[:, :-1].contiguous(), _i32(fx["m2i"]))
    assert ops.LAUNCHES == before, "a refused call launched a kernel"


# ---- 5. the hook API ---------------------------------------------------------------------------------------------------------------------
def test_add_lrp_swaps_the_two_batched_entries():
    _, _, _, lrp_wrapper = _mods()
    _, net, _ = fixture("tiny")
    try:
        lrp_wrapper.add_lrp(net, lrp_params={"alpha": 2., "beta": 1.})
        assert hasattr(net, "compute_lrp_maps_ab") and not hasattr(net, "compute_lrp_maps")
        lrp_wrapper.add_lrp(net)
        assert hasattr(net, "compute_lrp_maps") and not hasattr(net, "compute_lrp_maps_ab")
        lrp_wrapper.add_lrp(net, lrp_params={"alpha": 1.5, "beta": .5, "ignore_bias": True})
        assert hasattr(net, "compute_lrp_maps_ab") and not hasattr(net, "compute_lrp_maps")
        assert not any(k.startswith("_lrpx_resnet") for k in net.__dict__)          # engines are built at the first call
    finally:
        lrp_wrapper.add_lrp(net)
    assert hasattr(net, "compute_lrp_maps") and not hasattr(net, "compute_lrp_maps_ab")
