"""Conv mode 1 of the batched bottleneck-ResNet engine on the GPU (csrc/conv_geom_b6.hip, ops.ResNetEncoder(conv_mode=1)):
`lrpx_conv_geom_ex_b6` against fp64 with the fp32-grade criterion of tests/fp64_anchor.py (the inputs are the ones
tests/test_resnet_b6_host.py found fit for it), its edges in guard bands and NaN-filled surroundings against `lrpx_conv_geom_ex`, and
the engine end to end against the reference's fp64 results and against its own mode 0.

End-to-end criterion: < 1e-4 of the map's maximum."""
import os
import sys

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN, rel_err
from fp64_anchor import C, C_FORWARD, FLOOR, THREE, emulate, fp32_grade
from resnet_b6_cases import BWD_CASES, N_MAPS, bwd_case, bwd_device_operands, bwd_reference

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


def to_nhwc(t):
    """CPU NCHW -> device (n, H W, c)"""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).contiguous().cuda()


def to_nchw(t, h, w):
    return t.view(t.shape[0], h, w, -1).permute(0, 3, 1, 2).cpu()


def fixture2():
    """both engines on resnet_engine.npz, computed once and shared (read-only) by the tests that need them"""
    if "fx2" not in _CACHE:
        _, ops, _, _ = _mods()
        G = golden("resnet_engine.npz")
        net = _net(ENGINE, G["seed"])
        x, t, m2i = torch.from_numpy(G["x"]).cuda(), _nhwc(G["targets"]), _i32(G["map2img"])
        res = {}
        for mode in (0, 1):
            eng = ops.ResNetEncoder(net, conv_mode=mode)
            eng.forward(x)
            res[mode] = (eng, eng.relevance(t, m2i).clone())
        torch.cuda.synchronize()
        _CACHE["fx2"] = (G, net, res)
    return _CACHE["fx2"]


# ---- 1. transposed direction, fp32 grade -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in BWD_CASES])
def test_transposed_direction_is_fp32_grade(name):
    """n_img = 1, three maps on map2img = [0, 0, 0], with q and an addend, on the tensors of tests/resnet_b6_cases.py"""
    _lib, ops, _, _ = _mods()
    c = bwd_case(name)
    k, s, p, hw, ohw = c["k"], c["stride"], c["padding"], c["hw"], c["ohw"]
    xs, wb = bwd_device_operands(c)
    pb = ops.conv_geom_pack_bf16x3(wb.cuda(), _lib.GEOM_BWD)
    got = ops.conv_geom_ex(to_nhwc(c["r"]), pb, _lib.GEOM_BWD, N_MAPS, (hw, hw), (ohw, ohw), (k, k, s, s, p, p), c["cout"], c["n_oc"],
                           x=to_nhwc(xs), q=to_nhwc(c["q"]), addend=to_nhwc(c["addend"]), map2img=_i32([0] * N_MAPS), n_img=1, b6=True)
    torch.cuda.synchronize()
    fp32_grade(to_nchw(got, hw, hw), bwd_reference(c, torch.float64), bwd_reference(c, torch.float32),
               bwd_reference(c, torch.float64, THREE), f"conv_geom_ex_b6 BWD {name}")


# ---- 2. forward direction: the trace's stacked [W | W+] columns --------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,padding,cin,cout,hw", [(1, 1, 0, 2048, 512, 7), (3, 2, 1, 512, 512, 14), (7, 2, 3, 8, 64, 17)],
                         ids=["pw_2048_2x512_7", "c3s2_512_2x512_14", "stem7_k8_17"])
def test_forward_direction_is_fp32_grade(k, stride, padding, cin, cout, hw):
    """non-negative inputs: no witness margin and the forward bound (fp64_anchor.py, C_FORWARD)"""
    _lib, ops, _, _ = _mods()
    g = torch.Generator().manual_seed(500 + k + cin)
    n = 2
    ohw = (hw + 2 * padding - k) // stride + 1
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    ws = torch.cat([w, w.clamp(min=0)], 0)
    x = torch.randn(n, cin, hw, hw, generator=g).clamp(min=0) * torch.exp(torch.randn(n, cin, hw, hw, generator=g))
    conv = lambda a, b: torch.nn.functional.conv2d(a, b, stride=stride, padding=padding)
    got = ops.conv_geom_ex(to_nhwc(x), ops.conv_geom_pack_bf16x3(ws.cuda(), _lib.GEOM_FWD), _lib.GEOM_FWD, n, (hw, hw), (ohw, ohw),
                           (k, k, stride, stride, padding, padding), cin, 2 * cout, b6=True)
    torch.cuda.synchronize()
    fp32_grade(to_nchw(got, ohw, ohw), conv(x.double(), ws.double()), conv(x, ws), emulate(conv, x, ws, THREE),
               f"conv_geom_ex_b6 FWD {k}x{k} s{stride} {cin}->2x{cout} at {hw}x{hw}", c=C_FORWARD, margin_min=0)


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------------
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
        assert (self.view != SENTINEL).all(), what + ": left part of its output unwritten"
        assert torch.isfinite(self.view).all(), what + ": read beyond an operand (NaN surroundings)"


def in_nans(t):
    """the tensor on the device inside a NaN-filled allocation: a read beyond it poisons the result"""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), device="cuda")
    view = buf[GUARD:GUARD + t.numel()].view(*t.shape)
    view.copy_(t)
    return view


EDGES = [((3, 3, 2, 2, 1, 1), 20, 36), ((1, 1, 2, 2, 0, 0), 20, 36), ((7, 7, 2, 2, 3, 3), 20, 36), ((1, 1, 1, 1, 0, 0), 20, 36),
         ((1, 1, 1, 1, 0, 0), 4, 52), ((1, 1, 1, 1, 0, 0), 52, 4), ((1, 1, 1, 1, 0, 0), 8, 20), ((1, 1, 1, 1, 0, 0), 20, 8)]


@pytest.mark.parametrize("geom,c,co", EDGES, ids=["c3s2", "pws2", "c7s2", "pw", "pw_4_52", "pw_52_4", "pw_8_20", "pw_20_8"])
def test_edges_in_guard_bands_against_the_fp32_kernel(geom, c, co):
    """3 maps on 2 images [1, 0, 1], 11 x 9 pixels, channel counts that fill no tile: K = 4, 20, 36 and 52 (the second k-step of the last
    chunk a quarter full), n_oc = 8 (one column block, a wave with nothing to store); both directions.  Nothing written outside the
    output, everything inside written, no read outside an operand, and the error against fp64 within C x the fp32 kernel's."""
    _lib, ops, _, _ = _mods()
    g = torch.Generator().manual_seed(29 + c + 3 * co + geom[0])
    rnd = lambda *s: torch.randn(*s, generator=g)
    n_img, n_maps, h, w = 2, 3, 11, 9
    m2i = [1, 0, 1]
    kh, kw, sh, sw, ph, pw = geom
    oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    wt = rnd(co, c, kh, kw)
    F = torch.nn.functional

    # forward
    x = rnd(n_img, c, h, w)
    xin = in_nans(to_nhwc(x))
    ref64 = F.conv2d(x.double(), wt.double(), stride=(sh, sw), padding=(ph, pw))
    got = {}
    for b6 in (False, True):
        pack = ops.conv_geom_pack_bf16x3 if b6 else ops.conv_geom_pack
        out = Guarded(n_img, oh * ow, co)
        ops.conv_geom_ex(xin, pack(wt.cuda(), _lib.GEOM_FWD), _lib.GEOM_FWD, n_img, (h, w), (oh, ow), geom, c, co, out=out.view, b6=b6)
        out.check(f"conv_geom_ex FWD b6={b6} {geom}")
        got[b6] = to_nchw(out.view, oh, ow)
    e, e32 = rel_err(got[True], ref64), rel_err(got[False], ref64)
    print(f"conv_geom_ex_b6 FWD {geom} {c}->{co}: e {e:.2e}  fp32 kernel {e32:.2e}  bound {C * max(e32, FLOOR):.2e}")
    assert e <= C * max(e32, FLOOR)

    # transposed
    r, q, xm, addend = rnd(n_maps, co, oh, ow), rnd(n_img, co, oh, ow).abs() + 0.5, rnd(n_img, c, h, w).abs() + 0.5, rnd(n_maps, c, h, w)
    s64 = r.double() * q.double()[m2i]
    ref64 = xm.double()[m2i] * torch.nn.grad.conv2d_input((n_maps, c, h, w), wt.double(), s64, stride=(sh, sw), padding=(ph, pw)) \
        + addend.double()
    ops_in = [in_nans(to_nhwc(t)) for t in (r, xm, q, addend)]
    for b6 in (False, True):
        pack = ops.conv_geom_pack_bf16x3 if b6 else ops.conv_geom_pack
        out = Guarded(n_maps, h * w, c)
        ops.conv_geom_ex(ops_in[0], pack(wt.cuda(), _lib.GEOM_BWD), _lib.GEOM_BWD, n_maps, (h, w), (oh, ow), geom, co, c, x=ops_in[1],
                         q=ops_in[2], addend=ops_in[3], map2img=_i32(m2i), n_img=n_img, out=out.view, b6=b6)
        out.check(f"conv_geom_ex BWD b6={b6} {geom}")
        got[b6] = to_nchw(out.view, h, w)
    e, e32 = rel_err(got[True], ref64), rel_err(got[False], ref64)
    print(f"conv_geom_ex_b6 BWD {geom} {co}->{c}: e {e:.2e}  fp32 kernel {e32:.2e}  bound {C * max(e32, FLOOR):.2e}")
    assert e <= C * max(e32, FLOOR)
    if geom == (1, 1, 2, 2, 0, 0):          # rows / columns of odd index: no tap reaches their class
        assert torch.equal(got[True][:, :, 1::2, :], addend[:, :, 1::2, :]) and torch.equal(got[True][:, :, :, 1::2], addend[:, :, :, 1::2])


# ---- 4. map independence, bitwise --------------------------------------------------------------------------------------------------------
def test_a_map_does_not_depend_on_the_other_maps_of_the_call():
    G, _, res = fixture2()
    eng, r = res[1]                                                       # r: map2img = [1, 0, 1]
    assert eng.conv_mode == 1
    t = _nhwc(G["targets"])
    perm = [1, 0, 2]
    rp = eng.relevance(t[perm].contiguous(), _i32([G["map2img"][p] for p in perm]))
    for new, old in enumerate(perm):
        assert torch.equal(rp[new], r[old]), f"row {old} changed when the call's rows were permuted"
    for row in range(3):
        alone = eng.relevance(t[row:row + 1].contiguous(), _i32([G["map2img"][row]]))
        assert torch.equal(alone[0], r[row]), f"row {row} alone differs from row {row} in the call of three"
    ident = eng.relevance(t[:2].contiguous(), None)
    explicit = eng.relevance(t[:2].contiguous(), _i32([0, 1]))
    assert torch.equal(ident, explicit)


# ---- 5. the engine end to end ------------------------------------------------------------------------------------------------------------
def _against_mode0(what, r1, r0):
    for row in range(r1.shape[0]):
        d = rel_err(r1[row].cpu(), r0[row].cpu())
        print(f"{what} row {row}: mode 1 against mode 0 {d:.2e} of the map's maximum  bound 1.0e-04")
        assert d < 1e-4, (row, d)
    # Z+ from six products of non-negative operands is zero exactly where the fp32 sum is (a0 b0 != 0 whenever a b != 0)
    assert torch.equal(r1 == 0, r0 == 0), what + ": the zero pattern differs from mode 0's"


def test_engine_vs_reference_on_the_tiny_fixture():
    _, ops, _, _ = _mods()
    T = golden("resnet_tiny.npz")
    net = _net(TINY, T["seed"])
    t1, t2 = T["target1"], T["target2"]
    x, t, m2i = torch.from_numpy(T["x"]).cuda(), _nhwc(np.stack([t1[0], t2[0], t1[1], t2[1]])), _i32([0, 0, 1, 1])
    r = {}
    for mode in (0, 1):
        eng = ops.ResNetEncoder(net, conv_mode=mode)
        eng.forward(x)
        r[mode] = eng.relevance(t, m2i).clone()
    assert tuple(r[1].shape) == (4, 3, 38, 34)
    d64, d32 = T["r264"] - T["r164"], T["r2"].astype(np.float64) - T["r1"]
    for row, (want64, want32) in enumerate([(T["r164"][0], T["r1"][0]), (d64[0], d32[0]), (T["r164"][1], T["r1"][1]), (d64[1], d32[1])]):
        e, e32 = rel_err(r[1][row].cpu(), want64), rel_err(want32, want64)
        print(f"resnet engine mode 1 tiny fixture row {row}: e {e:.2e}  e32 {e32:.2e}  e/e32 {e / e32:.2f}  bound 1.0e-04")
        assert e < 1e-4, (row, e)
    _against_mode0("tiny fixture", r[1], r[0])


def test_engine_vs_reference_on_the_ragged_fixture():
    G, _, res = fixture2()
    r = res[1][1]
    assert tuple(r.shape) == (3,) + tuple(G["x"].shape[1:])
    for row in range(3):
        e, e32 = rel_err(r[row].cpu(), G["r64"][row]), rel_err(G["r32"][row], G["r64"][row])
        print(f"resnet engine mode 1 ragged fixture row {row} (image {G['map2img'][row]}): e {e:.2e}  e32 {e32:.2e}  e/e32 {e / e32:.2f}  "
              f"bound 1.0e-04")
        assert e < 1e-4, (row, e)
    _against_mode0("ragged fixture", r, res[0][1])


# ---- 6. what runs ------------------------------------------------------------------------------------------------------------------------
def test_mode_1_runs_the_b6_kernel_only():
    _lib, ops, _, lrp_wrapper = _mods()
    G, net, res = fixture2()
    x, t, m2i = torch.from_numpy(G["x"]).cuda(), _nhwc(G["targets"]), _i32(G["map2img"])
    delta = lambda before: {k: v - before.get(k, 0) for k, v in ops.LAUNCHES.items() if v != before.get(k, 0)}
    eng = ops.ResNetEncoder(net, conv_mode=1)
    n_convs = len(eng.plan.convs)
    before = dict(ops.LAUNCHES)
    eng.forward(x)
    d = delta(before)
    assert d.get(("conv_geom_ex_b6", _lib.GEOM_FWD)) == n_convs and ("conv_geom_ex_b6", _lib.GEOM_BWD) not in d, d
    before = dict(ops.LAUNCHES)
    r = eng.relevance(t, m2i)
    d = delta(before)
    assert d.get(("conv_geom_ex_b6", _lib.GEOM_BWD)) == n_convs and ("conv_geom_ex_b6", _lib.GEOM_FWD) not in d, d
    assert not any(k[0] == "conv_geom_ex" for k in d), d
    assert torch.equal(r, res[1][1])
    rep = eng.replica()
    assert rep.trace is None and rep.packs is eng.packs and rep.conv_mode == 1
    assert all(p["fwd"].dtype == torch.uint8 and p["bwd"].dtype == torch.uint8 for p in eng.packs)      # the bf16x3 packs only

    before = dict(ops.LAUNCHES)
    e0 = ops.ResNetEncoder(net)
    assert e0.conv_mode == 0
    e0.forward(x)
    e0.relevance(t, m2i)
    d = delta(before)
    assert not any(k[0] == "conv_geom_ex_b6" for k in d), d
    assert d[("conv_geom_ex", _lib.GEOM_FWD)] == n_convs and d[("conv_geom_ex", _lib.GEOM_BWD)] == n_convs, d

    lrp_wrapper.add_lrp(net)
    tn = torch.from_numpy(G["targets"]).cuda()
    m1 = net.compute_lrp_maps(x, tn, m2i, conv_mode=1)
    assert torch.equal(m1, res[1][1])
    m0 = net.compute_lrp_maps(x, tn, m2i)
    assert torch.equal(m0, res[0][1])
    assert net._lrpx_resnet.conv_mode == 0 and net._lrpx_resnet_mode1.conv_mode == 1
    e1 = net._lrpx_resnet_mode1
    net.compute_lrp_maps(x, tn, m2i, conv_mode=1)
    assert net._lrpx_resnet_mode1 is e1 and net._lrpx_resnet.conv_mode == 0       # one engine per mode, kept
    with pytest.raises(ValueError, match="modes 0"):
        net.compute_lrp_maps(x, tn, m2i, conv_mode=2)
