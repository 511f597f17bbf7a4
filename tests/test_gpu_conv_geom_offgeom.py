"""The runtime-geometry contraction engine (csrc/conv_geom_kernel.h) on the GPU at geometries outside ResNet-50's: even kernels, strides
of 3 and 4, sh != sw, padding other than k // 2, a stride above the kernel with padding, classes with 2 and 1 (and 3 and 2) taps per
axis, a class with no pixels, 121 taps, a 64-pixel tile that spans five maps - every geometry of tests/conv_geom_offgeom_cases.py through
every entry (lrpx_conv_geom, _ex, _ab, _grad, and the _b6 forms), each against its formula in fp64 on the CPU.

Criterion (tests/fp64_anchor.py, as test_conv_geom_grad_against_the_formula applies it to this kernel family):
rel_err(got, fp64) <= C * max(rel_err(fp32 CPU, fp64), FLOOR).  These are placement tests - a misplaced element is an O(1) error - so
no witness margin is asked; tests/test_conv_geom_offgeom_host.py has decided on the CPU that the six plane products of conv mode 1 pass
the bound on exactly these tensors.  Every output is pre-filled with NaN and must come back finite; pixels that no window reaches
(k2s2, k4s4, gap) hold exact zeros without an addend and the addend's bytes with one."""
import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import rel_err
from conv_geom_offgeom_cases import (AB_CHANNELS, ALPHA, BETA, CHANNELS, GEOMS, UNREACHED, ab_case, case, reference, unreached)
from fp64_anchor import C, FLOOR

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARD = 4096
MODES = pytest.mark.parametrize("b6", [False, True], ids=["fp32", "b6"])
ALL_GEOMS = pytest.mark.parametrize("gid", list(GEOMS))


def _mods():
    from lrp_amd import _lib, ops
    return _lib, ops


def _i32(v):
    return torch.tensor([int(a) for a in v], dtype=torch.int32, device="cuda")


def _rows(t_nchw):
    """(n, c, h, w) on the CPU -> (n, h w, c) on the device"""
    n, c, h, w = t_nchw.shape
    return t_nchw.permute(0, 2, 3, 1).reshape(n, h * w, c).float().contiguous().cuda()


def _nchw(rows, hw):
    return rows.cpu().view(rows.shape[0], hw[0], hw[1], -1).permute(0, 3, 1, 2)


def _nans(n, pix, c):
    return torch.full((n, pix, c), float("nan"), device="cuda")


def _pack(ops, b6):
    return ops.conv_geom_pack_bf16x3 if b6 else ops.conv_geom_pack


class Worst:
    """the worst e / max(e32, FLOOR) per entry of one test, printed once"""

    def __init__(self, what):
        self.what, self.seen = what, {}

    def check(self, got_rows, entry, c, addend):
        """got (n, pixels, n_oc) on the device against the entry's formula; addend: the NCHW addend the run carried, or None"""
        hw = c["ohw"] if entry == "fwd" else c["hw"]
        got = _nchw(got_rows, hw)
        what = f"{self.what} {entry} {c['gid']} K {c.get('k', c.get('kr'))} n_oc {c['n_oc']}"
        assert torch.isfinite(got).all(), what + ": part of the NaN-filled output was not written (or a NaN was read)"
        ref64, ref32 = reference(entry, c, torch.float64), reference(entry, c, torch.float32)
        assert got.shape == ref64.shape
        e, e32 = rel_err(got, ref64), rel_err(ref32, ref64)
        self.seen[entry] = max(self.seen.get(entry, 0.), e / max(e32, FLOOR))
        assert e <= C * max(e32, FLOOR), f"{what}: rel_err vs fp64 {e:.3e} > {C} x max(fp32's {e32:.3e}, {FLOOR:.0e})"
        if entry != "fwd" and c["gid"] in UNREACHED:
            dead = unreached(c["gid"])
            assert dead.any() and not dead.all()
            if addend is None:
                assert not got[:, :, dead].any(), what + ": a pixel that no window reaches is not an exact zero"
            else:
                assert torch.equal(got[:, :, dead].view(torch.int32), addend[:, :, dead].view(torch.int32)), \
                    what + ": a pixel that no window reaches does not hold the addend's bytes"

    def report(self):
        print(f"off-geometry {self.what}: worst e / max(e32, FLOOR) per entry: " + "  ".join(f"{k} {v:.2f}" for k, v in self.seen.items())
              + f"  bound {C:.0f}")


# ---- 1. forward ----------------------------------------------------------------------------------------------------------------------------
@MODES
@ALL_GEOMS
def test_forward(gid, b6):
    """lrpx_conv_geom with bias (the fp32 run only: it has no _b6 form) and lrpx_conv_geom_ex / _ex_b6 with bias"""
    _lib, ops = _mods()
    worst = Worst(f"forward {gid} {'b6' if b6 else 'fp32'}")
    for k, n_oc in CHANNELS:
        c = case(gid, k, n_oc)
        (h, w), (oh, ow), n = c["hw"], c["ohw"], c["n"]
        xin, bias = _rows(c["xin"]), c["bias"].cuda()
        pack = _pack(ops, b6)(c["wf"].cuda(), _lib.GEOM_FWD)
        if not b6:
            out = _nans(n, oh * ow, n_oc)
            ops.conv_geom(xin, pack, _lib.GEOM_FWD, n, (h, w), (oh, ow), c["geom"], k, n_oc, bias=bias, out=out)
            worst.check(out, "fwd", c, None)
        out = _nans(n, oh * ow, n_oc)
        ops.conv_geom_ex(xin, pack, _lib.GEOM_FWD, n, (h, w), (oh, ow), c["geom"], k, n_oc, bias=bias, out=out, b6=b6)
        worst.check(out, "fwd", c, None)
    worst.report()


# ---- 2. transposed: the relevance entries ----------------------------------------------------------------------------------------------------
@MODES
@ALL_GEOMS
def test_transposed_ex(gid, b6):
    """lrpx_conv_geom with x (the fp32 run only) and lrpx_conv_geom_ex / _ex_b6 with x, q and map2img, with and without an addend"""
    _lib, ops = _mods()
    worst = Worst(f"transposed {gid} {'b6' if b6 else 'fp32'}")
    for k, n_oc in CHANNELS:
        c = case(gid, k, n_oc)
        (h, w), n, m2i = c["hw"], c["n"], c["m2i"]
        args = (n, c["hw"], c["ohw"], c["geom"], k, n_oc)
        r, x, q, addend = _rows(c["r"]), _rows(c["x"]), _rows(c["q"]), _rows(c["addend"])
        pack = _pack(ops, b6)(c["w"].cuda(), _lib.GEOM_BWD)
        if not b6:
            out = _nans(n, h * w, n_oc)
            ops.conv_geom(r, pack, _lib.GEOM_BWD, *args, x=x[m2i].contiguous(), out=out)
            worst.check(out, "plain", c, None)
        for entry, add in (("ex", addend), ("ex_noadd", None)):
            out = _nans(n, h * w, n_oc)
            ops.conv_geom_ex(r, pack, _lib.GEOM_BWD, *args, x=x, q=q, addend=add, map2img=_i32(m2i), n_img=c["n_img"], out=out, b6=b6)
            worst.check(out, entry, c, None if add is None else c["addend"])
    worst.report()


@MODES
@ALL_GEOMS
def test_transposed_ab(gid, b6):
    """lrpx_conv_geom_ab / _ab_b6: the W+ half alone (q2 None, no addend) and the dual contraction over [W+ ; W-] with an addend"""
    _lib, ops = _mods()
    worst = Worst(f"alpha-beta {gid} {'b6' if b6 else 'fp32'}")
    for kr, n_oc in AB_CHANNELS:
        c = ab_case(gid, kr, n_oc)
        (h, w), n, m2i = c["hw"], c["n"], _i32(c["m2i"])
        args = (n, c["hw"], c["ohw"], c["geom"], kr, n_oc)
        r, xs, qp, qn, addend = (_rows(c[name]) for name in ("r", "xs", "qp", "qn", "addend"))
        out = _nans(n, h * w, n_oc)
        ops.conv_geom_ab(r, _pack(ops, b6)(c["rows"][:kr].cuda(), _lib.GEOM_BWD), *args, xs, qp, scale=ALPHA, map2img=m2i, n_img=c["n_img"],
                         out=out, b6=b6)
        worst.check(out, "ab_single", c, None)
        out = _nans(n, h * w, n_oc)
        ops.conv_geom_ab(r, _pack(ops, b6)(c["rows"].cuda(), _lib.GEOM_BWD), *args, xs, qp, q2=qn, scale=ALPHA, scale2=-BETA, addend=addend,
                         map2img=m2i, n_img=c["n_img"], out=out, b6=b6)
        worst.check(out, "ab_dual", c, c["addend"])
    worst.report()


@MODES
@ALL_GEOMS
def test_transposed_grad(gid, b6):
    """lrpx_conv_geom_grad / _grad_b6 with mask, scale, addend and clamp, and with none of them"""
    _lib, ops = _mods()
    worst = Worst(f"gradient {gid} {'b6' if b6 else 'fp32'}")
    for k, n_oc in CHANNELS:
        c = case(gid, k, n_oc)
        (h, w), n = c["hw"], c["n"]
        args = (n, c["hw"], c["ohw"], c["geom"], k, n_oc)
        g, pack = _rows(c["r"]), _pack(ops, b6)(c["w"].cuda(), _lib.GEOM_BWD)
        out = _nans(n, h * w, n_oc)
        ops.conv_geom_grad(g, pack, *args, mask=_rows(c["mask"]), scale=c["scale"].cuda(), clamp=True, addend=_rows(c["addend"]),
                           map2img=_i32(c["m2i"]), n_img=c["n_img"], out=out, b6=b6)
        worst.check(out, "grad_full", c, c["addend"])
        out = _nans(n, h * w, n_oc)
        ops.conv_geom_grad(g, pack, *args, out=out, b6=b6)
        worst.check(out, "grad_none", c, None)
    worst.report()


# ---- 3. sentinel bands -----------------------------------------------------------------------------------------------------------------------
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


def _at_end(t):
    """the tensor at the END of a NaN-filled allocation: a read beyond it leaves the allocation or poisons the result"""
    buf = torch.full((GUARD + t.numel(),), float("nan"), device="cuda")
    view = buf[GUARD:].view(t.shape)
    view.copy_(t)
    return view


@ALL_GEOMS
def test_never_writes_past_its_output(gid):
    """both directions, both arithmetics, into a buffer with a sentinel band on either side, at 36 -> 40 channels (no multiple of a
    tile); the operands sit at the end of their allocations.  Every element of the output is written, the bands stay."""
    _lib, ops = _mods()
    c = case(gid, 36, 40)
    (h, w), (oh, ow), n, k, n_oc = c["hw"], c["ohw"], c["n"], 36, 40
    for b6 in (False, True):
        out = Guarded(n, oh * ow, n_oc)
        ops.conv_geom_ex(_at_end(_rows(c["xin"])), _pack(ops, b6)(c["wf"].cuda(), _lib.GEOM_FWD), _lib.GEOM_FWD, n, (h, w), (oh, ow), c["geom"],
                         k, n_oc, bias=c["bias"].cuda(), out=out.view, b6=b6)
        out.check(f"conv_geom_ex FWD {gid} b6={b6}")
        out = Guarded(n, h * w, n_oc)
        ops.conv_geom_ex(_at_end(_rows(c["r"])), _pack(ops, b6)(c["w"].cuda(), _lib.GEOM_BWD), _lib.GEOM_BWD, n, (h, w), (oh, ow), c["geom"],
                         k, n_oc, x=_at_end(_rows(c["x"])), q=_at_end(_rows(c["q"])), addend=_at_end(_rows(c["addend"])),
                         map2img=_i32(c["m2i"]), n_img=c["n_img"], out=out.view, b6=b6)
        out.check(f"conv_geom_ex BWD {gid} b6={b6}")
        assert rel_err(_nchw(out.view, (h, w)), reference("ex", c, torch.float64)) <= C * max(
            rel_err(reference("ex", c, torch.float32), reference("ex", c, torch.float64)), FLOOR)


# ---- 4. the packers, round-tripped -----------------------------------------------------------------------------------------------------------
@MODES
@ALL_GEOMS
def test_packers_round_trip(gid, b6):
    """at the geometry's kernel and stride on a map of exactly one window (H = kh, W = kw, no padding: OH = OW = 1) a one-hot operand
    selects one weight per output element: 1 * w and zeros are exact in both arithmetics (the three bf16 planes of w sum to w in any
    order).  Forward pack: image t K + c holds a one at pixel t, channel c, and returns column (c, t) of every filter.  Transposed pack:
    map co holds a one in channel co of the single source pixel and returns filter co, every tap in its own class."""
    _lib, ops = _mods()
    kh, kw, sh, sw, _, _ = GEOMS[gid][0]
    geom, taps = (kh, kw, sh, sw, 0, 0), kh * kw
    gen = torch.Generator().manual_seed(4200 + list(GEOMS).index(gid))
    for k in (4, 36):
        eye_f = torch.eye(taps * k, device="cuda").view(taps * k, taps, k)
        eye_b = torch.eye(k, device="cuda").view(k, 1, k)
        for n_oc in (3, 40, 72):
            wt = torch.randn(n_oc, k, kh, kw, generator=gen)
            out = _nans(taps * k, 1, n_oc)
            ops.conv_geom_ex(eye_f, _pack(ops, b6)(wt.cuda(), _lib.GEOM_FWD), _lib.GEOM_FWD, taps * k, (kh, kw), (1, 1), geom, k, n_oc, out=out,
                             b6=b6)
            assert torch.equal(out.cpu().view(taps * k, n_oc), wt.permute(2, 3, 1, 0).reshape(taps * k, n_oc)), \
                f"forward pack {gid} K {k} n_oc {n_oc} b6={b6}: a weight did not come back exactly"
            wt = torch.randn(k, n_oc, kh, kw, generator=gen)
            out = _nans(k, taps, n_oc)
            ops.conv_geom_ex(eye_b, _pack(ops, b6)(wt.cuda(), _lib.GEOM_BWD), _lib.GEOM_BWD, k, (kh, kw), (1, 1), geom, k, n_oc,
                             x=torch.ones(k, taps, n_oc, device="cuda"), out=out, b6=b6)
            assert torch.equal(out.cpu(), wt.permute(0, 2, 3, 1).reshape(k, taps, n_oc)), \
                f"transposed pack {gid} K {k} n_oc {n_oc} b6={b6}: a weight did not come back exactly"
