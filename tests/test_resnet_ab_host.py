"""Host side of the general alpha-beta rule on the batched ResNet engine (no GPU):
  * the dual-coefficient formulation (tests/resnet_ab_cases.py) in fp64 against the reference's own fp64 results
    (tests/golden/resnet_ab.npz) on both fixtures and both (alpha, beta) pairs;
  * the new entry points of the C ABI and their host-side refusals;
  * a CPU emulation of the data path of `lrpx_conv_geom_ab_b6` - the bf16x3 pack image of the stacked rows, the dual-coefficient gather,
    the LDS image of the A tile and the MFMA fragments by the lane maps csrc/conv_geom_b6.hip documents - at a shape where the half
    boundary falls inside a 32-channel chunk;
  * the decision, on the CPU, that the tensors of the GPU kernel tests are fit for the fp32-grade criterion of tests/fp64_anchor.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from lrp_amd import _lib, ops
from lrp_amd.LRPtools import lrp_modules

from conftest import GOLDEN, rel_err
from fp64_anchor import C as BOUND_C, FLOOR, SIX, THREE, WITNESS_MARGIN, bf16_split3
from resnet_ab_cases import EDGE_CASES, PROD_CASES, ab_relevance, ab_trace, case, reference

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet import TINY, bottleneck_net  # noqa: E402
from make_golden_resnet_engine import ENGINE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lrpx_conv_geom_ab", "lrpx_conv_geom_ab_b6", "lrpx_resnet_coef_neg")


# ---- the formulation in fp64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["engine", "tiny"])
def test_dual_coefficient_formulation_reproduces_the_reference_in_fp64(fixture):
    AB = dict(np.load(os.path.join(GOLDEN, "resnet_ab.npz")))
    if fixture == "engine":
        G = dict(np.load(os.path.join(GOLDEN, "resnet_engine.npz")))
        cfg, x, targets, m2i = ENGINE, G["x"], G["targets"], list(G["map2img"])
    else:
        G = dict(np.load(os.path.join(GOLDEN, "resnet_tiny.npz")))
        t1, t2 = G["target1"], G["target2"]
        cfg, x, targets, m2i = TINY, G["x"], np.stack([t1[0], t2[0], t1[1], t2[1]]), list(AB["tiny_map2img"])
    net = bottleneck_net(np.random.RandomState(int(G["seed"])), lrp_modules.resAdd, cfg["base"], cfg["blocks"]).double()
    plan = ops.match_bottleneck_resnet(net)
    with torch.no_grad():
        tr = ab_trace(plan, torch.from_numpy(x).double())
        for alpha, beta in AB["pairs"]:
            want = AB["%s_a%g_b%g_r64" % (fixture, alpha, beta)]
            for m, img in enumerate(m2i):
                got = ab_relevance(plan, tr, torch.from_numpy(targets[m:m + 1]).double(), img, float(alpha), float(beta))[0]
                e = rel_err(got, want[m])
                print(f"dual-coefficient formulation {fixture} alpha {alpha:g} beta {beta:g} map {m} (image {img}): {e:.2e} of the map's maximum")
                assert e < 1e-9, (fixture, alpha, beta, m, e)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
def _lib_loaded():
    assert os.path.exists(_lib.LIB_PATH), "liblrpx.so not built (run __graft_entry__.build())"
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lrpx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lrpx_[a-z0-9_]+)\s*\(", src))
    lib = _lib_loaded()
    for s in NEW_SYMBOLS:
        assert s in declared, s + " is not declared in include/lrpx.h"
        assert s in _lib.SIGNATURES, s + " is not bound in _lib.py"
        assert hasattr(lib, s), s + " is not exported"
    assert "lrpx_conv_geom_ab_desc" in src
    assert lib.lrpx_version() == 101            # detected by presence, no new number


def _desc(**kw):
    """a consistent 3x3 s2 p1 dual descriptor on 8 x 8 -> 4 x 4, kr = 8, with made-up (aligned, never dereferenced) pointers"""
    f = dict(in_=0x10000, wpacked=0x20000, bias=None, x=0x30000, q=0x40000, addend=None, map2img=None, out=0x50000, dir=_lib.GEOM_BWD,
             n=1, n_img=1, h=8, w=8, oh=4, ow=4, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1, k=16, n_oc=8)
    ab = dict(q2=0x60000, scale=2., scale2=-1., kr=8)
    for k in list(kw):
        if k in ab:
            ab[k] = kw.pop(k)
    f.update(kw)
    return _lib.ConvGeomAbDesc(_lib.ConvGeomExDesc(**f), ab["q2"], ab["scale"], ab["scale2"], ab["kr"])


@pytest.mark.parametrize("entry", ["lrpx_conv_geom_ab", "lrpx_conv_geom_ab_b6"])
def test_new_entry_points_refuse_on_the_host(entry):
    lib = _lib_loaded()
    fn = getattr(lib, entry)

    def refused(d, word):
        assert fn(C.byref(d) if d is not None else None, None) == _lib.EINVAL
        msg = lib.lrpx_last_error_string()
        assert msg and entry.encode() in msg and word in msg, msg
    refused(None, b"null descriptor")
    refused(_lib.ConvGeomAbDesc(), b"null")
    refused(_desc(q2=None), b"q2")                                   # k = 2 kr without the second coefficient
    refused(_desc(q2=0x60004), b"aligned")
    refused(_desc(k=8), b"q2")                                       # the W+ half alone, with a second coefficient
    refused(_desc(kr=6, k=12), b"multiple of 4")
    refused(_desc(k=24), b"2 kr")
    refused(_desc(dir=_lib.GEOM_FWD), b"transposed direction only")
    refused(_desc(q=None), b"coefficient q")
    refused(_desc(bias=0x70000), b"bias")
    refused(_desc(oh=5), b"output 5x4")
    for bad in (float("nan"), float("inf")):
        refused(_desc(scale=bad), b"finite")
        refused(_desc(scale2=-bad), b"finite")
    refused(_desc(k=8, q2=None, scale2=-1.), b"scale2 zero")
    assert lib.lrpx_resnet_coef_neg(None, 8, None, None, None, 4, 4, None) == _lib.EINVAL
    assert b"null" in lib.lrpx_last_error_string()
    assert lib.lrpx_resnet_coef_neg(0x10000, 6, 0x20000, 0x30000, 0x40000, 4, 4, None) == _lib.EINVAL      # ld < 2 c
    assert b"bad sizes" in lib.lrpx_last_error_string()


def test_engine_checks_alpha_beta_before_it_touches_the_trace():
    eng = ops.ResNetEncoder.__new__(ops.ResNetEncoder)             # no device: the method must refuse before it reads any state
    for bad in ((float("nan"), 1.), (2., float("inf"))):
        with pytest.raises(ValueError, match="finite"):
            eng.relevance_alpha_beta(None, alpha=bad[0], beta=bad[1])


# ---- the data path of lrpx_conv_geom_ab_b6, emulated -------------------------------------------------------------------------------------
def _planes(t):
    """fp32 tensor -> (3, ...) fp64 array of its exact bf16 planes (the kernels' split3)"""
    return np.stack([p.double().numpy() for p in bf16_split3(t)])


def test_b6_dual_gather_data_path_emulation():
    """1x1, kr = 52 (K = 104: the half boundary at channel 52 lies inside chunk 1, chunk 3 holds 8 channels), n_oc = 40 (the second
    column block a quarter full), 70 pixels (a full tile and one of 6 rows), one map.  Written out as the kernel does it: the pack
    image by conv_geom_pack_bf16x3_kernel's index arithmetic on the rows [W+ ; W-]; per stage every thread's two float4 gathers with the
    half select, (R q) s in fp32, split3, the three 8-byte LDS stores; the fragments by the documented lane maps (A: row l & 31,
    k = 8 (l >> 5) + j of a k-step; B: one 16-byte slot per lane; accumulator e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column
    l & 31).  Every LDS slot a fragment reads must have been written in that stage, and - summing ALL plane products in fp64, which
    makes the operands exact - the result must be the fp64 product."""
    kr, n_oc, npix, alpha, beta = 52, 40, 70, 2., 1.
    K, ROW, FRAG = 2 * kr, 104, 3072                              # ROW: bf16 slots per LDS row (208 B); FRAG: bf16 per (ocb, tap, chunk)
    nchunk, n_ocb = -(-K // 32), -(-n_oc // 32)
    g = torch.Generator().manual_seed(52)
    wt = torch.randn(kr, n_oc, generator=g)
    rows = torch.cat([wt.clamp(min=0), wt.clamp(max=0)], 0)        # (K, n_oc): W[k][col] of the transposed direction
    r, qp = torch.randn(npix, kr, generator=g), torch.rand(npix, kr, generator=g) + 0.5
    qn = -(torch.rand(npix, kr, generator=g) + 0.5)
    x = torch.rand(npix, n_oc, generator=g)

    # the pack image: element idx -> (j, lane, ks, frag = (ocb, tap, chunk)), three planes 512 slots apart
    total = n_ocb * nchunk * 1024
    packed = np.full((total * 3,), np.nan)
    rows_pl = _planes(rows)
    for idx in range(total):
        j, lane, ks, frag = idx & 7, (idx >> 3) & 63, (idx >> 9) & 1, idx >> 10
        chunk, ocb = frag % nchunk, frag // nchunk
        k, col = chunk * 32 + 16 * ks + 8 * (lane >> 5) + j, ocb * 32 + (lane & 31)
        v = rows_pl[:, k, col] if (k < K and col < n_oc) else np.zeros(3)
        dst = ((frag * 2 + ks) * 3) * 512 + lane * 8 + j
        packed[[dst, dst + 512, dst + 1024]] = v
    assert not np.isnan(packed).any(), "the packer leaves part of the image unwritten"

    got = np.full((npix, n_oc), np.nan)
    f32 = lambda t: t.to(torch.float32)
    for blk in range(-(-npix // 64)):
        pix0 = blk * 64
        acc = np.zeros((4, 64, 16))                                 # [wave][lane][register]
        for chunk in range(nchunk):                                 # one tap: a stage per chunk
            lds = np.full((64, ROW), np.nan)
            for tid in range(256):
                c4 = 4 * (tid & 7)
                kc = chunk * 32 + c4
                for u in range(2):
                    row = (tid >> 3) + 32 * u
                    v = torch.zeros(4)
                    if pix0 + row < npix and kc < K:
                        neg = kc >= kr
                        c = kc - kr if neg else kc
                        v = f32(f32(r[pix0 + row, c:c + 4] * (qn if neg else qp)[pix0 + row, c:c + 4]) * (-beta if neg else alpha))
                    a_dst = ((c4 >> 4) * 96 + (c4 & 15) * 2) // 2   # in bf16 slots
                    pl = _planes(v)
                    for p in range(3):
                        lds[row, a_dst + 16 * p: a_dst + 16 * p + 4] = pl[p]
            for wave in range(4):
                wm, wn = wave & 1, wave >> 1
                if wn * 32 >= n_oc:
                    continue
                for lane in range(64):                              # what each lane's twelve 16-byte fragment reads touch
                    for ks in range(2):
                        a = np.stack([lds[wm * 32 + (lane & 31), (16 * (lane >> 5) + ks * 96 + 32 * p) // 2:][:8] for p in range(3)])
                        assert not np.isnan(a).any(), f"stage {chunk}: lane {lane} of wave {wave} reads an unwritten LDS slot"
                # the MFMAs of the stage: per k-step and k group (l >> 5), rows of lanes 0..31 against the columns of lanes 0..31
                for ks in range(2):
                    for kg in range(2):
                        A = np.stack([np.stack([lds[wm * 32 + rl, (16 * kg + ks * 96 + 32 * p) // 2:][:8] for p in range(3)]).sum(0)
                                      for rl in range(32)])                                   # (32 rows, 8 k)
                        B = np.stack([np.stack([packed[((wn * nchunk + chunk) * 2 + ks) * 1536 + 512 * p + (32 * kg + cl) * 8:][:8]
                                                for p in range(3)]).sum(0) for cl in range(32)])   # (32 columns, 8 k)
                        prod = A @ B.T                                                        # (row, column)
                        for lane in range(64):
                            for e in range(16):
                                acc[wave, lane, e] += prod[(e & 3) + 8 * (e >> 2) + 4 * (lane >> 5), lane & 31]
        for wave in range(4):
            wm, wn = wave & 1, wave >> 1
            for lane in range(64):
                oc = wn * 32 + (lane & 31)
                if oc >= n_oc:
                    continue
                for e in range(16):
                    q = pix0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
                    if q < npix:
                        assert np.isnan(got[q, oc]), "an output written twice"
                        got[q, oc] = acc[wave, lane, e] * x[q, oc].item()
    assert not np.isnan(got).any(), "part of the output is never written"
    a32 = torch.cat([(r * qp) * alpha, (r * qn) * (-beta)], 1)      # the operand as the kernel forms it, in fp32
    want = (a32.double() @ rows.double()).numpy() * x.double().numpy()
    e = np.abs(got - want).max() / np.abs(want).max()
    print(f"b6 dual gather data path, 1x1 kr 52 n_oc 40, 70 pixels: {e:.2e} of the maximum against the fp64 product")
    assert e < 1e-13, e


# ---- the GPU tests' tensors are fit for the fp32-grade bound ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in EDGE_CASES + PROD_CASES])
def test_the_kernel_test_inputs_are_fit_for_the_fp32_grade_bound(name):
    """on the GPU test's own tensors, with and without the addend as it runs them: the six products of conv mode 1 pass
    e <= C max(e32, FLOOR) although W+ and W- cancel, the three-product witness misses it by WITNESS_MARGIN"""
    c = case(name)
    for addend in (True, False):
        ref64, ref32 = reference(c, torch.float64, addend=addend), reference(c, torch.float32, addend=addend)
        six, three = reference(c, torch.float64, SIX, addend=addend), reference(c, torch.float64, THREE, addend=addend)
        e32, e6, e3 = rel_err(ref32, ref64), rel_err(six, ref64), rel_err(three, ref64)
        bound = BOUND_C * max(e32, FLOOR)
        print(f"alpha-beta kernel inputs {name} addend {addend}: e32 {e32:.2e}  six-product emulation {e6:.2e}  bound {bound:.2e}  "
              f"three-product witness {e3:.2e} = {e3 / bound:.1f}x the bound")
        assert e6 <= bound, (name, e6, bound)
        assert e3 / bound >= WITNESS_MARGIN, (name, e3 / bound)
