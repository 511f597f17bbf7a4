"""Host side of the ResNet engine's conv mode 1 (csrc/conv_geom_b6.hip; no GPU): the size of the bf16x3 image, the
refusals of the new entry points, the engine's mode check - and the decision, on the CPU, that the tensors of the GPU parity test
(tests/resnet_b6_cases.py) are fit for the fp32-grade criterion of tests/fp64_anchor.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from lrp_amd import _lib, ops
from lrp_amd.LRPtools import lrp_modules

from conftest import GOLDEN, rel_err
from fp64_anchor import C as BOUND_C, FLOOR, SIX, THREE, WITNESS_MARGIN
from resnet_b6_cases import BWD_CASES, bwd_case, bwd_reference

import sys
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet import bottleneck_net  # noqa: E402


def _lib_loaded():
    assert os.path.exists(_lib.LIB_PATH), "liblrpx.so not built (run __graft_entry__.build())"
    return _lib.load()


@pytest.mark.parametrize("n_oc,k,taps,want", [(64, 64, 9, 2 * 9 * 2 * 6144), (6, 20, 1, 6144), (8, 64, 49, 49 * 2 * 6144)])
def test_packed_bf16x3_bytes(n_oc, k, taps, want):
    """ceil(n_oc / 32) * taps * ceil(k / 32) * 2 k-steps * 3 planes * 1024: ragged channel counts pad to 32"""
    lib = _lib_loaded()
    assert lib.lrpx_conv_geom_packed_bf16x3_bytes(n_oc, k, taps) == want
    assert want == -(-n_oc // 32) * taps * -(-k // 32) * 2 * 3 * 1024
    assert lib.lrpx_conv_geom_packed_bf16x3_bytes(0, k, taps) == 0


def _desc(**kw):
    """a consistent 3x3 s2 p1 descriptor on 8 x 8 -> 4 x 4 with made-up (aligned, never dereferenced) pointers"""
    f = dict(in_=0x10000, wpacked=0x20000, bias=None, x=0x30000, q=0x40000, addend=None, map2img=None, out=0x50000, dir=_lib.GEOM_BWD,
             n=1, n_img=1, h=8, w=8, oh=4, ow=4, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1, k=8, n_oc=8)
    f.update(kw)
    return _lib.ConvGeomExDesc(**f)


def _refused(rc, lib, word):
    assert rc == _lib.EINVAL
    msg = lib.lrpx_last_error_string()
    assert msg and word in msg, msg


def test_new_entry_points_refuse_on_the_host():
    lib = _lib_loaded()
    ex = lambda d: lib.lrpx_conv_geom_ex_b6(C.byref(d), None)
    _refused(lib.lrpx_conv_geom_ex_b6(None, None), lib, b"null descriptor")
    _refused(ex(_lib.ConvGeomExDesc()), lib, b"null")
    _refused(ex(_desc(k=6)), lib, b"multiple of 4")
    _refused(ex(_desc(in_=0x10004)), lib, b"aligned")
    _refused(ex(_desc(bias=0x60000)), lib, b"bias")
    _refused(ex(_desc(oh=5)), lib, b"output 5x4")
    _refused(ex(_desc(dir=_lib.GEOM_FWD)), lib, b"transposed direction")          # x / q given to the forward direction
    _refused(lib.lrpx_conv_geom_pack_bf16x3(None, 8, 8, 3, 3, _lib.GEOM_BWD, None, None), lib, b"null")
    _refused(lib.lrpx_conv_geom_pack_bf16x3(0x10000, 8, 0, 3, 3, _lib.GEOM_BWD, 0x20000, None), lib, b"bad shape")
    _refused(lib.lrpx_conv_geom_pack_bf16x3(0x10000, 8, 8, 3, 3, 2, 0x20000, None), lib, b"direction")


def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib_loaded()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lrpx.h")).read()
    for s in ("lrpx_conv_geom_packed_bf16x3_bytes", "lrpx_conv_geom_pack_bf16x3", "lrpx_conv_geom_ex_b6"):
        assert s + "(" in hdr and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.lrpx_version() == 101            # detected by presence, no new number


def test_encoder_names_its_modes_before_it_asks_for_a_gpu():
    net = bottleneck_net(np.random.RandomState(3), lrp_modules.resAdd, 8, [2, 1])     # on the CPU
    for bad in (2, 3, -1, "1", True):
        with pytest.raises(ValueError, match="modes 0 .* and 1"):
            ops.ResNetEncoder(net, conv_mode=bad)
    with pytest.raises(ValueError, match="GPU"):
        ops.ResNetEncoder(net, conv_mode=1)                                           # a mode it has: the residency check speaks


@pytest.mark.parametrize("name", [c[0] for c in BWD_CASES])
def test_the_parity_inputs_are_fit_for_the_fp32_grade_bound(name):
    """x * convT(r * q, W+) + addend on the GPU test's own tensors in fp64, in fp32 and from the plane products: the six products
    of conv mode 1 pass e <= C max(e32, FLOOR), the three-product witness misses it by WITNESS_MARGIN"""
    c = bwd_case(name)
    ref64, ref32 = bwd_reference(c, torch.float64), bwd_reference(c, torch.float32)
    six, three = bwd_reference(c, torch.float64, SIX), bwd_reference(c, torch.float64, THREE)
    e32, e6, e3 = rel_err(ref32, ref64), rel_err(six, ref64), rel_err(three, ref64)
    bound = BOUND_C * max(e32, FLOOR)
    print(f"b6 parity inputs {name}: e32 {e32:.2e}  six-product emulation {e6:.2e}  bound {bound:.2e}  "
          f"three-product witness {e3:.2e} = {e3 / bound:.1f}x the bound")
    assert e6 <= bound, (name, e6, bound)
    assert e3 / bound >= WITNESS_MARGIN, (name, e3 / bound)
