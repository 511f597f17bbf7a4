"""Host-side logic of LRP through the bottleneck ResNet encoders (no GPU): the geometries the Conv2d rule accepts, what `add_lrp`
accepts and still refuses, the new entry points of the C ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch.nn as nn

import lrp_amd  # noqa: F401
from lrp_amd import _lib
from lrp_amd.LRPtools import lrp_modules, lrp_wrapper

from conftest import GOLDEN

NEW_SYMBOLS = ("lrpx_conv_geom", "lrpx_conv_geom_pack", "lrpx_conv_geom_packed_floats", "lrpx_maxpool_rule")


def _bottleneck_net(**kw):
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    from make_golden_resnet import bottleneck_net
    return bottleneck_net(np.random.RandomState(3), lrp_modules.resAdd, **kw)


def test_conv_geometry_accepts_the_resnet_geometries():
    cases = {(7, 7, 2, 2, 3, 3): nn.Conv2d(3, 8, 7, stride=2, padding=3), (1, 1, 1, 1, 0, 0): nn.Conv2d(8, 8, 1),
             (1, 1, 2, 2, 0, 0): nn.Conv2d(8, 8, 1, stride=2), (3, 3, 2, 2, 1, 1): nn.Conv2d(8, 8, 3, stride=2, padding=1),
             (3, 3, 1, 1, 1, 1): nn.Conv2d(8, 8, 3, padding=1), (1, 3, 1, 2, 0, 1): nn.Conv2d(8, 8, (1, 3), stride=(1, 2), padding=(0, 1))}
    for want, conv in cases.items():
        assert lrp_modules.conv_geometry(conv) == want


@pytest.mark.parametrize("conv", [nn.Conv2d(8, 8, 3, padding=2, dilation=2), nn.Conv2d(8, 8, 3, padding=1, groups=2),
                                  nn.Conv2d(8, 8, 3, padding=1, padding_mode="reflect"), nn.Conv2d(8, 8, 3, padding="same")],
                         ids=["dilation", "groups", "padding_mode", "string_padding"])
def test_conv_geometry_refuses_what_the_engine_does_not_run(conv):
    with pytest.raises(ValueError):
        lrp_modules.conv_geometry(conv)


def test_maxpool_rule_refuses_dilation():
    import torch
    pool = nn.MaxPool2d(3, 2, 1, dilation=2)
    pool.input = (torch.zeros(1, 1, 9, 9),)
    with pytest.raises(ValueError, match="dilation"):
        lrp_modules.Pool2d().propagate_relevance(pool, None, (torch.zeros(1, 1, 4, 4),), "alpha_beta", {})


def test_add_lrp_accepts_the_bottleneck_net_with_its_unused_head():
    """every leaf of the net has a rule or is the deferred AdaptiveAvgPool2d: the first refusal is the missing CPU path"""
    net = _bottleneck_net(base=8, blocks=[1, 1], head=True)
    assert any(isinstance(m, nn.AdaptiveAvgPool2d) for m in net.modules())
    with pytest.raises(_lib.LrpxError, match="no CPU path"):
        lrp_wrapper.add_lrp(net)


def test_unknown_leaves_are_still_refused_eagerly():
    with pytest.raises(ValueError, match="not known"):
        lrp_wrapper.add_lrp(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.Sigmoid()))
    with pytest.raises(ValueError, match="not known"):
        lrp_modules.get_lrp_module(nn.AdaptiveAvgPool2d(1))
    with pytest.raises(ValueError, match="not known"):
        lrp_wrapper.add_lrp(nn.Sequential(nn.Conv2d(3, 8, 1), nn.AdaptiveMaxPool2d(1)))


def test_pool_output_size_follows_aten():
    import torch
    for size, k, s, p, ceil_mode in [(9, 3, 2, 1, False), (8, 3, 2, 1, False), (8, 3, 2, 0, True), (7, 2, 2, 0, False), (7, 2, 2, 0, True),
                                     (6, 3, 1, 1, False), (5, 2, 3, 1, True), (112, 3, 2, 1, False)]:
        want = nn.MaxPool2d(k, s, p, ceil_mode=ceil_mode)(torch.zeros(1, 1, size, size)).shape[-1]
        assert lrp_modules._pool_out(size, k, s, p, ceil_mode) == want, (size, k, s, p, ceil_mode)


def test_new_symbols_are_bound_and_version_stays():
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("liblrpx.so not built")
    lib = _lib.load()
    assert lib.lrpx_version() == 101            # the capability is detected by the symbols, not by the number
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)


def test_new_entry_points_validate_on_the_host():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("liblrpx.so not built")
    lib = _lib.load()
    assert lib.lrpx_conv_geom(None, None) == _lib.EINVAL
    assert b"null" in lib.lrpx_last_error_string()
    d = _lib.ConvGeomDesc()
    assert lib.lrpx_conv_geom(C.byref(d), None) == _lib.EINVAL
    assert lib.lrpx_conv_geom_pack(None, 8, 8, 3, 3, _lib.GEOM_FWD, None, None) == _lib.EINVAL
    assert lib.lrpx_maxpool_rule(None, None, None, 1, 8, 8, 4, 4, 3, 3, 2, 2, 1, 1, None) == _lib.EINVAL
    assert b"null" in lib.lrpx_last_error_string()
    # packed size: 32-wide column blocks x taps x 32-channel chunks of 1024 floats
    assert lib.lrpx_conv_geom_packed_floats(64, 64, 9) == 2 * 9 * 2 * 1024
    assert lib.lrpx_conv_geom_packed_floats(6, 8, 49) == 1 * 49 * 1 * 1024
    assert lib.lrpx_conv_geom_packed_floats(0, 8, 1) == 0
