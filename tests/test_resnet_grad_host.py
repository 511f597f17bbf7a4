"""Host-side checks of the ResNet encoder engine's gradient chain (no GPU): the new entry points of the C ABI are
declared, bound and exported; every refusal of lrpx_conv_geom_grad / _grad_b6 / lrpx_resnet_relu_grad / lrpx_resnet_maxpool_grad is
reached through the C entry before anything touches a device; ops refuses a bad `relus`, wrong shapes and a missing trace; and the
stored fixtures meet the conditioning they were searched for (margins >= 1e-5, the reference's fp32 within 1e-5 of its fp64)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from lrp_amd import _lib, ops

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lrpx_conv_geom_grad", "lrpx_conv_geom_grad_b6", "lrpx_resnet_relu_grad", "lrpx_resnet_maxpool_grad")
FAKE = 0x1000            # a non-null, 16-byte aligned address: every refusal below comes before the first dereference


def _lib_loaded():
    assert os.path.exists(_lib.LIB_PATH), "liblrpx.so not built (run __graft_entry__.build())"
    return _lib.load()


def _desc(**kw):
    """a descriptor lrpx_conv_geom_grad would accept (3x3 s2 p1, 11x13 -> 6x7, 3 maps on 2 images), then `kw` over it"""
    base = dict(in_=FAKE, wpacked=FAKE, bias=None, x=None, q=None, addend=None, map2img=FAKE, out=FAKE, dir=_lib.GEOM_BWD, n=3, n_img=2,
                h=11, w=13, oh=6, ow=7, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1, k=12, n_oc=40)
    top = dict(mask=FAKE, scale=FAKE, clamp=0)
    for key, v in kw.items():
        (top if key in top else base)[key] = v
    return _lib.ConvGeomGradDesc(_lib.ConvGeomExDesc(**base), top["mask"], top["scale"], top["clamp"])


def test_new_symbols_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lrpx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lrpx_[a-z0-9_]+)\s*\(", src))
    for s in NEW_SYMBOLS:
        assert s in declared, s + " is not declared in include/lrpx.h"
        assert s in _lib.SIGNATURES, s + " is not bound in _lib.py"
    assert "lrpx_conv_geom_grad_desc" in src
    lib = _lib_loaded()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    for name in ("conv_geom_grad", "conv_geom_grad_b6", "resnet_relu_grad", "resnet_maxpool_grad"):
        assert callable(getattr(ops, name))
    assert C.sizeof(_lib.ConvGeomGradDesc) == C.sizeof(_lib.ConvGeomExDesc) + 24


@pytest.mark.parametrize("entry", ["lrpx_conv_geom_grad", "lrpx_conv_geom_grad_b6"])
@pytest.mark.parametrize("kw,message", [
    (dict(dir=_lib.GEOM_FWD), "transposed direction only"),
    (dict(x=FAKE), "x, q and bias must be null"),
    (dict(q=FAKE), "x, q and bias must be null"),
    (dict(bias=FAKE), "x, q and bias must be null"),
    (dict(mask=FAKE + 4), "mask and scale must be 16-byte aligned"),
    (dict(scale=FAKE + 8), "mask and scale must be 16-byte aligned"),
    (dict(clamp=2), "clamp is 0 or 1"),
    (dict(clamp=-1), "clamp is 0 or 1"),
    # what lrpx_conv_geom_ex refuses, in its words
    (dict(in_=None), "null pointer"),
    (dict(dir=7), "unknown direction 7"),
    (dict(n=0), "bad sizes"),
    (dict(n_img=0), "the transposed direction needs n_img > 0"),
    (dict(map2img=None), "without map2img there is one map per image"),
    (dict(kh=0), "bad window"),
    (dict(oh=5), "is not what input 11x13 gives"),
    (dict(k=10), "must be a multiple of 4"),
    (dict(in_=FAKE + 4), "16-byte aligned"),
], ids=lambda v: v if isinstance(v, str) else "-".join("%s=%s" % kv for kv in v.items()))
def test_conv_geom_grad_refusals(entry, kw, message):
    lib = _lib_loaded()
    assert getattr(lib, entry)(C.byref(_desc(**kw)), None) == _lib.EINVAL
    text = lib.lrpx_last_error_string().decode()
    assert message in text and entry in text, text


def test_null_descriptors_and_elementwise_refusals():
    lib = _lib_loaded()
    for entry in ("lrpx_conv_geom_grad", "lrpx_conv_geom_grad_b6"):
        assert getattr(lib, entry)(None, None) == _lib.EINVAL
        assert b"null descriptor" in lib.lrpx_last_error_string()
        assert getattr(lib, entry)(C.byref(_lib.ConvGeomGradDesc()), None) == _lib.EINVAL
    relu = lambda g=FAKE, n_maps=3, n_img=2, per=8, m2i=FAKE, clamp=0: lib.lrpx_resnet_relu_grad(g, FAKE, m2i, FAKE, n_maps, n_img, per, clamp, None)
    for call, message in ((lambda: relu(g=None), "null pointer"), (lambda: relu(n_maps=0), "bad sizes"), (lambda: relu(per=0), "bad sizes"),
                          (lambda: relu(m2i=None), "without map2img"), (lambda: relu(clamp=2), "clamp is 0 or 1")):
        assert call() == _lib.EINVAL
        assert message in lib.lrpx_last_error_string().decode()
    pool = lambda x=FAKE, n_maps=3, n_img=2, m2i=FAKE, oh=6, kh=3, c=4: lib.lrpx_resnet_maxpool_grad(x, FAKE, m2i, FAKE, n_maps, n_img, 11, 13, oh, 7, c,
                                                                                                   kh, 3, 2, 2, 1, 1, None)
    for call, message in ((lambda: pool(x=None), "null pointer"), (lambda: pool(c=0), "bad sizes or window"), (lambda: pool(kh=0), "bad sizes or window"),
                          (lambda: pool(oh=8), "bad sizes or window"), (lambda: pool(m2i=None), "without map2img")):
        assert call() == _lib.EINVAL
        assert "resnet_maxpool_grad" in lib.lrpx_last_error_string().decode() and message in lib.lrpx_last_error_string().decode()


def _engine_stub(trace):
    """the members ResNetEncoder's argument checks read, without a device: feature map 5 x 5 x 64 of 2 images of 38 x 34"""
    e = object.__new__(ops.ResNetEncoder)
    e.trace, e.n_img, e.dims, e.shape, e.cin, e.feat_hw = trace, 2, None, (2, 38, 34), 3, (5, 5)
    e.packs, e.plan = [dict(cout=64)], types.SimpleNamespace(blocks=[dict(conv3=0)])
    return e


def test_ops_refuses_bad_arguments_on_the_host():
    g = torch.zeros(2, 25, 64)
    with pytest.raises(ValueError, match="relus must be 'stem' or 'all'"):
        _engine_stub({}).guided_backprop(g, relus="every")
    with pytest.raises(ValueError, match="relus"):
        _engine_stub(None).guided_backprop(g, relus=None)
    for fn in ("gradient", "guided_backprop"):
        with pytest.raises(ValueError, match=fn + ": no trace"):
            getattr(_engine_stub(None), fn)(g)
        with pytest.raises(ValueError, match="no CPU path"):
            getattr(_engine_stub({}), fn)(g)
    # the wrapper's shape checks come before any device work
    args = (torch.zeros(3, 42, 12), torch.zeros(1), 3, (11, 13), (6, 7), (3, 3, 2, 2, 1, 1), 12, 40)
    with pytest.raises(ValueError, match="mask must be"):
        ops.conv_geom_grad(*args, mask=torch.zeros(3, 42, 12), n_img=2)
    with pytest.raises(ValueError, match="scale must be"):
        ops.conv_geom_grad(*args, scale=torch.zeros(40), n_img=2)
    with pytest.raises(ValueError, match="addend must have"):
        ops.conv_geom_grad(*args, addend=torch.zeros(3, 42, 40), n_img=2)
    with pytest.raises(ValueError, match="the input must hold"):
        ops.conv_geom_grad(torch.zeros(3, 41, 12), *args[1:], n_img=2)


def test_stored_fixtures_meet_their_conditioning():
    G = dict(np.load(os.path.join(GOLDEN, "resnet_grad.npz")))
    for net in ("tiny", "engine"):
        print(f"resnet_grad.npz {net}: seed {int(G[net + '_seed'])}  relu margin {float(G[net + '_relu_margin']):.2e}  "
              f"pool margin {float(G[net + '_pool_margin']):.2e}  e32 {float(G[net + '_e32']):.2e}")
        assert G[net + "_relu_margin"] >= 1e-5 and G[net + "_pool_margin"] >= 1e-5
        assert G[net + "_e32"] < 1e-5 and G[net + "_e32_rows"].max() == G[net + "_e32"]
        # the three passes are three different maps: the hooks of the reference's path did fire, and only at the stem
        p, s, a = G[net + "_plain64"], G[net + "_stem64"], G[net + "_all64"]
        scale = np.abs(p).max()
        assert np.abs(p - s).max() > 0.1 * scale and np.abs(s - a).max() > 0.1 * np.abs(s).max()
    D = dict(np.load(os.path.join(GOLDEN, "gridtd_resnet_grad.npz")))
    e32 = {k[4:]: float(v) for k, v in D.items() if k.startswith("e32_")}
    print(f"gridtd_resnet_grad.npz: relu margin {float(D['relu_margin']):.2e}  pool margin {float(D['pool_margin']):.2e}  e32 {e32}")
    assert D["relu_margin"] >= 1e-5 and D["pool_margin"] >= 1e-5
    assert len(e32) == 7 and max(e32.values()) < 1e-5
    assert int(D["net_seed"]) == int(G["engine_seed"])                 # the net and images whose margins resnet_grad.npz stores
