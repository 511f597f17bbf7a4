"""Host side of the gradient family of the single-LSTM adaptive-attention model (explainers/adaatt_grad.py, csrc/lrpx_adaatt_grad.hip;
DESIGN.md 5.16): the new symbols are declared, bound and exported under a prefix of their own; every new C entry refuses null pointers
and bad sizes with EINVAL before any launch and names itself; the fixture meets the conditions its generator
(tests/golden/make_golden_adaatt_grad.py) searched for; the five names are exported.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lrp_amd  # noqa: F401
from conftest import GOLDEN
from lrp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("lrpx_adaptive_grad_init", "lrpx_adaptive_grad_steps", "lrpx_adaptive_grad_pix_rows")
FIXTURES = ("adaatt_grad.npz", "adaatt_grad_maps.npz", "adaatt_grad_guided_maps.npz")


@pytest.fixture(scope="module")
def g():
    with np.load(os.path.join(GOLDEN, "adaatt_grad.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def test_symbols_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lrpx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lrpx_adaptive_[a-z0-9_]+)\s*\(", src))
    assert declared == set(ENTRIES)
    assert re.search(r"\}\s*lrpx_adaptive_gradstate\s*;", src)
    assert not [n for n in list(ENTRIES) + ["lrpx_adaptive_gradstate"] if n.startswith("lrpx_adaatt_")]
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), "%s is declared in include/lrpx.h but not exported" % name
        assert _lib.SIGNATURES[name][1][0]._type_ is _lib.AdaTrace and _lib.SIGNATURES[name][1][1]._type_ is _lib.AdaGradState
    # the ctypes structure follows the header's field order
    body = re.search(r"typedef struct lrpx_adaptive_gradstate \{(.*?)\}", src, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.AdaGradState._fields_], names


def test_exports_and_class_tree():
    from lrp_amd import explainers
    from lrp_amd.explainers import adaatt, adaatt_grad
    for name in ("AdaAttGradEngine", "ExplainAdaptiveGradient", "ExplainiAdaptiveGuidedGradient", "ExplainAdaptiveGradCam",
                 "ExplainAdaptiveGuidedGradCam"):
        assert getattr(explainers, name) is getattr(adaatt_grad, name), name
    assert issubclass(adaatt_grad.AdaAttGradEngine, adaatt.AdaAttEngine)
    for cls in (adaatt_grad.ExplainiAdaptiveGuidedGradient, adaatt_grad.ExplainAdaptiveGradCam, adaatt_grad.ExplainAdaptiveGuidedGradCam):
        assert issubclass(cls, adaatt_grad.ExplainAdaptiveGradient) and cls._RUNNING_SUMS is False
    assert issubclass(adaatt_grad.ExplainAdaptiveGradient, adaatt.ExplainAdaptiveAttention)
    assert [c.EX_TYPE for c in (adaatt_grad.ExplainAdaptiveGradient, adaatt_grad.ExplainiAdaptiveGuidedGradient, adaatt_grad.ExplainAdaptiveGradCam,
                                adaatt_grad.ExplainAdaptiveGuidedGradCam)] == ['gradient', 'GuidedBackpropagate', 'GradCam', 'GuidedGradCam']
    # the engine-cache key is the family's own
    import types

    import torch
    ex = adaatt_grad.ExplainAdaptiveGradient.__new__(adaatt_grad.ExplainAdaptiveGradient)
    ex.args, ex.model = types.SimpleNamespace(weight="w.pth"), {"fc.weight": torch.ones(2, 2)}
    lrp = adaatt.ExplainAdaptiveAttention.__new__(adaatt.ExplainAdaptiveAttention)
    lrp.args, lrp.model = ex.args, ex.model
    assert ex._engine_key() is not None and ex._engine_key()[0] == "adaatt_grad" != lrp._engine_key()[0]
    assert ex._engine_key()[1:] == lrp._engine_key()[1:]
    with pytest.raises(NotImplementedError, match="factor of 32"):          # before anything is loaded
        adaatt_grad.ExplainAdaptiveGuidedGradCam(ex.args, {"<start>": 0})
    # the base engine keeps refusing (tests/test_gpu_adaatt.py pins that on the GPU): the entries live in the subclass
    for name in ("trace", "guided_gradient", "explain_batch_guided", "explain_batch_gradient"):
        assert name in vars(adaatt_grad.AdaAttGradEngine) and name in vars(adaatt.AdaAttEngine), name
    assert "explain_features_gradient" in vars(adaatt_grad.AdaAttGradEngine)


def _trace(**kw):
    """a gradient trace whose pointers are non-null dummies (never dereferenced: every call below is refused on the host)"""
    t = _lib.AdaTrace()
    t.B, t.T, t.H, t.E, t.P = 2, 3, 512, 512, 12
    for name, _ in _lib.AdaTrace._fields_[5:]:
        setattr(t, name, 64)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _state(**kw):
    r = _lib.AdaGradState()
    for name, _ in _lib.AdaGradState._fields_[1:]:
        setattr(r, name, 64)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_every_entry_refuses_null_pointers_and_bad_sizes():
    lib = _lib.load()
    P, p = C.byref, C.c_void_p(64)
    ok, oks = _trace(), _state()
    calls = {
        "lrpx_adaptive_grad_init": lambda tr, gs, a=p: lib.lrpx_adaptive_grad_init(tr and P(tr), gs and P(gs), a, p, 4, p, None),
        "lrpx_adaptive_grad_steps": lambda tr, gs, a=p: lib.lrpx_adaptive_grad_steps(tr and P(tr), gs and P(gs), 3, a, p, None),
        "lrpx_adaptive_grad_pix_rows": lambda tr, gs, a=p: lib.lrpx_adaptive_grad_pix_rows(tr and P(tr), gs and P(gs), a, p, p, 192, None, 6, None),
    }
    assert set(calls) == set(ENTRIES)

    def refused(rc, name):
        assert rc == _lib.EINVAL, name
        assert name.encode() in lib.lrpx_last_error_string(), (name, lib.lrpx_last_error_string())
    for name, call in calls.items():
        bad_traces = [_trace(H=256), _trace(E=256), _trace(E=528), _trace(T=0), _trace(T=-1), _trace(P=0), _trace(P=300), _trace(B=0)]
        bad_traces += [_trace(**{k: None}) for k, _ in _lib.AdaTrace._fields_[5:]]           # every member, `o` and `sgate` included
        for bad in bad_traces:
            refused(call(bad, oks), name)
        for k, _ in _lib.AdaGradState._fields_[1:]:
            refused(call(ok, _state(**{k: None})), name)
        refused(call(None, oks), name)
        refused(call(ok, None), name)
        refused(call(ok, oks, None), name)                                                     # a null argument
    assert b"not a gradient trace" in (calls["lrpx_adaptive_grad_init"](_trace(o=None), oks), lib.lrpx_last_error_string())[1]
    # sizes
    refused(lib.lrpx_adaptive_grad_init(P(ok), P(oks), p, p, 3, p, None), "lrpx_adaptive_grad_init")           # tok_ld < T + 1
    refused(lib.lrpx_adaptive_grad_init(P(ok), P(oks), p, None, 4, p, None), "lrpx_adaptive_grad_init")
    refused(lib.lrpx_adaptive_grad_init(P(ok), P(oks), p, p, 4, None, None), "lrpx_adaptive_grad_init")
    refused(lib.lrpx_adaptive_grad_steps(P(ok), P(oks), 4, p, p, None), "lrpx_adaptive_grad_steps")            # n_steps > T
    refused(lib.lrpx_adaptive_grad_steps(P(ok), P(oks), 0, p, p, None), "lrpx_adaptive_grad_steps")
    refused(lib.lrpx_adaptive_grad_steps(P(ok), P(oks), 3, p, None, None), "lrpx_adaptive_grad_steps")
    pix = lib.lrpx_adaptive_grad_pix_rows
    refused(pix(P(ok), P(oks), p, p, p, 192, None, 5, None), "lrpx_adaptive_grad_pix_rows")                    # no row list: n_rows must be B*T
    refused(pix(P(ok), P(oks), p, p, p, 192, p, 0, None), "lrpx_adaptive_grad_pix_rows")
    refused(pix(P(ok), P(oks), p, p, p, 192, p, 7, None), "lrpx_adaptive_grad_pix_rows")
    refused(pix(P(ok), P(oks), p, p, p, 190, None, 6, None), "lrpx_adaptive_grad_pix_rows")                    # C % 4
    refused(pix(P(ok), P(oks), p, None, p, 192, None, 6, None), "lrpx_adaptive_grad_pix_rows")
    refused(pix(P(ok), P(oks), p, p, None, 192, None, 6, None), "lrpx_adaptive_grad_pix_rows")


def test_fixture_meets_its_conditions(g):
    for k in ("small", "long", "vgg"):
        assert float(g[k + "_e32_d_feat"]) < 1e-5, k
        assert float(g[k + "_e32_r_words"]) < 3e-6, k
    assert g["vgg_cam"].shape == (3, 196) and float(g["vgg_cam"].max()) > 0 and float(g["vgg_cam"].min()) >= 0
    assert int(g["guided_equals_gradient"]) == 1
    assert g["small_d_feat"].shape == (2, 3, 12, 192) and g["long_d_feat"].shape == (3, 12, 192) and g["vgg_d_feat"].shape == (3, 196, 128)
    assert g["small_r_words"].shape == (2, 3, 3) and g["long_r_words"].shape == (3, 26) and g["vgg_r_words64"].shape == (3, 3)
    assert g["long_words"].tolist() == [23, 24, 25] and g["long_caption"].shape == (1, 27)
    for t in range(3):                                                   # normalised rows (:1016-1019), nothing behind word t
        assert abs(float(np.abs(g["vgg_r_words"][t]).max()) - 1.0) < 1e-6 and not g["vgg_r_words"][t, t + 1:].any()
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 1 << 20, name
    for name, kind in (("adaatt_grad_maps.npz", "gradient"), ("adaatt_grad_guided_maps.npz", "guided")):
        with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as f:
            assert int(f["seed"]) == int(g["seed"]) and f["vgg_%s_map_full_2" % kind].shape == (1, 3, 224, 224)
            assert all(f["vgg_%s_map_sub4_%d" % (kind, t)].shape == (1, 3, 56, 56) for t in range(3))
