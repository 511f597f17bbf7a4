"""The public surface of the caption explainers is the one recorded in tests/golden/explainer_api.json (written by
tests/golden/make_golden_explainer_api.py from the commit named in the file, before the two engines and the two drop-in families were
put on shared bases): every public method of `GridTDEngine`, `AOAEngine` and the ten `Explain*` classes with its `inspect.signature`,
and every public class constant (`EPS`, `EX_TYPE`, `TF_MODEL_BIAS`, `NEEDS_ENCODER_GRADIENT`, ...) with its value.  Only what ADDED lists
may have appeared since.  Both engines derive from explainers/engine_base.py's base, both drop-in families from explainers/dropin.py's,
and the static-buffer drivers (HIP graph, recorded step, stream events) exist in the base alone."""
import json
import os
import sys

import lrp_amd  # noqa: F401
from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_explainer_api as G  # noqa: E402

# public names the recorded commit did not have: `grad_cam` moved to the engines' base (AOAEngine gains it)
ADDED = {"aoa.AOAEngine": {"grad_cam"}}


def _golden():
    with open(G.JSON) as f:
        return json.load(f)


def test_public_methods_and_constants_are_the_recorded_ones():
    want, got = _golden()["classes"], G.inventory()
    assert sorted(want) == sorted(got) and len(want) == 12
    for cls, w in want.items():
        for kind in ("methods", "constants"):
            for name, v in w[kind].items():
                assert name in got[cls][kind], "%s.%s is gone" % (cls, name)
                assert got[cls][kind][name] == v, "%s.%s: %r, recorded %r" % (cls, name, got[cls][kind][name], v)
        new = (set(got[cls]["methods"]) | set(got[cls]["constants"])) - set(w["methods"]) - set(w["constants"])
        assert new <= ADDED.get(cls, set()), "%s: new public names %s" % (cls, sorted(new))
    assert got["gridtd.ExplainGridTDAttention"]["constants"]["NEEDS_ENCODER_GRADIENT"] is False
    assert got["gridtd.ExplainiGridTDGuidedGradient"]["constants"]["NEEDS_ENCODER_GRADIENT"] is True


def test_engines_and_drop_ins_derive_from_the_shared_bases():
    from lrp_amd.explainers import aoa, dropin, engine_base, gridtd
    assert issubclass(gridtd.GridTDEngine, engine_base.EngineBase) and issubclass(aoa.AOAEngine, engine_base.EngineBase)
    assert issubclass(gridtd.ExplainGridTDAttention, dropin.ExplainerBase) and issubclass(aoa.ExplainAOAAttention, dropin.ExplainerBase)
    for name in ("replica", "sample_lrp", "forwardlrp_context", "beam_search", "grad_cam", "_f16", "_row_index"):      # one body each
        assert name in vars(engine_base.EngineBase) and name not in vars(gridtd.GridTDEngine) and name not in vars(aoa.AOAEngine), name
    for name in ("preprocess_img", "explain_cnn", "teacherforce_forward"):
        assert name not in vars(gridtd.ExplainGridTDAttention) and name not in vars(aoa.ExplainAOAAttention), name


def test_static_buffer_drivers_live_in_the_base_alone():
    from lrp_amd.explainers import engine_base
    here = os.path.dirname(os.path.abspath(engine_base.__file__))
    for mod in ("gridtd.py", "aoa.py"):
        with open(os.path.join(here, mod)) as f:
            src = f.read()
        for needle in ("CUDAGraph(", "Recording(", "torch.cuda.Event("):
            assert needle not in src, "%s still holds %s" % (mod, needle)
