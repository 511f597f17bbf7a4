"""The alpha-beta rule of a conv under a 2x2 max-pool, decided on the CPU: the folded formulation the kernels implement
equals the reference's layered rule; the cases of tests/test_gpu_vgg_ab.py are fit for the fp32-grade criterion; the `lrp_params`
switch of the caption engines refuses what it must before any device work."""
import math

import pytest
import torch

import vgg_ab_cases as V
from conftest import rel_err
from fp64_anchor import C, FLOOR, SIX, THREE, WITNESS_MARGIN

NAMES = [c[0] for c in V.EDGE_CASES]


@pytest.mark.parametrize("name", NAMES)
def test_folded_formulation_equals_the_layered_rule_in_fp64(name):
    c = V.case(name)
    for alpha, beta in ((V.ALPHA, V.BETA), (1.5, 0.5), (1., 0.)):
        want = V.layered(c, torch.float64, alpha, beta)
        got = V.reference(c, torch.float64, addend=False, alpha=alpha, beta=beta, q=V.coef(c, torch.float64))
        assert rel_err(got, want) < 1e-12, (name, alpha, beta, rel_err(got, want))


def test_the_cases_hold_ties_zero_windows_and_uncovered_pixels():
    c = V.case("c11x9_20_36")
    win = V.winners(c["a"])
    assert win[:, :, 10, :].abs().sum() == 0 and win[:, :, :, 8].abs().sum() == 0          # under no window
    pooled = torch.nn.functional.max_pool2d(c["a"], 2, 2)
    assert (pooled == 0).any() and (pooled != 0).any()                                      # all-zero windows: no winner
    a = c["a"][:, :, :10, :8].unfold(2, 2, 2).unfold(3, 2, 2).flatten(4)
    assert ((a == a.max(-1, keepdim=True).values).sum(-1) > 1)[pooled != 0].any()           # ties among non-zero maxima
    assert win.sum() == (pooled != 0).sum()                                                 # exactly one winner per non-zero window
    assert V.upsample(c, c["r"])[:, :, 10, :].abs().sum() == 0


@pytest.mark.parametrize("name", NAMES)
def test_cases_are_fit_for_the_fp32_grade_criterion(name):
    worst, least = V.fit(V.case(name))
    assert worst <= 1, f"{name}: the six-product emulation misses C x max(e32, FLOOR) ({worst:.2f} x the bound)"
    assert least >= WITNESS_MARGIN, f"{name}: the three-product witness is only {least:.2f} x the bound"


def test_criterion_constants_are_the_anchor_modules():
    assert (C, FLOOR, WITNESS_MARGIN) == (6.0, 1e-7, 2.0) and len(SIX) == 6 and len(THREE) == 3


# ---- the lrp_params switch (explainers/engine_base.py) -----------------------------------------------------------------------------------
def _engine(cnn="vgg", resnet=False, lrp_params=None):
    from lrp_amd.explainers.engine_base import EngineBase

    class Enc(object):
        def relevance(self, feat, row2img):
            return "preset"

        def relevance_alpha_beta(self, feat, row2img, alpha, beta):
            return ("ab", alpha, beta)
    e = EngineBase.__new__(EngineBase)
    e.cnn = Enc() if cnn else None
    e.vgg, e.resnet, e.lrp_params = None, resnet, lrp_params
    return e


def test_lrp_rule_accepts_and_normalises():
    from lrp_amd.explainers.engine_base import _lrp_rule
    assert _lrp_rule("t", None) is None
    assert _lrp_rule("t", {}) is None
    assert _lrp_rule("t", {"alpha": 1., "beta": 0.}) is None
    assert _lrp_rule("t", {"alpha": 1, "beta": 0, "ignore_bias": True}) is None
    assert _lrp_rule("t", {"alpha": 2., "beta": 1.}) == (2., 1.)
    assert _lrp_rule("t", {"alpha": 1.5, "beta": 0.5, "ignore_bias": True}) == (1.5, 0.5)
    assert _lrp_rule("t", {"beta": 1}) == (1., 1.)
    assert _lrp_rule("t", {"alpha": 3.}) == (3., 0.)


@pytest.mark.parametrize("bad", [{"alpha": 2., "gamma": 1.}, {"alpha": math.nan, "beta": 1.}, {"alpha": 2., "beta": math.inf},
                                 {"alpha": 2., "beta": -math.inf}, {"alpha": 2., "beta": 1., "ignore_bias": False}, {"alpha": "2"},
                                 {"alpha": None, "beta": 1.}, {"alpha": True}, [2., 1.], (2., 1.), "alpha2beta1"])
def test_lrp_rule_refuses(bad):
    from lrp_amd.explainers.engine_base import _lrp_rule
    with pytest.raises(ValueError, match="Eng.entry"):
        _lrp_rule("Eng.entry", bad)


def test_maps_stage_of_an_engine_without_a_device():
    e = _engine()
    assert e._maps_stage("explain_batch")(None, None) == "preset"                       # None: the engine's own relevance
    assert e._maps_stage("explain_batch").__self__ is e.cnn                             # ... the bound method itself, no wrapper
    e.lrp_params = {"alpha": 1., "beta": 0.}
    assert e._maps_stage("explain_batch").__self__ is e.cnn
    e = _engine(resnet=True, lrp_params={"alpha": 2., "beta": 1.})
    assert e._maps_stage("explain_batch")(None, None) == ("ab", 2., 1.)
    assert e._maps_stage("explain_cnn", None)(None, None) == "preset"                   # a drop-in's own value wins, the engine's is not read
    assert e._maps_stage("explain_cnn", {"alpha": 1.5, "beta": .5})(None, None) == ("ab", 1.5, .5)
    assert e.lrp_params == {"alpha": 2., "beta": 1.}                                    # ... and is not written
    with pytest.raises(ValueError, match="unknown keys"):
        _engine(lrp_params={"alhpa": 2.})._maps_stage("explain_batch")
    with pytest.raises(ValueError, match="ignore_bias"):
        _engine(lrp_params={"ignore_bias": False})._maps_stage("explain_batch")


def test_engines_without_an_encoder_refuse_the_switch():
    e = _engine(cnn=None)
    assert e._maps_stage("explain_batch") is None
    e._features_stage("explain_features")
    e._preset_only("explain_batch_graph", "why")
    for params in ({"alpha": 2., "beta": 1.}, {"alpha": 1., "beta": 0.}, {}):
        e.lrp_params = params
        for call in (lambda: e._maps_stage("explain_batch"), lambda: e._features_stage("explain_features"),
                     lambda: e._preset_only("explain_batch_graph", "why")):
            with pytest.raises(ValueError, match="EngineBase.explain"):
                call()
    with_encoder = _engine(lrp_params={"alpha": 2., "beta": 1.})
    with pytest.raises(ValueError, match="features"):
        with_encoder._features_stage("explain_batch")                                   # AoA features= on an engine that has an encoder


def test_graph_replay_and_gradient_entries_are_preset_only():
    e = _engine(lrp_params={"alpha": 2., "beta": 1.})
    with pytest.raises(NotImplementedError, match="EngineBase.explain_batch_graph.*not recordable"):
        e._preset_only("explain_batch_graph", e._NO_STATIC_AB)
    with pytest.raises(NotImplementedError, match="gradient family"):
        e._preset_only("explain_batch_gradient", e._NO_GRAD_AB)
    with pytest.raises(ValueError, match="unknown keys"):                                # validation comes first
        _engine(lrp_params={"beta ": 1.})._preset_only("explain_batch_graph", "why")
    for params in (None, {"alpha": 1., "beta": 0.}, {}):
        _engine(lrp_params=params)._preset_only("explain_batch_graph", "why")


def test_entry_points_validate_before_any_device_work():
    """every entry point of the three engines reaches the helper before it touches its arguments: a bare engine (no weights, no
    device) with a bad `lrp_params` raises the helper's ValueError from arguments that would fail anything else"""
    from lrp_amd.explainers.adaatt import AdaAttEngine
    from lrp_amd.explainers.aoa import AOAEngine
    from lrp_amd.explainers.gridtd import GridTDBUEngine, GridTDEngine
    bad, ab = {"alpha": 2., "oops": 1.}, {"alpha": 2., "beta": 1.}

    def bare(cls, params, cnn=True):
        e = cls.__new__(cls)
        e.cnn = object() if cnn else None
        e.vgg, e.resnet, e.lrp_params = None, True, params
        return e
    for cls in (GridTDEngine, AdaAttEngine):
        for entry in ("explain_batch", "explain_stream", "explain_batch_graph", "explain_batch_replay"):
            with pytest.raises(ValueError, match="unknown keys"):
                getattr(bare(cls, bad), entry)(None, None)
        for entry in ("explain_batch_graph", "explain_batch_replay"):
            with pytest.raises(NotImplementedError, match="lrp_params"):
                getattr(bare(cls, ab), entry)(None, None)
    for entry in ("explain_batch_gradient", "explain_batch_guided"):
        with pytest.raises(NotImplementedError, match="lrp_params"):
            getattr(bare(GridTDEngine, ab), entry)(None, None)
    for entry in ("explain_batch", "explain_batch_graph", "explain_batch_replay"):
        with pytest.raises(ValueError, match="unknown keys"):
            getattr(bare(AOAEngine, bad), entry)(None, 0, images=None)
    with pytest.raises(ValueError, match="unknown keys"):
        bare(AOAEngine, bad).explain_stream(None, 0)
    for entry in ("explain_batch_graph", "explain_batch_replay", "explain_batch_gradient"):
        with pytest.raises(NotImplementedError, match="lrp_params"):
            getattr(bare(AOAEngine, ab), entry)(None, 0, images=None)
    for entry in ("explain_batch", "explain_batch_graph", "explain_batch_replay"):
        with pytest.raises(ValueError, match="features"):
            getattr(bare(AOAEngine, ab), entry)(None, 0, features=object())
    with pytest.raises(ValueError, match="features"):
        bare(AdaAttEngine, ab).explain_features(None, None)
    from lrp_amd.explainers.adaatt_grad import AdaAttGradEngine
    for entry in ("explain_batch_gradient", "explain_batch_guided"):
        with pytest.raises(NotImplementedError, match="lrp_params"):
            getattr(bare(AdaAttGradEngine, ab), entry)(None, None)
        with pytest.raises(ValueError, match="unknown keys"):
            getattr(bare(AdaAttGradEngine, bad), entry)(None, None)
        getattr(AdaAttGradEngine, entry)                                                # (the preset passes the helper: checked on the GPU)
    with pytest.raises(ValueError, match="features"):
        bare(AdaAttGradEngine, ab).explain_features_gradient(None, None)
    with pytest.raises(ValueError, match="features"):
        bare(AdaAttGradEngine, {"alpha": 1., "beta": 0.}).explain_features_gradient(None, None)
    with pytest.raises(ValueError, match="no encoder"):
        bare(GridTDBUEngine, ab, cnn=False).explain_batch(None, None)
    with pytest.raises(ValueError, match="no encoder"):
        bare(GridTDBUEngine, ab, cnn=False).explain_stream([])


def test_vgg16_conv_mode_and_pool_keyword_are_refused_on_the_host():
    from lrp_amd import ops
    v = ops.Vgg16.__new__(ops.Vgg16)
    for mode in (2, 3, -1, True, None):
        with pytest.raises(ValueError, match="conv_mode"):
            v.relevance_alpha_beta(None, conv_mode=mode)
    with pytest.raises(ValueError, match="finite"):
        v.relevance_alpha_beta(None, alpha=math.nan, conv_mode=1)
    for pool in (0, 3, 4):
        with pytest.raises(ValueError, match="pool"):
            ops.conv_geom_ab(None, None, 1, (4, 4), (4, 4), (3, 3, 1, 1, 1, 1), 4, 4, None, None, pool=pool)
