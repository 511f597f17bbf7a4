"""The bottom-up gridTD model, `GridTDModelBU` (models/gridTDmodel.py:1863-2464), without a device: the synthetic state has the key names and
shapes the reference's `state_dict()` had when tests/golden/gridtd_bu.npz was written, `GridTDBUEngine` refuses a state that is not that
model's by host logic alone (before the library is loaded, before any device is asked for), and the fixture is what its generator
(tests/golden/make_golden_gridtd_bu.py) says it is: arrays only, finite, and within its own recorded conditions."""
import os

import numpy as np
import pytest

import lrp_amd  # noqa: F401
from conftest import GOLDEN
from lrp_amd import _lib, weights
from lrp_amd.explainers.gridtd import GridTDBUEngine, GridTDEngine

FIXTURE = os.path.join(GOLDEN, "gridtd_bu.npz")


@pytest.fixture(scope="module")
def g():
    with np.load(FIXTURE, allow_pickle=False) as f:          # arrays only: an object array would raise here
        return {k: f[k] for k in f.files}


def _small_state(**kw):
    return weights.make_gridtd_bu_state(seed=0, vocab_size=53, **kw)


def test_state_has_the_recorded_keys_and_shapes(g):
    sd = weights.make_gridtd_bu_state(seed=int(g["seed"]), vocab_size=int(g["V"]))
    assert list(sd) == [str(k) for k in g["state_keys"]]
    for (k, v), shape in zip(sd.items(), g["state_shapes"]):
        assert list(v.shape) == [int(s) for s in shape[:v.ndim]] and not shape[v.ndim:].any(), k
        assert v.dtype == np.float32
    assert sd["img_projector.weight"].shape == (512, 2048) and sd["global_img_feature_proj.weight"].shape == (512, 512)
    assert sd["AdaAttention.W_v_proj.weight"].shape == (36, 512) and not any(k.startswith("img_encoder.") for k in sd)
    # the defaults are the reference's sizes; the draw is a function of the seed alone
    again = weights.make_gridtd_bu_state(seed=int(g["seed"]), vocab_size=int(g["V"]))
    assert all(np.array_equal(sd[k], again[k]) for k in sd)


def _no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was loaded before the state was refused")
    monkeypatch.setattr(_lib, "load", boom)


def test_refuses_a_state_with_encoder_keys(monkeypatch):
    _no_library(monkeypatch)
    sd = _small_state()
    sd["img_encoder.encoder.0.weight"] = np.zeros((64, 3, 3, 3), np.float32)
    with pytest.raises(ValueError, match=r"img_encoder\.encoder\.0\.weight"):
        GridTDBUEngine(sd)


def test_refuses_a_4d_projector(monkeypatch):
    _no_library(monkeypatch)
    sd = _small_state()
    sd["img_projector.weight"] = sd["img_projector.weight"].reshape(512, 2048, 1, 1)
    with pytest.raises(ValueError, match=r"img_projector\.weight"):
        GridTDBUEngine(sd)


def test_refuses_a_global_projector_whose_input_is_not_h(monkeypatch):
    _no_library(monkeypatch)
    sd = _small_state()
    sd["global_img_feature_proj.weight"] = np.zeros((512, 2048), np.float32)          # `GridTDModel`'s: from the raw features
    with pytest.raises(ValueError, match=r"global_img_feature_proj\.weight"):
        GridTDBUEngine(sd)
    with pytest.raises(ValueError, match=r"img_projector\.weight"):          # the decoder state of a ResNet gridTD model: its 1 x 1 conv comes first
        GridTDBUEngine(weights.make_gridtd_resnet_state(seed=0, vocab_size=53, num_pixels=36))


def test_is_a_gridtd_engine_with_its_own_surface():
    assert issubclass(GridTDBUEngine, GridTDEngine)
    for name in ("encode", "explain_batch", "explain_batch_graph", "explain_batch_replay", "explain_stream", "guided_gradient",
                 "explain_batch_guided", "explain_batch_gradient", "_rel_tail"):
        assert name in vars(GridTDBUEngine), name
    for name in ("greedy", "trace", "relevance", "beam_search", "sample_lrp", "forwardlrp_context", "replica"):      # inherited
        assert name not in vars(GridTDBUEngine) and hasattr(GridTDBUEngine, name), name


def test_fixture_is_arrays_only_finite_and_within_its_conditions(g):
    assert os.path.getsize(FIXTURE) < 1 << 20
    for k, v in g.items():
        assert isinstance(v, np.ndarray) and v.dtype != object, k
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), k
    assert float(g["pair_e32_r_feat"]) < 1e-5 and float(g["long_e32_r_feat"]) < 1e-5
    assert float(g["pair_e32_r_words"]) < 3e-6 and float(g["long_e32_r_words"]) < 3e-6
    assert float(g["decode_margin"]) > 1e-4
    B, T, P, C = 2, 3, 36, 2048
    assert g["pair_r_feat"].shape == (B, P, C, T) and g["pair_r_feat"].dtype == np.float32          # stored word last
    r_feat, r_long = g["pair_r_feat"].transpose(0, 3, 1, 2), g["long_r_feat"].transpose(2, 0, 1)
    assert g["pair_r_words"].shape == (B, T, T) and g["pair_r_words64"].dtype == np.float64
    assert g["pair_nonzero"].tolist() == [36, 20] and g["long_nonzero"].tolist() == [8]
    assert not r_feat[1, :, 20:].any()                                            # padded regions: exact zeros
    assert r_feat[1, :, :20].any(axis=-1).all() and r_feat[0].any(axis=-1).all()
    assert g["long_words"].tolist() == [23, 24, 25] and g["long_caption"].shape == (1, 27)
    assert r_long.shape == (3, P, C) and not r_long[:, 8:].any() and r_long[:, :8].any(axis=-1).all() and g["long_r_words"].shape == (3, 26)
    for t in range(T):                                                            # entries behind word t are zero; the largest is 1
        assert not g["pair_r_words"][:, t, t + 1:].any()
        assert np.allclose(np.abs(g["pair_r_words"][:, t]).max(-1), 1.0)
    # the recorded fp32 - fp64 distance of r_words is the one the two stored arrays have
    e = np.abs(g["pair_r_words"].astype(np.float64) - g["pair_r_words64"]).max() / np.abs(g["pair_r_words64"]).max()
    assert abs(e - float(g["pair_e32_r_words"])) < 1e-12
    assert g["decode_greedy"].shape == (2, 6) and g["decode_sample_seq"].shape == (2, 8) and g["decode_fl_pred_sub"].shape[:2] == (2, 8)
