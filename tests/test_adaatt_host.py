"""Host side of the single-LSTM adaptive-attention explainer (explainers/adaatt.py, csrc/lrpx_adaatt.hip): the new
symbols are declared, bound and exported; every new C entry refuses null pointers and bad sizes with EINVAL before any launch;
`weights.make_adaatt_state` gives the reference model's keys and shapes; `AdaAttEngine._check_state` refuses what is not this model's
state; the fixture meets the conditions its generator (tests/golden/make_golden_adaatt.py) searched for.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lrp_amd  # noqa: F401
from conftest import GOLDEN
from lrp_amd import _lib, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("lrpx_adaatt_fwd_inputs", "lrpx_adaatt_fwd_recurrence", "lrpx_adaatt_fwd_attention_all", "lrpx_adaatt_fwd_pre",
           "lrpx_adaatt_fwd_step", "lrpx_adaatt_rel_init", "lrpx_adaatt_rel_steps", "lrpx_adaatt_rel_glob", "lrpx_adaatt_rel_pix_rows")
FIXTURES = ("adaatt.npz", "adaatt_maps.npz")


@pytest.fixture(scope="module")
def g():
    with np.load(os.path.join(GOLDEN, "adaatt.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def test_symbols_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lrpx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lrpx_adaatt_[a-z0-9_]+)\s*\(", src))
    assert declared == set(ENTRIES)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES, name
    for struct in ("lrpx_adaatt_trace", "lrpx_adaatt_step_args", "lrpx_adaatt_relstate"):
        assert re.search(r"\}\s*%s\s*;" % struct, src), struct
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), "%s is declared in include/lrpx.h but not exported" % name
    from lrp_amd import explainers
    from lrp_amd.explainers import adaatt
    assert explainers.AdaAttEngine is adaatt.AdaAttEngine and explainers.ExplainAdaptiveAttention is adaatt.ExplainAdaptiveAttention
    assert issubclass(adaatt.AdaAttEngine, adaatt.EngineBase) and issubclass(adaatt.ExplainAdaptiveAttention, adaatt.ExplainerBase)
    # the ctypes structures follow the header's field order
    for cls, struct in ((_lib.AdaTrace, "lrpx_adaatt_trace"), (_lib.AdaStepArgs, "lrpx_adaatt_step_args"), (_lib.AdaRelState, "lrpx_adaatt_relstate")):
        body = re.search(r"typedef struct %s \{(.*?)\}" % struct, src, flags=re.S).group(1)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def _trace(**kw):
    """a trace whose pointers are non-null dummies (never dereferenced: every call below is refused on the host)"""
    t = _lib.AdaTrace()
    t.B, t.T, t.H, t.E, t.P = 2, 3, 512, 512, 12
    for name, _ in _lib.AdaTrace._fields_[5:]:
        setattr(t, name, 64)
    t.o = t.sgate = None
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _rel(**kw):
    r = _lib.AdaRelState()
    for name, _ in _lib.AdaRelState._fields_[1:]:
        setattr(r, name, 64)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_every_entry_refuses_null_pointers_and_bad_sizes():
    lib = _lib.load()
    P, p = C.byref, C.c_void_p(64)
    ok, okr = _trace(), _rel()
    sa = _lib.AdaStepArgs()
    for name, _ in _lib.AdaStepArgs._fields_:
        setattr(sa, name, 64)
    d = _lib.ConvDesc()          # all zero: not the gate rule
    calls = {
        "fwd_inputs": lambda tr, a=p: lib.lrpx_adaatt_fwd_inputs(P(tr), a, p, p, 4, None),
        "fwd_recurrence": lambda tr, a=p: lib.lrpx_adaatt_fwd_recurrence(P(tr), a, p, None),
        "fwd_attention_all": lambda tr, a=p: lib.lrpx_adaatt_fwd_attention_all(P(tr), a, p, p, p, p, p, p, None),
        "fwd_pre": lambda tr, a=p: lib.lrpx_adaatt_fwd_pre(P(tr), 0, a, p, p, 4, None),
        "fwd_step": lambda tr, a=p: lib.lrpx_adaatt_fwd_step(P(tr), 0, P(sa) if a else None, None),
        "rel_init": lambda tr, a=p: lib.lrpx_adaatt_rel_init(P(tr), P(okr), a, p, p, 4, None),
        "rel_steps": lambda tr, a=p: lib.lrpx_adaatt_rel_steps(P(tr), P(okr), 3, P(d) if a else None, p, 6, 1, None),
        "rel_glob": lambda tr, a=p: lib.lrpx_adaatt_rel_glob(P(tr), P(okr), a, p, None),
        "rel_pix_rows": lambda tr, a=p: lib.lrpx_adaatt_rel_pix_rows(P(tr), P(okr), a, p, p, None, 6, None),
    }
    assert len(calls) == len(ENTRIES)
    for name, call in calls.items():
        for bad in (_trace(H=256), _trace(T=0), _trace(P=300), _trace(E=500), _trace(xh=None), _trace(beta=None)):
            assert call(bad) == _lib.EINVAL, name
            assert b"adaatt" in lib.lrpx_last_error_string()
        assert call(ok, None) == _lib.EINVAL, name                      # a null argument (rel_steps with a full set: not the gate rule's descriptor)
    assert calls["rel_steps"](ok) == _lib.EINVAL and b"gate rule" in lib.lrpx_last_error_string()
    # a null trace / state, sizes out of range
    assert lib.lrpx_adaatt_fwd_inputs(None, p, p, p, 4, None) == _lib.EINVAL
    assert lib.lrpx_adaatt_fwd_inputs(P(ok), p, p, p, 2, None) == _lib.EINVAL                   # tok_ld < T
    assert lib.lrpx_adaatt_fwd_pre(P(ok), 3, p, p, p, 4, None) == _lib.EINVAL                   # t == T
    assert lib.lrpx_adaatt_fwd_step(P(ok), -1, P(sa), None) == _lib.EINVAL
    assert lib.lrpx_adaatt_rel_init(P(ok), None, p, p, p, 4, None) == _lib.EINVAL
    assert lib.lrpx_adaatt_rel_init(P(ok), P(_rel(r_ctx=None)), p, p, p, 4, None) == _lib.EINVAL
    assert lib.lrpx_adaatt_rel_init(P(ok), P(okr), p, p, p, 3, None) == _lib.EINVAL             # tok_ld must hold T + 1 ids
    assert lib.lrpx_adaatt_rel_steps(P(ok), P(okr), 4, P(d), p, 6, 1, None) == _lib.EINVAL      # n_steps > T
    assert lib.lrpx_adaatt_rel_steps(P(ok), P(okr), 3, P(d), p, 5, 1, None) == _lib.EINVAL      # idx_ld < B*T
    assert lib.lrpx_adaatt_rel_pix_rows(P(ok), P(okr), p, p, p, None, 5, None) == _lib.EINVAL   # no row list: n_rows must be B*T
    assert lib.lrpx_adaatt_rel_pix_rows(P(ok), P(okr), p, p, p, p, 0, None) == _lib.EINVAL
    assert lib.lrpx_adaatt_rel_pix_rows(P(ok), P(okr), p, p, p, p, 7, None) == _lib.EINVAL


def test_state_has_the_reference_models_keys_and_shapes(g):
    sd = weights.make_adaatt_state(seed=int(g["seed"]), vocab_size=int(g["V"]))
    assert list(sd) == [str(k) for k in g["state_keys"]]
    for k, shp in zip(g["state_keys"], g["state_shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(s) for s in shp if s), k
    bare = weights.make_adaatt_state(seed=3, vocab_size=503, feat_dim=192, num_pixels=12, encoder=None)
    assert not [k for k in bare if k.startswith("img_encoder.")]
    assert list(bare) == [k for k in sd if not k.startswith("img_encoder.")]
    assert bare["img_projector.weight"].shape == (512, 192, 1, 1) and bare["AdaAttention.W_v_proj.weight"].shape == (12, 512)
    assert bare["AdaLSTM.lstm_cell.weight_ih"].shape == (2048, 1024) and bare["AdaLSTM.x_gate.weight"].shape == (512, 1024)
    again = weights.make_adaatt_state(seed=3, vocab_size=503, feat_dim=192, num_pixels=12, encoder=None)
    assert all(np.array_equal(bare[k], again[k]) for k in bare)
    with pytest.raises(ValueError):
        weights.make_adaatt_state(encoder="resnet101")


def test_check_state_refusals():
    from lrp_amd.explainers.adaatt import AdaAttEngine
    good = weights.make_adaatt_state(seed=1, vocab_size=307, feat_dim=192, num_pixels=12, encoder=None)
    AdaAttEngine._check_state(good)
    with pytest.raises(ValueError, match="gridTD state"):
        AdaAttEngine._check_state(weights.make_gridtd_resnet_state(seed=1, vocab_size=307, feat_dim=192, num_pixels=12))
    wide = dict(good)
    wide["AdaLSTM.lstm_cell.weight_ih"] = np.zeros((2048, 1536), np.float32)
    with pytest.raises(ValueError, match="2E = 1024"):
        AdaAttEngine._check_state(wide)
    flat = dict(good)
    flat["img_projector.weight"] = good["img_projector.weight"].reshape(512, 192)
    with pytest.raises(ValueError, match="1 x 1 Conv2d"):
        AdaAttEngine._check_state(flat)
    with pytest.raises(ValueError, match="gridTD state"):          # ... and the constructor refuses before it touches the device
        AdaAttEngine(weights.make_gridtd_resnet_state(seed=1, vocab_size=307, feat_dim=192, num_pixels=12))


def test_interleaved_gate_rows():
    from lrp_amd.explainers.adaatt import interleave_index
    il = interleave_index(512).numpy()
    assert il.shape == (16 * 171,) and il.max() == 5 * 512
    live = il[il < 5 * 512]
    assert sorted(live.tolist()) == list(range(5 * 512))            # every gate row exactly once
    for r in (0, 7, 16 * 100 + 11, 16 * 170 + 9):
        j, k = divmod(r, 16)
        u, q = divmod(k, 5)
        assert il[r] == q * 512 + 3 * j + u
    assert (il[15::16] == 5 * 512).all() and (il[16 * 170 + 10:] == 5 * 512).all()          # padding rows: the zero row


def test_fixture_meets_its_conditions(g):
    for k in ("small", "long", "vgg"):
        assert float(g[k + "_e32_r_feat"]) < 1e-5, k
        assert float(g[k + "_e32_r_words"]) < 3e-6, k
    assert float(g["decode_margin"]) > 1e-4
    assert g["small_r_feat"].shape == (2, 3, 12, 192) and g["long_r_feat"].shape == (3, 12, 192) and g["vgg_r_feat"].shape == (3, 196, 128)
    assert g["long_words"].tolist() == [23, 24, 25] and g["long_caption"].shape == (1, 27)
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 1 << 20, name
    with np.load(os.path.join(GOLDEN, "adaatt_maps.npz"), allow_pickle=False) as f:
        assert int(f["seed"]) == int(g["seed"]) and f["vgg_map_full_2"].shape == (1, 3, 224, 224)
