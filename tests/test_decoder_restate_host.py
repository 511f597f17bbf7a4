"""tests/decoder_restate.py pinned on the CPU: (1) on REAL traces of the oracle (oracle/lrp_oracle.py, which the reference's own fixtures
pin) the fp32 restatements reproduce `gridtd_explain_wordt`, `aoa_explain_wordt`, `gridtd_guided_wordt` and `aoa_gradient_wordt` for every
word, within the bounds the suite holds these quantities to (`_check_rows`, tests/test_gpu_gridtd_bu.py: feature side 1e-4 of the maximum,
r_words 1e-5); (2) every drawn case of tests/test_gpu_decoder_alone.py meets the yardstick condition: of the three fp32 summation orders
each lies within C x max(the worst of the other two, FLOOR) of fp64 - one order alone is too narrow a yardstick for sums that cancel."""
import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from lrp_amd import weights

import decoder_restate as R
from conftest import rel_err
from fp64_anchor import C as C_GRADE, FLOOR

V, T = 61, 4


def _O():
    from oracle import lrp_oracle as O
    return O


def _sd(np_state):
    return {k: torch.from_numpy(v) for k, v in np_state.items()}


def _b(x):
    return x.unsqueeze(0)


def _logit(tr):
    return torch.stack([tr["pred"][t][tr["caption"][t + 1]] for t in range(tr["T"])])


def _check(what, feat, want_feat, words, want_words, t):
    e, d = rel_err(feat, want_feat), float((words[:t + 1] - want_words).abs().max())
    print("%s word %d: feature side %.2e of the maximum, r_words %.2e" % (what, t, e, d))
    assert e < 1e-4 and d < 1e-5, (what, t, e, d)
    assert torch.count_nonzero(words[t + 1:]) == 0


@pytest.fixture(scope="module")
def gridtd():
    O = _O()
    sd = _sd(weights.make_gridtd_resnet_state(seed=3, vocab_size=V, feat_dim=64, num_pixels=6))
    rs = np.random.RandomState(11)
    feats = torch.from_numpy(np.maximum(rs.standard_normal((64, 2, 3)), 0).astype(np.float32))
    cap = weights.make_captions(5, 1, T, V)[0]
    return O, sd, feats, feats.reshape(64, -1).mean(1), cap


def _gridtd_d(tr, grad):
    d = dict(h2=_b(tr["h2"]), c1=_b(tr["c1"]), c2=_b(tr["c2"]), alpha=_b(tr["alpha"]), beta=_b(tr["beta"]),
             tok=torch.tensor([tr["caption"]]), logit=_logit(tr))
    for k in ("i1", "f1", "i2", "f2", "s", "ctx", "ctx_hat"):
        d[k] = _b(tr[k])
    if grad:      # the oracle's gradient trace keeps tanh(g): back to the pre-activation the kernels read
        for k in ("g1", "g2"):
            d[k] = _b(torch.atanh(tr[k].double()).float())
        d["o1"], d["o2"], d["sgate"] = _b(tr["o1"]), _b(tr["o2"]), _b(tr["sen_gate"])
    else:
        d["g1"], d["g2"] = _b(tr["g1"]), _b(tr["g2"])
        d["xh1"], d["xh2"] = _b(torch.cat([tr["x1"], tr["h1"][:-1]], 1)), _b(torch.cat([tr["x2"], tr["h2"][:-1]], 1))
        d["hc"] = _b(tr["h2"][1:] + tr["ctx_hat"])
        for k in ("Vp", "proj_pre", "glob_pre", "avg"):
            d[k] = _b(tr[k])
    return d


def test_gridtd_relevance_restated_vs_oracle(gridtd):
    O, sd, feats, avg, cap = gridtd
    tr = O.gridtd_trace(sd, feats, avg, cap)
    out = R.gridtd_rel(_gridtd_d(tr, False), sd, None, torch.float32, "torch")
    w_proj, P = sd["img_projector.weight"].reshape(R.H, -1), tr["P"]
    for t in range(T):
        want_feat, want_words = O.gridtd_explain_wordt(sd, tr, t)
        r_avg = O.eps_dense(out["r_glob"][t], tr["avg"], tr["glob_pre"], sd["global_img_feature_proj.weight"])           # :1116-1119
        r_feat = O.eps_identity(r_avg[None], tr["F_pix"] / P, tr["avg"][None]) \
            + O.eps_dense(out["a_proj"][t] * O.eps_stabilise(tr["proj_pre"]), tr["F_pix"], tr["proj_pre"], w_proj)       # :1120-1128
        _check("gridTD relevance", r_feat, want_feat, out["r_words_norm"][t], want_words, t)
        assert torch.equal(out["a_glob"][t], out["r_glob"][t] / O.eps_stabilise(tr["glob_pre"]))
        assert torch.equal(R.gridtd_u(r_avg[None], tr["avg"][None], 1, P)[0], r_avg / (P * O.eps_stabilise(tr["avg"])))


def test_gridtd_guided_restated_vs_oracle(gridtd):
    O, sd, feats, avg, cap = gridtd
    tr = O.gridtd_grad_trace(sd, feats, avg, cap)
    out = R.gridtd_grad(_gridtd_d(tr, True), sd, None, torch.float32, "torch")
    w_proj, P = sd["img_projector.weight"].reshape(R.H, -1), tr["P"]
    for t in range(T):
        want_feat, want_words = O.gridtd_guided_wordt(sd, tr, t)
        d_avg = out["d_glob"][t] @ sd["global_img_feature_proj.weight"]                                                  # :1663-1667
        d_feat = (d_avg[None] / P + out["a_proj"][t] @ w_proj) * (tr["F_pix"] > 0).float()                               # :1668, :1674
        _check("gridTD guided", d_feat, want_feat, out["r_words_norm"][t], want_words, t)


@pytest.fixture(scope="module")
def aoa():
    O = _O()
    sd = _sd(weights.make_aoa_state(seed=3, vocab_size=V, feat_dim=64, with_encoder=False))
    rs = np.random.RandomState(12)
    F_pix = torch.from_numpy(np.maximum(rs.standard_normal((5, 64)), 0).astype(np.float32))
    return O, sd, F_pix, weights.make_captions(6, 1, T, V)[0]


def _aoa_d(tr, grad):
    d = dict(xh=_b(torch.cat([tr["x"], tr["h"][:-1]], 1)), h=_b(tr["h"]), c=_b(tr["c"]), tok=torch.tensor([tr["caption"]]), logit=_logit(tr),
             lin=_b(tr["c_aoa_lin"]), hc=_b(tr["h"][1:] + tr["c_aoa"]), glob=_b(tr["glob"]))
    for k in ("g", "i", "f", "ctx", "c_aoa", "alpha", "value", "Vp", "proj_pre"):
        d[k] = _b(tr[k])
    if grad:
        d["o"], d["sg"] = _b(tr["o"]), _b(torch.sigmoid(tr["c_aoa_gate"]))
    return d


@pytest.mark.parametrize("head", [0, 7])
def test_aoa_relevance_restated_vs_oracle(aoa, head):
    O, sd, F_pix, cap = aoa
    tr = O.aoa_trace(sd, F_pix, cap)
    out = R.aoa_rel(_aoa_d(tr, False), sd, head, None, torch.float32, "torch")
    w_proj, P = sd["img_projector.weight"].reshape(R.H, -1), tr["P"]
    for t in range(T):
        want_feat, want_words = O.aoa_explain_wordt(sd, tr, t, head)
        r_proj = O.eps_identity(out["r_glob"][t][None], tr["Vp"] / P, tr["glob"][None]) \
            + O.eps_dense(out["a_val"][t] * O.eps_stabilise(tr["value"]), tr["Vp"], tr["value"], sd["decoder_v_proj.weight"])   # :1136-1144
        r_feat = O.eps_dense(r_proj, tr["F_pix"], tr["proj_pre"], w_proj)                                                # :1145-1148
        _check("AoA relevance, head %d" % head, r_feat, want_feat, out["r_words_norm"][t], want_words, t)
        assert torch.equal(out["U"][t], out["r_glob"][t] / (P * O.eps_stabilise(tr["glob"])))


@pytest.mark.parametrize("head", [0, 7])
def test_aoa_gradient_restated_vs_oracle(aoa, head):
    O, sd, F_pix, cap = aoa
    tr = O.aoa_trace(sd, F_pix, cap, grad=True)
    out = R.aoa_grad(_aoa_d(tr, True), sd, head, None, torch.float32, "torch")
    for t in range(T):
        want_feat, want_words = O.aoa_gradient_wordt(sd, tr, t, head)
        _check("AoA gradient, head %d" % head, out["d_feat"][t], want_feat, out["r_words_norm"][t], want_words, t)


def test_lens_leave_zero_rows_and_the_live_rows_alone(aoa):
    """`lens`: rows behind an image's last word are zero in every output, the live rows are those of the full evaluation"""
    O, sd, F_pix, cap = aoa
    d = _aoa_d(O.aoa_trace(sd, F_pix, cap, grad=True), True)
    for fn in (lambda l: R.aoa_rel(d, sd, 3, l, torch.float32, "rev128"), lambda l: R.aoa_grad(d, sd, 3, l, torch.float32, "il128")):
        full, cut = fn(None), fn([2])
        for k in full:
            assert torch.equal(cut[k][:2], full[k][:2]) and torch.count_nonzero(cut[k][2:]) == 0, k


# ---- (2) the yardstick condition on every drawn case ---------------------------------------------------------------------------------------
def _yardstick(what, refs32, ref64, live):
    worst, e32 = 0.0, 0.0
    for k in ref64:
        errs = R.worst_of(refs32, ref64, k, live)[1]
        e32 = max(e32, max(errs))
        for j, e in enumerate(errs):
            others = max(errs[:j] + errs[j + 1:])
            ratio = e / max(others, FLOOR)
            worst = max(worst, ratio)
            assert e <= C_GRADE * max(others, FLOOR), "%s %s: fp32 in order %s is %.2e from fp64, the worst of the other two %.2e: not a " \
                "draw the kernels can be graded on (another seed, or the floor)" % (what, k, R.ORDERS[j], e, others)
    print("%s: worst e / max(worst other order, FLOOR) over all outputs %.2f; fp32 at worst %.1e of the maximum from fp64" % (what, worst, e32))


@pytest.mark.parametrize("family, T_, lens", R.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_drawn_cases_meet_the_yardstick(family, T_, lens):
    case = R.case(family, T_, lens)
    ref64, refs32, live = R.references(family, T_, lens)
    assert live.any() and not any(torch.isnan(v).any() or torch.isinf(v).any() for v in ref64.values())
    print("%s T %d lens %s: max|.| %s" % (family, T_, lens, ", ".join("%s %.1e" % (k, float(v.abs().max())) for k, v in ref64.items())))
    _yardstick("%s T %d lens %s" % (family, T_, lens), refs32, ref64, live)
    assert case is R.case(family, T_, lens)          # (the draws are cached: the kernel tests see these very tensors)
