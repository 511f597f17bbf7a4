"""tests/decoder_fwd_restate.py pinned on the CPU: (1) on REAL inputs the fp32 restatements reproduce the oracle's `gridtd_trace` (both
`gate_h_new`, both biases), `aoa_trace` (both biases) and `gridtd_lrp_weights`, and the reference's own run of the single-LSTM model stored in
tests/golden/adaatt.npz (`small_tr_*`, `long_tr_*`) - every trace tensor within 1e-5 of its maximum; (2) every drawn case of
tests/test_gpu_decoder_fwd_alone.py is what its description says (scores past +-89, sentinel above / below every pixel score, saturated gates,
the AoA heads' spans) and meets the yardstick condition of tests/test_decoder_restate_host.py::_yardstick: of the three fp32 summation orders
each lies within C x max(the worst of the other two, FLOOR) of fp64.  A condition on the inputs, not a measurement of the kernels."""
import os

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from lrp_amd import weights

import decoder_fwd_restate as F
from conftest import GOLDEN, rel_err
from test_decoder_restate_host import _yardstick

V, T = 61, 4
BOUND = 1e-5


def _O():
    from oracle import lrp_oracle as O
    return O


def _sd(np_state):
    return {k: torch.from_numpy(v) for k, v in np_state.items()}


def _close(what, got, want):
    e = rel_err(got, want)
    print("%s: %.2e of the maximum" % (what, e))
    assert tuple(got.shape) == tuple(want.shape) and e < BOUND, (what, e)


# ---- (1) the restatements against the oracle and the reference's stored run ----------------------------------------------------------------
@pytest.mark.parametrize("model_bias, gate_h_new", [(False, False), (False, True), (True, True), (True, False)])
def test_gridtd_fwd_restated_vs_oracle(model_bias, gate_h_new):
    O = _O()
    sd = _sd(weights.make_gridtd_resnet_state(seed=3, vocab_size=V, feat_dim=64, num_pixels=6))
    rs = np.random.RandomState(11)
    feats = torch.from_numpy(np.maximum(rs.standard_normal((64, 2, 3)), 0).astype(np.float32))
    cap = weights.make_captions(5, 1, T, V)[0]
    tr = O.gridtd_trace(sd, feats, feats.reshape(64, -1).mean(1), cap, model_bias=model_bias, gate_h_new=gate_h_new)
    att_img = tr["Vp"] @ sd["AdaAttention.W_v_proj.weight"].t() + sd["AdaAttention.W_v_proj.bias"]
    enc = dict(glob=tr["glob"][None], Vp=tr["Vp"][None], att_img=att_img[None])
    out = F.gridtd_fwd(sd, enc, torch.from_numpy(cap)[None], torch.float32, "torch", model_bias, gate_h_new)
    for k in ("h1", "c1", "h2", "c2", "g1", "i1", "f1", "g2", "i2", "f2", "s", "ctx", "ctx_hat", "alpha", "beta"):
        _close("gridTD " + k, out[k][0], tr[k])
    _close("gridTD x1", out["xh1"][0][:, :F.H + 2 * F.E], tr["x1"])
    _close("gridTD x2", out["xh2"][0][:, :2 * F.H], tr["x2"])
    assert torch.equal(out["xh1"][0][:, F.H + 2 * F.E:], out["h1"][0][:-1]) and torch.equal(out["xh2"][0][:, 2 * F.H:], out["h2"][0][:-1])
    pred = out["hc"][0] @ sd["fc.weight"].t() + sd["fc.bias"]
    _close("gridTD pred", pred, tr["pred"])
    want = torch.stack([tr["pred"][t][tr["caption"][t + 1]] for t in range(T)])
    _close("gridTD target logit", F.target_logit(out["hc"], sd["fc.weight"], sd["fc.bias"], torch.from_numpy(cap)[None], torch.float32, "torch"), want)
    # get_lrp_weight_step on the trace's own scores: a skipped arg-max word and one that is not
    for t in range(T):
        k = int(torch.argmax(tr["pred"][t]))
        for skip_ids in ((), (k,)):
            skip = torch.zeros(V, dtype=torch.bool)
            skip[list(skip_ids)] = True
            w_ctx, w_h = O.gridtd_lrp_weights(sd, tr["pred"][t], tr["h2"][t + 1], tr["ctx_hat"][t], set(skip_ids))
            hcw, ks, wh_, wc_ = F.lrp_reweight(tr["pred"][t][None], tr["h2"][t + 1][None], tr["ctx_hat"][t][None], sd["fc.weight"], skip, 0,
                                               torch.float32)
            assert int(ks[0]) == k
            _close("lrp weights, word %d%s" % (t, " (skipped)" if skip_ids else ""), torch.stack([wc_[0], wh_[0]]), torch.stack([w_ctx, w_h]))
            _close("re-weighted fc input", hcw[0], tr["ctx_hat"][t] * w_ctx + w_h * tr["h2"][t + 1])


@pytest.mark.parametrize("grad", [False, True])
def test_aoa_fwd_restated_vs_oracle(grad):
    O = _O()
    sd = _sd(weights.make_aoa_state(seed=3, vocab_size=V, feat_dim=64, with_encoder=False))
    rs = np.random.RandomState(12)
    F_pix = torch.from_numpy(np.maximum(rs.standard_normal((5, 64)), 0).astype(np.float32))
    cap = weights.make_captions(6, 1, T, V)[0]
    tr = O.aoa_trace(sd, F_pix, cap, grad=grad)
    enc = dict(glob=tr["glob"][None], key=tr["key"][None], value=tr["value"][None])
    out = F.aoa_fwd(sd, enc, torch.from_numpy(cap)[None], 8, torch.float32, "torch", grad)
    for mine, ref in (("h", "h"), ("c", "c"), ("g", "g"), ("i", "i"), ("f", "f"), ("o", "o"), ("ctx", "ctx"), ("c_aoa", "c_aoa"), ("lin", "c_aoa_lin"),
                      ("gate", "c_aoa_gate"), ("alpha", "alpha")):
        _close("AoA " + mine, out[mine][0], tr[ref])
    _close("AoA x", out["xh"][0][:, :F.E + F.H], tr["x"])
    assert torch.equal(out["xh"][0][:, F.E + F.H:], out["h"][0][:-1])
    _close("AoA pred", out["hc"][0] @ sd["fc.weight"].t() + sd["fc.bias"], tr["pred"])
    assert torch.equal(out["sg"], torch.sigmoid(out["gate"]))


@pytest.mark.parametrize("which", ["small", "long"])
def test_adaatt_fwd_restated_vs_the_reference_run(which):
    with np.load(os.path.join(GOLDEN, "adaatt.npz"), allow_pickle=False) as f:
        g = {k: f[k] for k in f.files}
    P, CH = 12, 192
    sd = _sd(weights.make_adaatt_state(seed=int(g["seed"]), vocab_size=int(g["V"]), feat_dim=CH, num_pixels=P, encoder=None))
    n = 1 if which == "long" else 2
    feats = torch.from_numpy(weights.make_bu_features(int(g["feat_seed"]) + (which == "long"), n, P, CH))          # (B, P, C)
    caps = torch.from_numpy(g[which + "_caption"])
    Vp = torch.relu(feats @ sd["img_projector.weight"].reshape(F.H, CH).t() + sd["img_projector.bias"])          # adaptiveattention.py:584
    glob = torch.relu(feats.mean(1) @ sd["global_img_feature_proj.weight"].t() + sd["global_img_feature_proj.bias"])          # :585
    att_img = Vp @ sd["AdaAttention.W_v_proj.weight"].t() + sd["AdaAttention.W_v_proj.bias"]
    out = F.adaatt_fwd(sd, dict(glob=glob, Vp=Vp, att_img=att_img), caps, torch.float32, "torch")
    sel = (lambda x: x[0]) if which == "long" else (lambda x: x)
    pairs = dict(ht="h", ct="c", gt="g", it_act="i", ft_act="f", st="s", context="ctx", context_hat="ctx_hat", alphas="alpha", betas="beta")
    for ref, mine in pairs.items():
        _close("AdaAtt %s %s" % (which, mine), sel(out[mine]), torch.from_numpy(g["%s_tr_%s" % (which, ref)]))
    pred = out["hc"] @ sd["fc.weight"][::97].t() + sd["fc.bias"][::97]
    _close("AdaAtt %s predictions" % which, sel(pred), torch.from_numpy(g[which + "_tr_predictions"]))


def test_building_blocks_restated():
    gen = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(5, 260, generator=gen), torch.randn(7, 260, generator=gen), torch.randn(7, generator=gen)
    want = torch.nn.functional.linear(x.double(), w.double(), b.double())
    for o in F.ORDERS:
        assert rel_err(F.linear(x, w, b, 0, torch.float64, o), want) < 1e-14
        assert rel_err(F.linear(x, w, b, 1, torch.float64, o), torch.relu(want)) < 1e-14
        assert rel_err(F.mean_pixels(x.view(1, 5, 260), torch.float64, o), x.double().mean(0, keepdim=True)) < 1e-14
    lp = torch.log_softmax(x.double(), -1)
    idx, val = F.argmax_logprob(x, torch.float64, "rev128")
    assert torch.equal(idx, x.argmax(-1)) and rel_err(val, lp.max(-1).values) < 1e-14
    tie = torch.tensor([[1.0, 0.0, 1.0], [2.0, 2.0, 2.0], [float("-inf"), 0.5, 3.0]])
    assert F.argmax_logprob(tie, torch.float64, "torch")[0].tolist() == [0, 0, 2]


# ---- (2) the drawn cases -------------------------------------------------------------------------------------------------------------------
CASES = sorted(set(F.all_cases()))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_drawn_cases_meet_the_yardstick(case):
    model, P, variant, B, T_, model_bias, gate_h_new, zero_state = case
    ref64, refs32 = F.references(*case)
    assert not any(torch.isnan(v).any() or torch.isinf(v).any() for v in ref64.values())
    live = torch.ones(B, dtype=torch.bool)
    print("%s: max|.| %s" % (case, ", ".join("%s %.1e" % (k, float(v.abs().max())) for k, v in ref64.items())))
    _yardstick(str(case), refs32, ref64, live)
    if B == max(F.B_SWEEP):          # the kernel tests also grade the first 1, 17, .. images of this draw alone
        for b in F.B_SWEEP[:-1]:
            _yardstick("%s, the first %d images" % (case, b), refs32, ref64, torch.arange(B) < b)
    assert F.references(*case)[0] is ref64          # (cached: the kernel tests grade against these very tensors)
    # the draw is what it is described as
    if model == "aoa":
        sc = ref64["scores"].abs().amax(dim=(0, 1, 3))          # per head
        print("AoA scaled scores, max |.| per head: %s" % ", ".join("%.1f" % v for v in sc.tolist()))
        k = 2.0 if variant == "over" else 1.0          # (model bias moves h, and with it the queries, a little: 20 %)
        assert 32 * k < sc[0] < 48 * k and sc[4] > 89 and sc[7] < 0.01
        assert (ref64["ctx"][0] > 0).all() and (ref64["ctx"][1:] < 0).all()          # the negated value rows
    else:
        zsc = ref64["zsc"]
        pix, sen = zsc[..., :-1], zsc[..., -1]
        print("pixel scores %.1f .. %.1f, sentinel %.1f .. %.1f" % (float(pix.min()), float(pix.max()), float(sen.min()), float(sen.max())))
        if variant == "over":
            assert pix.max() > 89 and pix.min() < -89
            assert not torch.isfinite(torch.exp(pix.float()).sum(-1)).all()          # without the max subtraction: inf
        else:
            assert 30 < pix.max() < 44 and -44 < pix.min() < -30
            if variant == "hi":
                assert (sen[:, :, None] > pix).all() and (ref64["beta"] > 0.9).all()
            else:
                assert (sen[:, :, None] < pix).all() and (ref64["beta"] < 1e-3).all()
    gates = {"gridtd": ("i1", "f1", "o1", "sgate", "i2", "f2", "o2"), "aoa": ("i", "f", "o", "sg"), "adaatt": ("i", "f", "o", "sgate")}[model]
    for k in gates:          # every sigmoid gate holds an exact 1, a 0 (below 1e-30: sigmoid(-100) is a denormal) and an exact 0.5
        g32 = refs32[0][k]
        assert (g32 == 1).any() and (g32 < 1e-30).any() and (g32 == 0.5).any(), k
    for k in ("g1", "g2") if model == "gridtd" else ("g",):
        assert (ref64[k] == 0).any() and (ref64[k] > 45).any() and (ref64[k] < -45).any(), k
