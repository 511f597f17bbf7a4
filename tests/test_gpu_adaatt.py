"""The single-LSTM adaptive-attention model explained (`AdaAttEngine`, explainers/adaatt.py; csrc/lrpx_adaatt.hip) against
tests/golden/adaatt.npz / adaatt_maps.npz: the reference's `AdaptiveAttentionCaptioningModel` and `ExplainAdaptiveAttention`
(tests/golden/make_golden_adaatt.py).  The relevance kernels are also held alone, against an fp64 restatement of
models/adaptiveattention.py:679-771 kept in this file.  Every deviation is printed before it is asserted."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN, assert_close_modulo_pool_ties, rel_err
from fp64_anchor import fp32_grade

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

PAIRS = dict(ht="h", ct="c", gt="g", it_act="i", ft_act="f", st="s", context="ctx", context_hat="ctx_hat", alphas="alpha", betas="beta")
P, CH, H, E = 12, 192, 512, 512
W = H + 2 * E


def _load(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _stab(z):
    zt = z + 0.01 * torch.sign(z)
    return torch.where(zt == 0, torch.full_like(zt, 0.01), zt)


def _features(g, which):
    from lrp_amd import weights
    n = 1 if which == "long" else 2
    return torch.from_numpy(weights.make_bu_features(int(g["feat_seed"]) + (which == "long"), n, P, CH))


def _explain(eng, feats, caps, lens=None):
    """`explain_features` in its parts, keeping what the tests read: r_feat (B,T,P,C), r_words (B,T,T), predictions, the trace, r_glob
    (B,T,E) and r_proj (B,T,P,H) = the reference's `r_img_feature_proj` (the pixel rule's a_proj times z~(proj_nb))"""
    enc = eng.encode(features=feats)
    caps = caps.to(eng.device)
    B, T = caps.shape[0], caps.shape[1] - 1
    tr = eng.trace(enc, caps, predictions=True)
    r_feat, r_words, _ = eng.relevance(enc, tr, lens)
    torch.cuda.synchronize()
    rs = eng.last_rel
    out = types.SimpleNamespace(r_feat=r_feat.view(B, T, P, CH).clone(), r_words=r_words.view(B, T, T).clone(), pred=tr["pred"].clone(),
                                tr={k: v.clone() for k, v in tr.items() if torch.is_tensor(v)}, r_glob=rs["r_glob"].view(B, T, E).clone())
    out.r_proj = (rs["a_proj"].view(B, T, P, H) * _stab(enc["proj_nb"])[:, None]).clone() if lens is None else None
    return out


@pytest.fixture(scope="module")
def fx():
    """the fixture, the engine on its features-only state, and ONE explained `small` batch shared by the tests (clones)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import weights
    from lrp_amd.explainers.adaatt import AdaAttEngine
    g = _load("adaatt.npz")
    V = int(g["V"])
    eng = AdaAttEngine(weights.make_adaatt_state(seed=int(g["seed"]), vocab_size=V, feat_dim=CH, num_pixels=P, encoder=None))
    feats, caps = _features(g, "small"), torch.from_numpy(g["small_caption"])
    return types.SimpleNamespace(g=g, V=V, eng=eng, feats=feats, caps=caps, run=_explain(eng, feats, caps))


@pytest.fixture(scope="module")
def small():
    """a V = 503 engine for the kernel tests and the tests that compare the engine with itself"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import weights
    from lrp_amd.explainers.adaatt import AdaAttEngine
    return AdaAttEngine(weights.make_adaatt_state(seed=5, vocab_size=503, feat_dim=CH, num_pixels=P, encoder=None))


@pytest.fixture(scope="module")
def vgg():
    """the engine with the VGG16 encoder and ONE accumulate=True run on the fixture's image"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import weights
    from lrp_amd.explainers.adaatt import AdaAttEngine
    g = _load("adaatt.npz")
    sd = weights.make_adaatt_state(seed=int(g["seed"]), vocab_size=int(g["V"]))
    eng = AdaAttEngine(sd)
    img, cap = torch.from_numpy(weights.make_images(int(g["seed"]), 1)), torch.from_numpy(g["vgg_caption"]).view(1, -1)
    maps, r_words, pred, r_feat, tr, enc = eng.explain_batch(img, cap, accumulate=True, return_features=True, predictions=True)
    torch.cuda.synchronize()
    return types.SimpleNamespace(g=g, sd=sd, eng=eng, img=img, cap=cap, maps=maps.cpu(), r_words=r_words.cpu(), pred=pred.cpu(), r_feat=r_feat.cpu(),
                                 tr={k: v.clone() for k, v in tr.items() if torch.is_tensor(v)}, wm=weights.make_word_map(int(g["V"])))


def _small_inputs(k, B=2, T=3):
    from lrp_amd import weights
    return (torch.from_numpy(weights.make_bu_features(10 + k, B, P, CH)).cuda(), torch.from_numpy(weights.make_captions(20 + k, B, T, 503)).cuda())


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------------------
def _restate(d, lens, dtype):
    """models/adaptiveattention.py:679-763 up to the projector rule, row by row, in `dtype` on the CPU, from trace tensors `d` (any values).
    Returns r_h[0], r_c[0], r_ctx = r_context / z~(ctx), r_glob, r_words (not normalised), a_proj - zeros in rows behind an image's
    last word."""
    t_ = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d.items()}
    B, T = t_["beta"].shape
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    out = dict(r_h=z(B * T, H), r_c=z(B * T, H), r_ctx=z(B * T, H), r_glob=z(B * T, E), r_words=z(B * T, T), a_proj=z(B * T, P, H))
    for b in range(B):
        for t in range(T if lens is None else lens[b]):
            row = b * T + t
            hc, ch, cx, beta, lg = t_["hc"][b, t], t_["ctx_hat"][b, t], t_["ctx"][b, t], t_["beta"][b, t], t_["logit"][row]
            r_hc = t_["fcw"][t_["tok"][b, t + 1]] * hc / _stab(lg) * lg                               # :700-703
            r_h = t_["h"][b, t + 1] / _stab(hc) * r_hc                                                # :705-708
            r_ch = ch / _stab(hc) * r_hc                                                              # :710-713
            r_cx = (1 - beta) * cx / _stab(ch) * r_ch                                                 # :714-717
            r_c = beta * t_["s"][b, t] / _stab(ch) * r_ch                                             # :719-724
            out["r_ctx"][row] = r_cx / _stab(cx)
            for i in range(t, -1, -1):
                rc = r_c + r_h                                                                        # :726
                tg, cn = torch.tanh(t_["g"][b, i]), t_["c"][b, i + 1]
                r_g = t_["i"][b, i] * tg / _stab(cn) * rc                                             # :727-730
                r_c = t_["f"][b, i] * t_["c"][b, i] / _stab(cn) * rc                                  # :731-734
                rx = t_["xh"][b, i] * ((r_g / _stab(tg)) @ t_["wg"])                                  # :735-738, columns [h | emb | glob]
                r_h = rx[:H]                                                                          # :739
                if i == t:
                    out["r_glob"][row] = rx[H + E:]                                                   # :740-741
                out["r_words"][row, i] = rx[H:H + E].sum()                                            # :742, :764
            out["r_h"][row], out["r_c"][row] = r_h, r_c
            out["a_proj"][row] = t_["Vp"][b] * t_["alpha"][b, t][:, None] * out["r_ctx"][row][None] / _stab(t_["proj_nb"][b])   # :756-763
    return out


@pytest.mark.parametrize("T, lens", [(3, None), (3, [2, 0]), (3, [3, 2]), (26, None), (26, [26, 5])],
                         ids=["T3", "T3_lens20", "T3_lens32", "T26", "T26_lens"])
def test_relevance_kernels_alone_vs_fp64(small, T, lens):
    """rel_init, the lock-steps (gate rule + point-wise launch) and the pixel rule on a trace of drawn values, B = 2: with and without
    `lens`, with and without a row list, with and without the dead columns; outputs pre-filled with NaN"""
    from lrp_amd import _lib, ops
    from lrp_amd._lib import AdaRelState, EPI_REL, check, ptr, stream_ptr
    lib, eng, B, dev = _lib.load(), small, 2, "cuda"
    gen = torch.Generator(device="cpu").manual_seed(300 + T)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    rows = B * T
    sd = eng.sd
    d = dict(xh=rnd(B, T, W), h=0.5 * rnd(B, T + 1, H), c=rnd(B, T + 1, H), g=rnd(B, T, H), i=torch.sigmoid(rnd(B, T, H)),
             f=torch.sigmoid(rnd(B, T, H)), s=0.5 * rnd(B, T, H), ctx=torch.relu(rnd(B, T, H)), alpha=torch.softmax(rnd(B, T, P), -1),
             beta=torch.sigmoid(rnd(B, T)), logit=rnd(rows), fcw=sd["fc.weight"].cpu(), tok=torch.randint(1, 500, (B, T + 1), generator=gen),
             proj_nb=rnd(B, P, H))
    d["ctx"][:, :, 7] = 0                                                                            # z~(0) = eps
    d["ctx_hat"] = d["beta"][..., None] * d["s"] + (1 - d["beta"][..., None]) * d["ctx"]
    d["hc"] = d["h"][:, 1:] + d["ctx_hat"]
    d["Vp"] = torch.relu(d["proj_nb"] + 0.1)
    a = "AdaLSTM.lstm_cell."
    d["wg"] = torch.cat([sd[a + "weight_hh"][2 * H:3 * H], sd[a + "weight_ih"][2 * H:3 * H]], 1).cpu()
    ref64, ref32 = _restate(d, lens, torch.float64), _restate(d, lens, torch.float32)

    tr = eng._alloc_trace(B, T)
    for k in ("xh", "h", "c", "g", "i", "f", "s", "ctx", "ctx_hat", "hc", "alpha", "beta"):
        tr[k].copy_(d[k])
    logit, tok, Vp, proj_nb = d["logit"].to(dev), d["tok"].to(dev), d["Vp"].to(dev), d["proj_nb"].to(dev)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
    idx, _, _ = eng._row_index(B, T)
    active = [b * T + t for b in range(B) for t in range(T) if lens is None or t < lens[b]]

    def run(cut):
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        rs = dict(r_h=nan(rows, H), r_c=nan(rows, H), r_ctx=nan(rows, H), r_glob=nan(rows, E), A=nan(rows, H), rx=nan(rows, W), r_words=nan(rows, T))
        c = AdaRelState()
        c.lens = ptr(lens_t)
        for k, v in rs.items():
            setattr(c, k, ptr(v))
        ctr, crs = C.byref(tr["_c"]), C.byref(c)
        check(lib.lrpx_adaatt_rel_init(ctr, crs, ptr(sd["fc.weight"]), ptr(logit), ptr(tok), T + 1, stream_ptr()))
        dd = ops.conv_desc(rs["A"], eng.p_wg, rows, 0, H, W, 1, EPI_REL, pix_per_map=1, oc_split=W, x=tr["xh"], map2img=idx[0], out0=rs["rx"])
        check(lib.lrpx_adaatt_rel_steps(ctr, crs, T, C.byref(dd), ptr(idx), idx.shape[1], cut, stream_ptr()))
        full = nan(rows, P, H)
        check(lib.lrpx_adaatt_rel_pix_rows(ctr, crs, ptr(Vp), ptr(proj_nb), ptr(full), None, rows, stream_ptr()))
        rs["a_proj"] = full
        if active:
            rl = torch.tensor(active, dtype=torch.int32, device=dev)
            rs["a_proj_rows"] = nan(len(active), P, H)
            check(lib.lrpx_adaatt_rel_pix_rows(ctr, crs, ptr(Vp), ptr(proj_nb), ptr(rs["a_proj_rows"]), ptr(rl), len(active), stream_ptr()))
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in rs.items()}

    got, wide = run(1), run(0)
    live = torch.zeros(rows, dtype=torch.bool)
    live[active] = True
    # exact zeros: A after the last lock-step, inactive rows, behind word t
    assert torch.count_nonzero(got["A"]) == 0 and not torch.isnan(got["A"]).any()
    for k in ("r_ctx", "r_glob", "r_words", "a_proj"):
        assert torch.count_nonzero(got[k][~live]) == 0 and not torch.isnan(got[k]).any(), k
    for row in active:
        assert torch.count_nonzero(got["r_words"][row, row % T + 1:]) == 0
    if active:
        assert torch.equal(got["a_proj_rows"], got["a_proj"][live])
    # the dead columns: every live output bit for bit
    for k in ("r_h", "r_c", "r_ctx", "r_glob", "r_words", "A", "a_proj"):
        assert torch.equal(got[k][live], wide[k][live]), "cut_dead_columns changes " + k
    if not active:
        return
    for k in ("r_ctx", "a_proj", "r_glob", "r_words", "r_h", "r_c"):
        fp32_grade(got[k][live], ref64[k][live], ref32[k][live], ref32[k][live], "T %d lens %s %s" % (T, lens, k), margin_min=0)


# ---- 2. the trace against the reference ----------------------------------------------------------------------------------------------------
def _trace_errs(tr, pred, g, prefix, b=None):
    sel = (lambda v: v) if b is None else (lambda v: v[b])
    errs = {ref: rel_err(sel(tr[mine].cpu()), g[prefix + "_tr_" + ref]) for ref, mine in PAIRS.items()}
    errs["predictions"] = rel_err(sel(pred.cpu())[..., ::97], g[prefix + "_tr_predictions"])
    return errs


@pytest.mark.parametrize("decoupled", [True, False], ids=["decoupled", "per_step"])
def test_trace_vs_reference(fx, vgg, decoupled):
    cases = [("small", fx.eng, fx.eng.encode(features=fx.feats), fx.caps, None),
             ("long", fx.eng, fx.eng.encode(features=_features(fx.g, "long")), torch.from_numpy(fx.g["long_caption"]), 0),
             ("vgg", vgg.eng, vgg.eng.encode(vgg.img), vgg.cap, 0)]
    for name, eng, enc, caps, b in cases:
        eng.decoupled = decoupled
        try:
            tr = eng.trace(enc, caps, predictions=True)
        finally:
            eng.decoupled = True
        torch.cuda.synchronize()
        errs = _trace_errs(tr, tr["pred"], fx.g, name, b)
        print("%s trace, %s: deviations (of the maximum): %s" % (name, "decoupled" if decoupled else "per step",
                                                                 ", ".join("%s %.2e" % kv for kv in errs.items())))
        for k, e in errs.items():
            assert e < 1e-4, (name, k, e)
        assert torch.equal(tr["xh"][:, :, :H], tr["h"][:, :-1])          # the h columns of the input rows


# ---- 3. relevance against the reference ------------------------------------------------------------------------------------------------------
def _words_row(what, got, ref32, ref64):
    """r_words of one row: 1e-5 of the reference's fp32 row; a row of a LONG caption between 1e-5 and the fp64-anchored criterion of
    tests/test_gpu_t20.py (|got - fp64| <= 3 max(|ref32 - fp64|, 1e-5)) is held to that criterion instead"""
    d = float(np.abs(got - ref32).max())
    noise, e64 = float(np.abs(ref32.astype(np.float64) - ref64).max()), float(np.abs(got.astype(np.float64) - ref64).max())
    print("%s: r_words %.2e of the fp32 reference (fp64: %.2e; the reference's own fp32 from fp64 %.2e)" % (what, d, e64, noise))
    return d, e64, noise


def _check_rows(what, run, g, prefix, rows, long=False):
    """SURVEY §8(d)'s bounds: r_feat (and r_glob, r_proj) within 1e-4 of each map's maximum, r_words within 1e-5, zero behind word t"""
    for (b, t, w) in rows:
        e = {k: rel_err(getattr(run, k)[b, t].cpu(), g[prefix + "_" + k][w]) for k in ("r_feat", "r_glob", "r_proj") if getattr(run, k, None) is not None}
        print("%s image %d word %d: of the maximum: %s" % (what, b, t, ", ".join("%s %.2e" % kv for kv in e.items())))
        d, e64, noise = _words_row("%s image %d word %d" % (what, b, t), run.r_words[b, t, :t + 1].cpu().numpy(), g[prefix + "_r_words"][w][:t + 1],
                                   g[prefix + "_r_words64"][w][:t + 1])
        for k, v in e.items():
            assert v < 1e-4, (what, k, b, t, v)
        if long and d >= 1e-5:
            assert e64 <= 3.0 * max(noise, 1e-5), (what, b, t, "vs fp64", e64, noise)
        else:
            assert d < 1e-5, (what, b, t, d)
        assert torch.count_nonzero(run.r_words[b, t, t + 1:]) == 0


def test_relevance_small_vs_reference(fx):
    assert fx.eng.cnn is None and (fx.eng.P, fx.eng.C, fx.eng.H) == (P, CH, H)
    _check_rows("small", fx.run, fx.g, "small", [(b, t, (b, t)) for b in range(2) for t in range(3)])
    r_feat, r_words = fx.eng.explain_features(fx.feats, fx.caps)
    torch.cuda.synchronize()
    assert torch.equal(r_feat, fx.run.r_feat) and torch.equal(r_words, fx.run.r_words)


def test_relevance_long_caption_vs_reference(fx):
    g = fx.g
    run = _explain(fx.eng, _features(g, "long"), torch.from_numpy(g["long_caption"]))
    assert run.r_feat.shape == (1, 26, P, CH)
    _check_rows("long", run, g, "long", [(0, int(t), i) for i, t in enumerate(g["long_words"])], long=True)


def test_relevance_vgg_vs_reference(vgg):
    g = vgg.g
    assert vgg.r_feat.shape == (1, 3, 196, 512) and vgg.eng.vgg is not None
    for t in range(3):
        e = rel_err(vgg.r_feat[0, t][:, ::4], g["vgg_r_feat"][t])
        print("vgg word %d: r_feat %.2e of the maximum (every 4th channel)" % (t, e))
        d, _, _ = _words_row("vgg word %d" % t, vgg.r_words[0, t, :t + 1].numpy(), g["vgg_r_words"][t][:t + 1], g["vgg_r_words64"][t][:t + 1])
        assert e < 1e-4 and d < 1e-5, (t, e, d)
        assert torch.count_nonzero(vgg.r_words[0, t, t + 1:]) == 0


# ---- 4. the maps end to end --------------------------------------------------------------------------------------------------------------------
def test_maps_end_to_end_vs_reference(vgg):
    """whole pipeline on the GPU, the reference's running sums; compared modulo max-pool tie flips with the bounds of the test of the
    same name in tests/test_gpu_gridtd.py (conftest.OBSERVED: the encoder and the chain are the same)"""
    gm = _load("adaatt_maps.npz")
    assert int(gm["seed"]) == int(vgg.g["seed"])
    for t in range(3):
        assert_close_modulo_pool_ties(vgg.maps[0, t][None, :, ::4, ::4], gm["vgg_map_sub4_%d" % t], what=t)
    assert_close_modulo_pool_ties(vgg.maps[0, 2], gm["vgg_map_full_2"][0], what="full")


def test_explainer_class_drop_in(vgg):
    """`ExplainAdaptiveAttention(args, word_map, model).explain_caption(img)` returns what the reference's class returns"""
    from lrp_amd.explainers import ExplainAdaptiveAttention
    g, gm = vgg.g, _load("adaatt_maps.npz")
    args = types.SimpleNamespace(embed_dim=512, hidden_dim=512, encoder='vgg16', weight='', save_path='', dataset='synthetic', height=224, width=224)
    ex = ExplainAdaptiveAttention(args, vgg.wm, model={k: torch.from_numpy(v) for k, v in vgg.sd.items()})
    maps, rws = ex.explain_caption(vgg.img, caption_encode=g["vgg_caption"].tolist())
    torch.cuda.synchronize()
    assert len(maps) == 3 and len(rws) == 3 and ex.caption_length == 3 and ex.beam_caption_encode == g["vgg_caption"].tolist()
    for t in range(3):
        assert maps[t].shape == (1, 3, 224, 224) and rws[t].shape == (t + 1,)
        assert_close_modulo_pool_ties(maps[t].cpu()[:, :, ::4, ::4], gm["vgg_map_sub4_%d" % t], what=t)
        d = np.abs(rws[t].cpu().numpy() - g["vgg_r_words"][t][:t + 1]).max()
        print("drop-in word %d: r_words %.2e" % (t, d))
        assert d < 1e-5
    assert rel_err(ex.predictions.cpu()[:, ::97], g["vgg_tr_predictions"]) < 1e-4
    assert rel_err(ex.alphas.cpu(), g["vgg_tr_alphas"]) < 1e-4 and rel_err(ex.betas.cpu(), g["vgg_tr_betas"]) < 1e-4
    rf, rw = ex.explain_caption_wordt(1)
    assert rf.shape == (1, 512, 14, 14) and rel_err(rf.cpu()[0].reshape(512, 196).t()[:, ::4], g["vgg_r_feat"][1]) < 1e-4
    # without a caption: the reference's own procedure, beam_search(beam_size=3, max_cap_length=20)
    ex.get_hidden_parameters(vgg.img)
    assert ex.beam_caption_encode[1:] == g["decode_beam"].tolist()
    tf = ex.teacherforce_forward(vgg.img, g["vgg_caption"].tolist()[:-1])
    assert rel_err(tf.cpu()[:, ::97], g["vgg_tr_predictions"]) < 1e-4


# ---- 5. the engine against itself ------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    torch.cuda.synchronize()
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert not torch.isnan(a).any(), (what, i)
        assert torch.equal(a, b), "%s, output %d: %d of %d elements differ, largest difference %.3g" % (
            what, i, int((a != b).sum()), a.numel(), float((a.double() - b.double()).abs().max()))


def _clones(out):
    return tuple(t.clone() for t in out)


@pytest.mark.parametrize("B", [17, 65])
def test_batch_independence(small, B):
    """one image alone equals the same image inside a batch of 17 (17 crosses the 16-row tile of the gate GEMM) and of 65 (the recurrence
    and the skinny linears run in slices of 64 images), in both trace paths"""
    feats, caps = _small_inputs(3, B=B)
    for decoupled in (True, False):
        small.decoupled = decoupled
        try:
            many = _clones(small.explain_features(feats, caps, predictions=True))
            for b in (0, B - 1):
                one = small.explain_features(feats[b:b + 1], caps[b:b + 1], predictions=True)
                _same(one, tuple(t[b:b + 1] for t in many), "image %d alone, decoupled %s" % (b, decoupled))
        finally:
            small.decoupled = True


def test_unequal_caption_lengths(small):
    feats, caps = _small_inputs(4)
    full = _clones(small.explain_features(feats, caps))
    for lens in ([3, 2], [2, 0]):
        r_feat, r_words = small.explain_features(feats, caps, lens=lens)
        torch.cuda.synchronize()
        for b in range(2):
            assert torch.equal(r_feat[b, :lens[b]], full[0][b, :lens[b]]) and torch.equal(r_words[b, :lens[b]], full[1][b, :lens[b]]), (lens, b)
            assert torch.count_nonzero(r_feat[b, lens[b]:]) == 0 and torch.count_nonzero(r_words[b, lens[b]:]) == 0
    r_feat, r_words = small.explain_features(feats, caps, lens=[0, 0])
    assert r_feat.shape == (2, 3, P, CH) and torch.count_nonzero(r_feat) == 0 and torch.count_nonzero(r_words) == 0


def test_stream_and_replica_match_serial(small):
    batches = [_small_inputs(k) + (([3, 2],) if k == 1 else ()) for k in range(3)]
    rep = small.replica()
    assert rep.cnn is None and rep.sd is small.sd and rep._idx_cache is not small._idx_cache
    serial = [_clones((rep if i % 2 else small).explain_features(b[0], b[1], lens=b[2] if len(b) > 2 else None)) for i, b in enumerate(batches)]
    got = [_clones(o) for o in small.explain_stream(batches, depth=2)]
    assert len(got) == 3 and len(small._replicas) == 2
    for k in range(3):
        _same(got[k], serial[k], "batch %d" % k)


@pytest.mark.parametrize("entry", ["explain_batch_graph", "explain_batch_replay"])
def test_static_steps_are_bit_identical_to_the_eager_step(small, entry):
    """call 0 captures / records, calls 1 and 2 replay on new features and captions"""
    outs = []
    for k in range(3):
        feats, caps = _small_inputs(5 + k)
        got = _clones(getattr(small, entry)(feats, caps, predictions=True))
        assert len(got) == 3          # r_feat, r_words, predictions
        _same(got, small.explain_features(feats, caps, predictions=True), "%s, call %d" % (entry, k))
        outs.append(got)
    assert not torch.equal(outs[0][0], outs[1][0])          # (the inputs really differed)
    assert len(small._graphs if entry.endswith("graph") else small._recordings) == 1


def test_static_steps_with_the_vgg16_encoder(vgg):
    from lrp_amd import weights
    for entry in ("explain_batch_graph", "explain_batch_replay"):
        for k in range(2):
            img, cap = torch.from_numpy(weights.make_images(40 + k, 1)).cuda(), torch.from_numpy(weights.make_captions(50 + k, 1, 3, int(vgg.g["V"]))).cuda()
            got = _clones(getattr(vgg.eng, entry)(img, cap))
            _same(got, vgg.eng.explain_batch(img, cap), "%s with VGG16, call %d" % (entry, k))


# ---- 6. the model's own decoding loops -----------------------------------------------------------------------------------------------------
def test_decode_loops_vs_reference(vgg):
    from lrp_amd.explainers.beam import caption_from_sequence
    g, eng, wm = vgg.g, vgg.eng, vgg.wm
    start, end = wm['<start>'], wm['<end>']
    enc = eng.encode(vgg.img)
    toks = eng.greedy(enc, g["decode_greedy"].shape[1], start, end)
    assert toks.cpu().tolist() == g["decode_greedy"].tolist()
    seq = eng.beam_search(enc, int(g["decode_beam_size"]), int(g["decode_beam_steps"]), start, end)
    assert caption_from_sequence(seq, wm)[1:] == g["decode_beam"].tolist()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_fire_before_any_launch(small, monkeypatch):
    from lrp_amd import _lib, weights
    from lrp_amd.explainers.adaatt import AdaAttEngine
    feats, caps = _small_inputs(0)
    enc = small.encode(features=feats)

    def boom(*a, **k):
        raise AssertionError("a library call before the refusal")
    monkeypatch.setattr(_lib, "load", boom)
    for call in (lambda: small.guided_gradient(enc, None), lambda: small.explain_batch_guided(feats, caps),
                 lambda: small.explain_batch_gradient(feats, caps), lambda: small.trace(enc, caps, grad=True)):
        with pytest.raises(NotImplementedError, match="follow-up"):
            call()
    for call in (lambda: small.sample_lrp(enc, 8, 1, 2, []), lambda: small.forwardlrp_context(enc, caps, [3, 3], [])):
        with pytest.raises(NotImplementedError, match="no sample_lrp / forwardlrp_context"):
            call()
    for bad in (feats[:, :11], feats[:, :, :191], torch.zeros(2, 196, 512), torch.zeros(2, P)):
        for entry in (lambda f: small.encode(features=f), lambda f: small.explain_features(f, caps), lambda f: small.explain_batch_graph(f, caps),
                      lambda f: small.explain_batch_replay(f, caps)):
            with pytest.raises(ValueError, match="AdaAttEngine"):
                entry(bad)
    with pytest.raises(ValueError, match="takes \\(B, P, C\\) features"):          # images, but this engine has no encoder
        small.explain_batch(torch.zeros(2, 3, 224, 224), caps)
    with pytest.raises(ValueError, match="gridTD state"):
        AdaAttEngine(weights.make_gridtd_state(seed=1, vocab_size=307))


# ---- 8. a ResNet encoder ---------------------------------------------------------------------------------------------------------------------
def _net(seed, base, blocks):
    """the tiny bottleneck net of tests/test_gpu_gridtd_resnet.py (tests/golden/make_golden_resnet.py: bottleneck_net)"""
    from make_golden_resnet import bottleneck_net
    from lrp_amd.LRPtools import lrp_modules
    return bottleneck_net(np.random.RandomState(seed), lrp_modules.resAdd, base, blocks)


def test_resnet_encoder():
    """45 x 51 images through the tiny bottleneck net (P = 12 = 3 x 4, C = 192): `explain_batch` is the encoder, `explain_features` on its
    features and `ResNetEncoder.relevance`, bit for bit; graph and recording are refused"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import weights
    from lrp_amd.explainers.adaatt import AdaAttEngine
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "resnet_engine.npz"))["x"])
    net = _net(int(np.load(os.path.join(GOLDEN, "gridtd_resnet.npz"))["net_seed"]), 12, [1, 2, 1]).cuda()
    eng = AdaAttEngine(weights.make_adaatt_state(seed=7, vocab_size=503, feat_dim=CH, num_pixels=P, encoder=None), encoder=net)
    assert eng.resnet and eng.vgg is None and eng.cnn.feature_shape(45, 51) == (3, 4, CH)
    caps = torch.from_numpy(weights.make_captions(8, x.shape[0], 3, 503))
    maps, r_words, r_feat, tr, enc = eng.explain_batch(x, caps, return_features=True)
    maps, r_words, r_feat, feats = maps.clone(), r_words.clone(), r_feat.clone(), enc["feats"].clone()
    assert maps.shape == (x.shape[0], 3, 3, 45, 51)
    rf2, rw2 = eng.explain_features(feats, caps)
    torch.cuda.synchronize()
    assert torch.equal(rf2, r_feat) and torch.equal(rw2, r_words)
    eng.cnn.forward(x.cuda())
    B, T = caps.shape[0], 3
    row2img = torch.arange(B, device="cuda", dtype=torch.int32).repeat_interleave(T)
    again = eng.cnn.relevance(r_feat.view(B * T, P, CH).contiguous(), row2img)
    torch.cuda.synchronize()
    assert torch.equal(again.view_as(maps), maps)
    for entry in (eng.explain_batch_graph, eng.explain_batch_replay):
        with pytest.raises(NotImplementedError, match="ResNet"):
            entry(x, caps)
    with pytest.raises(ValueError, match="AdaAttEngine"):
        eng.explain_batch(torch.zeros(2, 3, 64, 64), caps)
