"""The gradient family of the single-LSTM adaptive-attention model (`AdaAttGradEngine`, explainers/adaatt_grad.py;
csrc/lrpx_adaatt_grad.hip) against tests/golden/adaatt_grad*.npz: the reference's `ExplainAdaptiveGradient`,
`ExplainiAdaptiveGuidedGradient` and `ExplainAdaptiveGradCam` (tests/golden/make_golden_adaatt_grad.py).  The kernels are also held
alone, against an fp64 restatement of models/adaptiveattention.py:965-1021 kept in this file - unfolded: the products with W_ih stay in
the time loop and the projector product stays in the pixel loop, as the reference has them.  Every deviation is printed before it is
asserted."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN, assert_close_modulo_pool_ties, forward_flips, gradient_e2e_bounds, rel_err
from fp64_anchor import fp32_grade

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

P, CH, H, E = 12, 192, 512, 512


def _load(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _features(g, which):
    from lrp_amd import weights
    n = 1 if which == "long" else 2
    return torch.from_numpy(weights.make_bu_features(int(g["feat_seed"]) + (which == "long"), n, P, CH))


def _small_inputs(k, B=2, T=3):
    from lrp_amd import weights
    return (torch.from_numpy(weights.make_bu_features(10 + k, B, P, CH)).cuda(), torch.from_numpy(weights.make_captions(20 + k, B, T, 503)).cuda())


@pytest.fixture(scope="module")
def fx():
    """the fixture and the engine on its features-only state"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import weights
    from lrp_amd.explainers import AdaAttGradEngine
    g = _load("adaatt_grad.npz")
    eng = AdaAttGradEngine(weights.make_adaatt_state(seed=int(g["seed"]), vocab_size=int(g["V"]), feat_dim=CH, num_pixels=P, encoder=None))
    return types.SimpleNamespace(g=g, eng=eng)


@pytest.fixture(scope="module")
def small():
    """a V = 503 engine for the kernel tests and the tests that compare the engine with itself"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import weights
    from lrp_amd.explainers import AdaAttGradEngine
    return AdaAttGradEngine(weights.make_adaatt_state(seed=5, vocab_size=503, feat_dim=CH, num_pixels=P, encoder=None))


@pytest.fixture(scope="module")
def vgg():
    """the engine with the VGG16 encoder, ONE run of each batch entry on the fixture's image, and the end-to-end bounds of this run's
    forward (conftest.forward_flips / gradient_e2e_bounds)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import weights
    from lrp_amd.explainers import AdaAttGradEngine
    g = _load("adaatt_grad.npz")
    sd = weights.make_adaatt_state(seed=int(g["seed"]), vocab_size=int(g["V"]))
    eng = AdaAttGradEngine(sd)
    img, cap = torch.from_numpy(weights.make_images(int(g["seed"]), 1)), torch.from_numpy(g["vgg_caption"]).view(1, -1)
    maps, r_words, d_feat, tr, enc = eng.explain_batch_gradient(img, cap, return_features=True)
    out = types.SimpleNamespace(g=g, sd=sd, eng=eng, img=img, cap=cap, maps=maps.cpu(), r_words=r_words.cpu(), d_feat=d_feat.cpu(),
                                wm=weights.make_word_map(int(g["V"])))
    gm, gw = eng.explain_batch_guided(img, cap)
    out.guided, out.guided_r_words = gm.cpu(), gw.cpu()
    cams, cw = eng.explain_batch_gradient(img, cap, cam=True)
    out.cams, out.cam_r_words = cams.cpu(), cw.cpu()
    eng.vgg.forward(img.cuda())
    out.e2e = gradient_e2e_bounds(forward_flips(eng.vgg, sd, img), "adaptive-attention gradient family, golden image")
    return out


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------------------
def _restate(d, lens, dtype):
    """models/adaptiveattention.py:965-1021 row by row, unfolded, in `dtype` on the CPU, from trace tensors `d` (any values).  Returns
    d_ctx, gsum = sum_i G_i, d_glob, r_words (normalised, :1016-1019), d_feat - zeros in rows behind an image's last word."""
    t_ = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d.items()}
    B, T = t_["beta"].shape
    Cc = t_["w_proj"].shape[1]
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    out = dict(d_ctx=z(B * T, H), gsum=z(B * T, 4 * H), d_glob=z(B * T, E), r_words=z(B * T, T), d_feat=z(B * T, P, Cc))
    for b in range(B):
        for t in range(T if lens is None else lens[b]):
            row = b * T + t
            d_h = t_["fcw"][t_["tok"][b, t + 1]]                                                      # :987, :992
            d_ctx = d_h * (1 - t_["beta"][b, t])                                                      # :989
            d_c = d_h * t_["beta"][b, t] * t_["sgate"][b, t] * (1 - torch.tanh(t_["c"][b, t + 1]) ** 2)          # :990-991
            d_proj = t_["alpha"][b, t][:, None] * d_ctx[None]                                         # :993-994  (P, H)
            d_glob, gsum, r_w = z(E), z(4 * H), z(T)
            for i in range(t, -1, -1):                                                                # :995-1010
                tc, tg = torch.tanh(t_["c"][b, i + 1]), torch.tanh(t_["g"][b, i])
                ia, fa, oa = t_["i"][b, i], t_["f"][b, i], t_["o"][b, i]
                d_oa = d_h * tc
                d_c = d_c + d_h * oa * (1 - tc ** 2)
                d_fa, d_ia, d_ga = d_c * t_["c"][b, i], d_c * tg, d_c * ia
                G = torch.cat([d_ia * ia * (1 - ia), d_fa * fa * (1 - fa), d_ga * (1 - tg ** 2), d_oa * oa * (1 - oa)])
                d_c = d_c * fa
                d_h = G @ t_["w_hh"]                                                                  # :1007
                d_x = G @ t_["w_ih"]                                                                  # :1008
                d_glob = d_glob + d_x[E:]                                                             # :1009
                r_w[i] = d_x[:E].sum()                                                                # :1010, :1016
                gsum = gsum + G
            d_avg = d_glob @ t_["w_gp"]                                                               # :1011
            out["d_feat"][row] = d_avg[None] / P + d_proj @ t_["w_proj"]                              # :1013-1015, pixel by pixel
            m = r_w.abs().max()
            out["r_words"][row] = r_w / m if m > 0 else r_w                                           # :1017-1019
            out["d_ctx"][row], out["gsum"][row], out["d_glob"][row] = d_ctx, gsum, d_glob
    return out


@pytest.mark.parametrize("B, T, lens", [(2, 3, None), (2, 3, [2, 0]), (2, 3, [3, 2]), (2, 26, None), (2, 26, [26, 5]), (5, 14, None)],
                         ids=["T3", "T3_lens20", "T3_lens32", "T26", "T26_lens", "B5_T14"])
def test_gradient_kernels_alone_vs_fp64(small, B, T, lens):
    """init, the lock-steps, the r_words reduction, the three GEMMs and the spread kernel on a trace of drawn values: with and without
    `lens`, with and without a row list, outputs pre-filled with NaN.  B = 5, T = 14: 70 rows cross the lock-step kernel's row tiles (32 rows;
    and 64, the largest tile `linear_mfma_core` takes)"""
    from lrp_amd import _lib, ops
    from lrp_amd._lib import AdaGradState, EPI_PLAIN, check, ptr, stream_ptr
    lib, eng, dev = _lib.load(), small, "cuda"
    gen = torch.Generator(device="cpu").manual_seed(700 + 10 * T + B)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    rows, sd, a = B * T, eng.sd, "AdaLSTM.lstm_cell."
    d = dict(c=rnd(B, T + 1, H), g=rnd(B, T, H), i=torch.sigmoid(rnd(B, T, H)), f=torch.sigmoid(rnd(B, T, H)), o=torch.sigmoid(rnd(B, T, H)),
             sgate=torch.sigmoid(rnd(B, T, H)), alpha=torch.softmax(rnd(B, T, P), -1), beta=torch.sigmoid(rnd(B, T)),
             tok=torch.randint(1, 500, (B, T + 1), generator=gen), fcw=sd["fc.weight"].cpu(), w_hh=sd[a + "weight_hh"].cpu(),
             w_ih=sd[a + "weight_ih"].cpu(), w_gp=sd["global_img_feature_proj.weight"].cpu(), w_proj=eng.w_proj2d.cpu())
    ref64, ref32 = _restate(d, lens, torch.float64), _restate(d, lens, torch.float32)

    tr = eng._alloc_trace(B, T, True)
    for k in ("c", "g", "i", "f", "o", "sgate", "alpha", "beta"):
        tr[k].copy_(d[k])
    tok = d["tok"].to(dev)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
    active = [b * T + t for b in range(B) for t in range(T) if lens is None or t < lens[b]]
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    gs = dict(d_ctx=nan(rows, H), d_c=nan(rows, H), g0=nan(rows, 4 * H), g1=nan(rows, 4 * H), gsum=nan(rows, 4 * H), wpart=nan(rows, T, H // 16),
              r_words=nan(rows, T))
    c = AdaGradState()
    c.lens = ptr(lens_t)
    for k, v in gs.items():
        setattr(c, k, ptr(v))
    ctr, cgs, st = C.byref(tr["_c"]), C.byref(c), stream_ptr()
    check(lib.lrpx_adaptive_grad_init(ctr, cgs, ptr(sd["fc.weight"]), ptr(tok), T + 1, ptr(eng.wsum), st))
    check(lib.lrpx_adaptive_grad_steps(ctr, cgs, T, ptr(eng.w_hh_t), ptr(eng.wsum), st))
    check(lib.lrpx_rel_words_norm(ptr(gs["r_words"]), rows, T, st))

    def dense(x, wp, n):
        out = nan(rows, n)
        ops.conv_mfma(x, wp, rows, 0, x.shape[1], -(-n // 32) * 32, 1, EPI_PLAIN, pix_per_map=1, oc_split=n, out0=out)
        return out
    gs["d_glob"] = dense(gs["gsum"], eng.p_ih_glob, E)
    d_avg, v1 = dense(gs["d_glob"], eng.p_gp_rel, CH), dense(gs["d_ctx"], eng.p_proj_rel, CH)
    gs["d_feat"] = nan(rows, P, CH)
    check(lib.lrpx_adaptive_grad_pix_rows(ctr, cgs, ptr(v1), ptr(d_avg), ptr(gs["d_feat"]), CH, None, rows, st))
    if active:
        rl = torch.tensor(active, dtype=torch.int32, device=dev)
        gs["d_feat_rows"] = nan(len(active), P, CH)
        check(lib.lrpx_adaptive_grad_pix_rows(ctr, cgs, ptr(v1), ptr(d_avg), ptr(gs["d_feat_rows"]), CH, ptr(rl), len(active), st))
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in gs.items()}
    live = torch.zeros(rows, dtype=torch.bool)
    live[active] = True
    # exact zeros: inactive rows, behind word t
    for k in ("d_ctx", "gsum", "d_glob", "r_words", "d_feat"):
        assert not torch.isnan(got[k]).any(), k
        assert torch.count_nonzero(got[k][~live]) == 0, k
    for row in active:
        assert torch.count_nonzero(got["r_words"][row, row % T + 1:]) == 0
    if not active:
        return
    assert torch.equal(got["d_feat_rows"], got["d_feat"][live])
    for k in ("d_ctx", "gsum", "d_glob", "r_words", "d_feat"):
        fp32_grade(got[k][live], ref64[k][live], ref32[k][live], ref32[k][live], "B %d T %d lens %s %s" % (B, T, lens, k), margin_min=0)


# ---- 2. the decoder gradient against the reference -------------------------------------------------------------------------------------------
def _words_row(what, got, ref32, ref64):
    """r_words of one row: 1e-5 of the reference's fp32 row; a row of a LONG caption between 1e-5 and the fp64-anchored criterion of
    tests/test_gpu_t20.py (|got - fp64| <= 3 max(|ref32 - fp64|, 1e-5)) is held to that criterion instead (tests/test_gpu_adaatt.py)"""
    d = float(np.abs(got - ref32).max())
    noise, e64 = float(np.abs(ref32.astype(np.float64) - ref64).max()), float(np.abs(got.astype(np.float64) - ref64).max())
    print("%s: r_words %.2e of the fp32 reference (fp64: %.2e; the reference's own fp32 from fp64 %.2e)" % (what, d, e64, noise))
    return d, e64, noise


def _decoder(eng, feats, caps, mask_features=True):
    enc = eng.encode(features=feats)
    caps = caps.to(eng.device)
    B, T = caps.shape[0], caps.shape[1] - 1
    tr = eng.trace(enc, caps, predictions=False, grad=True)
    d_feat, r_words, _ = eng.guided_gradient(enc, tr, mask_features=mask_features)
    torch.cuda.synchronize()
    return d_feat.view(B, T, P, CH).clone(), r_words.view(B, T, T).clone()


@pytest.mark.parametrize("decoupled", [True, False], ids=["decoupled", "per_step"])
def test_decoder_gradient_vs_reference(fx, decoupled):
    """SURVEY §8(d)'s bounds as tests/test_gpu_adaatt.py uses them: d_feat within 1e-4 of each map's maximum, r_words within 1e-5 of the fp32
    row (a `long` row: `_words_row`), exact zeros behind word t; `mask_features` changes nothing"""
    g, eng = fx.g, fx.eng
    eng.decoupled = decoupled
    try:
        for name, caps, rows in (("small", g["small_caption"], [(b, t, (b, t)) for b in range(2) for t in range(3)]),
                                 ("long", g["long_caption"], [(0, int(t), i) for i, t in enumerate(g["long_words"])])):
            feats, caps = _features(g, name), torch.from_numpy(caps)
            d_feat, r_words = _decoder(eng, feats, caps)
            plain = _decoder(eng, feats, caps, mask_features=False)
            assert torch.equal(d_feat, plain[0]) and torch.equal(r_words, plain[1]), "mask_features changes the result"
            for (b, t, w) in rows:
                e = rel_err(d_feat[b, t].cpu(), g[name + "_d_feat"][w])
                print("%s image %d word %d (%s): d_feat %.2e of the maximum" % (name, b, t, "decoupled" if decoupled else "per step", e))
                dd, e64, noise = _words_row("%s image %d word %d" % (name, b, t), r_words[b, t, :t + 1].cpu().numpy(), g[name + "_r_words"][w][:t + 1],
                                            g[name + "_r_words64"][w][:t + 1])
                assert e < 1e-4, (name, b, t, e)
                if name == "long" and dd >= 1e-5:
                    assert e64 <= 3.0 * max(noise, 1e-5), (name, b, t, "vs fp64", e64, noise)
                else:
                    assert dd < 1e-5, (name, b, t, dd)
                assert torch.count_nonzero(r_words[b, t, t + 1:]) == 0
    finally:
        eng.decoupled = True


# ---- 3. VGG16 end to end ----------------------------------------------------------------------------------------------------------------------
def test_vgg_decoder_gradient_vs_reference(vgg):
    g = vgg.g
    assert vgg.d_feat.shape == (1, 3, 196, 512) and vgg.eng.vgg is not None
    for t in range(3):
        e = rel_err(vgg.d_feat[0, t][:, ::4], g["vgg_d_feat"][t])
        print("vgg word %d: d_feat %.2e of the maximum (every 4th channel)" % (t, e))
        d, _, _ = _words_row("vgg word %d" % t, vgg.r_words[0, t, :t + 1].numpy(), g["vgg_r_words"][t][:t + 1], g["vgg_r_words64"][t][:t + 1])
        assert e < 1e-4 and d < 1e-5, (t, e, d)
        assert torch.count_nonzero(vgg.r_words[0, t, t + 1:]) == 0
    assert torch.equal(vgg.guided_r_words, vgg.r_words) and torch.equal(vgg.cam_r_words, vgg.r_words)


@pytest.mark.parametrize("kind", ["gradient", "guided"])
def test_vgg_maps_end_to_end_vs_reference(vgg, kind):
    """whole pipeline on the GPU; compared modulo the flipped decisions of THIS run's forward, as tests/test_gpu_gradient.py does"""
    gm = _load("adaatt_grad_maps.npz" if kind == "gradient" else "adaatt_grad_guided_maps.npz")
    assert int(gm["seed"]) == int(vgg.g["seed"])
    maps = vgg.maps if kind == "gradient" else vgg.guided
    assert maps.shape == (1, 3, 3, 224, 224)
    for t in range(3):
        assert_close_modulo_pool_ties(maps[0, t][None, :, ::4, ::4], gm["vgg_%s_map_sub4_%d" % (kind, t)], what="%s %d" % (kind, t), **vgg.e2e)
    assert_close_modulo_pool_ties(maps[0, 2], gm["vgg_%s_map_full_2" % kind][0], what=kind + " full", **vgg.e2e)


def test_vgg_grad_cam_vs_reference(vgg):
    """(1, 196) heat maps in [0, 1]: a ratio of two sums over the GPU forward's features, 1e-3 absolute end to end"""
    g = vgg.g
    assert tuple(vgg.cams.shape) == (1, 3, 196)
    for t in range(3):
        d = float(np.abs(vgg.cams[0, t].numpy() - g["vgg_cam"][t]).max())
        print("vgg word %d: Grad-CAM %.2e absolute (the reference's maximum %.3f)" % (t, d, float(g["vgg_cam"][t].max())))
        assert d < 1e-3, (t, d)


def test_drop_in_classes(vgg):
    """the three classes return the reference's shapes and the same values through `explain_caption(img, caption_encode=...)`"""
    from lrp_amd.explainers import ExplainAdaptiveGradCam, ExplainAdaptiveGradient, ExplainiAdaptiveGuidedGradient
    g = vgg.g
    args = types.SimpleNamespace(embed_dim=512, hidden_dim=512, encoder='vgg16', weight='', save_path='', dataset='synthetic', height=224, width=224)
    model = {k: torch.from_numpy(v) for k, v in vgg.sd.items()}
    cap = g["vgg_caption"].tolist()
    for cls, kind in ((ExplainAdaptiveGradient, "gradient"), (ExplainiAdaptiveGuidedGradient, "guided")):
        gm = _load("adaatt_grad_maps.npz" if kind == "gradient" else "adaatt_grad_guided_maps.npz")
        ex = cls(args, vgg.wm, model=model)
        assert type(ex.engine).__name__ == "AdaAttGradEngine"
        maps, rws = ex.explain_caption(vgg.img, caption_encode=cap)
        torch.cuda.synchronize()
        assert len(maps) == 3 and len(rws) == 3 and ex.caption_length == 3 and ex.beam_caption_encode == cap
        for t in range(3):
            assert maps[t].shape == (1, 3, 224, 224) and rws[t].shape == (t + 1,)
            assert_close_modulo_pool_ties(maps[t].cpu()[:, :, ::4, ::4], gm["vgg_%s_map_sub4_%d" % (kind, t)], what="drop-in %s %d" % (kind, t), **vgg.e2e)
            d = np.abs(rws[t].cpu().numpy() - g["vgg_r_words"][t][:t + 1]).max()
            print("drop-in %s word %d: r_words %.2e" % (kind, t, d))
            assert d < 1e-5
        rf, rw = ex.explain_caption_wordt(1)
        assert rf.shape == (1, 512, 14, 14) and rw.shape == (2,)
        assert rel_err(rf.cpu()[0].reshape(512, 196).t()[:, ::4], g["vgg_d_feat"][1]) < 1e-4
        one = ex.explain_cnn(rf)                                             # a fresh gradient per call: no running sums in this family
        assert one.shape == (1, 3, 224, 224) and torch.equal(one, ex.explain_cnn(rf))
        assert rel_err(one, maps[1]) < 1e-5                                  # (the same activations and masks: fp32 rounding of a map run alone)
    exc = ExplainAdaptiveGradCam(args, vgg.wm, model=model)
    cams, rws = exc.explain_caption(vgg.img, caption_encode=cap)
    assert len(cams) == 3 and all(tuple(c.shape) == (1, 196) for c in cams) and rws[2].shape == (3,)
    for t in range(3):
        assert np.abs(cams[t].cpu().numpy()[0] - g["vgg_cam"][t]).max() < 1e-3, t
    rf, _ = exc.explain_caption_wordt(2)
    assert np.abs(exc.explain_cnn(rf).cpu().numpy()[0] - g["vgg_cam"][2]).max() < 1e-3


# ---- 4. the engine against itself ------------------------------------------------------------------------------------------------------------
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
    """one image alone equals the same image inside a batch of 17 (51 rows: two row tiles of the lock-step kernel, another kernel
    instance than alone) and of 65 (195 rows: seven tiles; the trace's recurrence runs in slices of 64 images)"""
    feats, caps = _small_inputs(3, B=B)
    many = _clones(small.explain_features_gradient(feats, caps))
    assert many[0].shape == (B, 3, P, CH) and many[1].shape == (B, 3, 3)
    for b in (0, B - 1):
        one = small.explain_features_gradient(feats[b:b + 1], caps[b:b + 1])
        _same(one, tuple(t[b:b + 1] for t in many), "image %d alone" % b)


def test_unequal_caption_lengths(small):
    feats, caps = _small_inputs(4)
    full = _clones(small.explain_features_gradient(feats, caps))
    for lens in ([3, 2], [2, 0]):
        d_feat, r_words = small.explain_features_gradient(feats, caps, lens=lens)
        torch.cuda.synchronize()
        for b in range(2):
            assert torch.equal(d_feat[b, :lens[b]], full[0][b, :lens[b]]) and torch.equal(r_words[b, :lens[b]], full[1][b, :lens[b]]), (lens, b)
            assert torch.count_nonzero(d_feat[b, lens[b]:]) == 0 and torch.count_nonzero(r_words[b, lens[b]:]) == 0
    d_feat, r_words = small.explain_features_gradient(feats, caps, lens=[0, 0])
    assert d_feat.shape == (2, 3, P, CH) and torch.count_nonzero(d_feat) == 0 and torch.count_nonzero(r_words) == 0


def test_replica_stream_and_repeat_match_serial(small):
    batches = [_small_inputs(k) + (([3, 2],) if k == 1 else ()) for k in range(3)]
    rep = small.replica()
    assert type(rep) is type(small) and rep.w_hh_t is small.w_hh_t and rep._idx_cache is not small._idx_cache
    grad = lambda eng, f, c, lens: eng.explain_features_gradient(f, c, lens=lens)
    serial = [_clones(grad(rep if i % 2 else small, b[0], b[1], b[2] if len(b) > 2 else None)) for i, b in enumerate(batches)]
    got = [_clones(o) for o in small._explain_stream(batches, 2, grad)]
    assert len(got) == 3 and len(small._replicas) == 2
    for k in range(3):
        _same(got[k], serial[k], "batch %d" % k)
    _same(_clones(grad(small, batches[0][0], batches[0][1], None)), serial[0], "a second call on the same input")
    # `explain_stream` as inherited: the LRP explanation, what `AdaAttEngine` gives
    lrp = [_clones(o) for o in small.explain_stream(batches, depth=2)]
    for k, b in enumerate(batches):
        _same(lrp[k], small.explain_features(b[0], b[1], lens=b[2] if len(b) > 2 else None), "inherited explain_stream, batch %d" % k)


# ---- 5. a ResNet encoder ---------------------------------------------------------------------------------------------------------------------
def test_resnet_encoder():
    """45 x 51 images through the tiny bottleneck net of tests/test_gpu_adaatt.py::test_resnet_encoder (P = 12 = 3 x 4, C = 192): the batch
    entries are the encoder, the decoder gradient and `ResNetEncoder.gradient` / `.guided_backprop(relus="stem")`, bit for bit"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from make_golden_resnet import bottleneck_net
    from lrp_amd import weights
    from lrp_amd.LRPtools import lrp_modules
    from lrp_amd.explainers import AdaAttGradEngine
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "resnet_engine.npz"))["x"])
    net = bottleneck_net(np.random.RandomState(int(np.load(os.path.join(GOLDEN, "gridtd_resnet.npz"))["net_seed"])), lrp_modules.resAdd, 12,
                         [1, 2, 1]).cuda()
    eng = AdaAttGradEngine(weights.make_adaatt_state(seed=7, vocab_size=503, feat_dim=CH, num_pixels=P, encoder=None), encoder=net)
    assert eng.resnet and eng.vgg is None and eng.cnn.feature_shape(45, 51) == (3, 4, CH)
    B, T = x.shape[0], 3
    caps = torch.from_numpy(weights.make_captions(8, B, T, 503))
    row2img = torch.arange(B, device="cuda", dtype=torch.int32).repeat_interleave(T)
    for entry, chain in ((eng.explain_batch_gradient, eng.cnn.gradient), (eng.explain_batch_guided, lambda d, m: eng.cnn.guided_backprop(d, m, relus="stem"))):
        maps, r_words, d_feat, tr, enc = entry(x, caps, return_features=True)
        maps, r_words, d_feat, feats = maps.clone(), r_words.clone(), d_feat.clone(), enc["feats"].clone()
        assert maps.shape == (B, T, 3, 45, 51) and d_feat.shape == (B, T, P, CH)
        df2, rw2 = eng.explain_features_gradient(feats, caps)
        torch.cuda.synchronize()
        assert torch.equal(df2, d_feat) and torch.equal(rw2, r_words)
        eng.cnn.forward(x.cuda())
        again = chain(d_feat.view(B * T, P, CH).contiguous(), row2img)
        torch.cuda.synchronize()
        assert torch.equal(again.view_as(maps), maps)
        assert float(maps.abs().max()) > 0
    cams, _ = eng.explain_batch_gradient(x, caps, cam=True)
    assert cams.shape == (B, T, 12)
    with pytest.raises(NotImplementedError, match="factor of 32"):
        eng.explain_batch_guided(x, caps, gradcam=True)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_fire_before_any_launch(small, monkeypatch):
    from lrp_amd import _lib
    from lrp_amd.explainers import ExplainAdaptiveGuidedGradCam
    feats, caps = _small_inputs(0)
    enc = small.encode(features=feats)
    plain = small.trace(enc, caps, predictions=False)                        # no output gate, no sentinel gate
    torch.cuda.synchronize()

    def boom(*a, **k):
        raise AssertionError("a library call before the refusal")
    monkeypatch.setattr(_lib, "load", boom)
    with pytest.raises(NotImplementedError, match="factor of 32"):
        small.explain_batch_guided(feats, caps, gradcam=True)
    args = types.SimpleNamespace(embed_dim=512, hidden_dim=512, encoder='vgg16', weight='', save_path='', dataset='synthetic', height=224, width=224)
    with pytest.raises(NotImplementedError, match="factor of 32"):
        ExplainAdaptiveGuidedGradCam(args, {"<start>": 0, "<end>": 1})
    with pytest.raises(ValueError, match="grad=True"):
        small.guided_gradient(enc, plain)
    for bad in (feats[:, :11], feats[:, :, :191], torch.zeros(2, 196, 512), torch.zeros(2, P)):
        with pytest.raises(ValueError, match="AdaAttEngine"):
            small.explain_features_gradient(bad, caps)
    for entry in (small.explain_batch_gradient, small.explain_batch_guided):
        with pytest.raises(ValueError, match="takes \\(B, P, C\\) features"):          # images, but this engine has no encoder
            entry(torch.zeros(2, 3, 224, 224), caps)
