"""The gridTD LRP explainer on the batched bottleneck-ResNet encoder engine: `GridTDEngine(state, encoder=...)` and the
drop-in `ExplainGridTDAttention` against the reference's `GridTDModel('resnet101')` + `explain_caption` on the small net of
tests/golden/resnet_engine.npz (tests/golden/gridtd_resnet.npz: B = 2, T = 3, P = 12 = 3 x 4, C = 192, images 45 x 51 - every decoder
kernel at C != 512, P != 196 and maps whose floats are no multiple of four), in both encoder conv modes; the seam itself byte for byte
against the composed pieces; and one case at the real sizes C = 2048, P = 196, 448 x 448 against the CPU oracle's decoder.
Every deviation is printed before it is asserted."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet import bottleneck_net  # noqa: E402

PREFIX = "img_encoder.encoder."
PAIRS = dict(h1t="h1", c1t="c1", h2t="h2", c2t="c2", g1t="g1", g2t="g2", i1t_act="i1", f1t_act="f1", i2t_act="i2", f2t_act="f2", st="s",
             context="ctx", context_hat="ctx_hat", alphas="alpha", betas="beta")


def _net(seed, base, blocks):
    from lrp_amd.LRPtools import lrp_modules
    return bottleneck_net(np.random.RandomState(seed), lrp_modules.resAdd, base, blocks)


def _resnet_keys(net, blocks):
    """the net's tensors under the key names of models/resnet.py (layerN.M.*; bottleneck_net keeps one `layers` container)"""
    import re
    first = np.cumsum([0] + list(blocks))
    sd = {}
    for k, v in net.state_dict().items():
        m = re.match(r"layers\.(\d+)\.(.*)", k)
        if m:
            i = int(m.group(1))
            n = int(np.searchsorted(first, i, side="right")) - 1
            k = "layer{}.{}.{}".format(n + 1, i - first[n], m.group(2))
        sd[PREFIX + k] = v.detach().cpu().clone()
    return sd


@pytest.fixture(scope="module")
def fx():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import weights
    g = np.load(os.path.join(GOLDEN, "gridtd_resnet.npz"))
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "resnet_engine.npz"))["x"])
    net = _net(int(g["net_seed"]), 12, [1, 2, 1]).cuda()
    sd = weights.make_gridtd_resnet_state(seed=int(g["decoder_seed"]), vocab_size=int(g["V"]), feat_dim=192, num_pixels=12)
    cap = torch.from_numpy(g["caption"])
    return types.SimpleNamespace(g=g, x=x, net=net, sd=sd, cap=cap, runs={})


def _run(fx, mode):
    """one engine and one accumulate=True run per encoder mode, shared by the tests (results are clones: never overwritten)"""
    if mode not in fx.runs:
        from lrp_amd.explainers.gridtd import GridTDEngine
        eng = GridTDEngine(fx.sd, encoder=fx.net, encoder_conv_mode=mode)
        maps, r_words, pred, r_feat, tr, enc = eng.explain_batch(fx.x, fx.cap, accumulate=True, return_features=True, predictions=True)
        torch.cuda.synchronize()
        fx.runs[mode] = types.SimpleNamespace(eng=eng, maps=maps.clone(), r_words=r_words.clone(), pred=pred.clone(), r_feat=r_feat.clone(),
                                              tr={k: v.clone() for k, v in tr.items() if torch.is_tensor(v)},
                                              feats=enc["feats"].clone())
    return fx.runs[mode]


MODES = [0, 1]


@pytest.mark.parametrize("mode", MODES)
def test_trace_vs_reference(fx, mode):
    r, g = _run(fx, mode), fx.g
    assert r.eng.cnn.conv_mode == mode and r.eng.vgg is None and r.eng.P == 12 and r.eng.C == 192 and r.eng.cnn.feat_hw == (3, 4)
    errs = {"features": rel_err(r.feats.cpu().view(2, 12, 192).permute(0, 2, 1).reshape(2, 192, 3, 4), g["features"])}
    for ref_name, mine in PAIRS.items():
        errs[ref_name] = rel_err(r.tr[mine].cpu(), g["tr_" + ref_name])
    errs["predictions"] = rel_err(r.pred.cpu()[:, :, ::97], g["tr_predictions"])
    print("mode %d trace deviations (of the maximum): %s" % (mode, ", ".join("%s %.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e < 1e-4, (k, e)


@pytest.mark.parametrize("mode", MODES)
def test_decoder_relevance_vs_reference(fx, mode):
    r, g = _run(fx, mode), fx.g
    got = r.r_feat.cpu().view(2, 3, 3, 4, 192).permute(0, 1, 4, 2, 3)                 # (B, T, C, h, w)
    for b in range(2):
        for t in range(3):
            e, e64 = rel_err(got[b, t], g["r_feat"][b, t]), rel_err(got[b, t], g["r_feat64"][b, t])
            d = np.abs(r.r_words[b, t, :t + 1].cpu().numpy() - g["r_words"][b, t, :t + 1]).max()
            d64 = np.abs(r.r_words[b, t, :t + 1].cpu().numpy() - g["r_words64"][b, t, :t + 1]).max()
            print("mode %d image %d word %d: r_feat %.2e of the maximum (fp64: %.2e), r_words %.2e (fp64: %.2e)" % (mode, b, t, e, e64, d, d64))
            assert e < 1e-4 and e64 < 1e-4, (b, t, e, e64)
            assert d < 1e-5, (b, t, d)
            assert torch.count_nonzero(r.r_words[b, t, t + 1:]) == 0


@pytest.mark.parametrize("mode", MODES)
def test_running_sum_maps_vs_reference_fp64(fx, mode):
    r, g = _run(fx, mode), fx.g
    assert r.maps.shape == (2, 3, 3, 45, 51)
    for b in range(2):
        for t in range(3):
            e = rel_err(r.maps[b, t].cpu(), g["maps64"][b, t])
            print("mode %d image %d word %d: running-sum map %.2e of its maximum against fp64 (the reference's fp32: %.2e)" % (
                mode, b, t, e, rel_err(g["maps"][b, t], g["maps64"][b, t])))
            assert e < 1e-4, (b, t, e)


@pytest.mark.parametrize("mode", MODES)
def test_the_seam_is_the_composed_pieces_byte_for_byte(fx, mode):
    """explain_batch == ResNetEncoder(module, mode).forward / .relevance around the decoder's own r_feat; accumulate == cumsum_maps"""
    from lrp_amd import ops
    r = _run(fx, mode)
    eng = r.eng
    maps, r_words, r_feat, tr, enc = eng.explain_batch(fx.x, fx.cap, return_features=True)
    ref = ops.ResNetEncoder(fx.net, conv_mode=mode)
    feats = ref.forward(fx.x.cuda())
    assert torch.equal(feats, enc["feats"]) and torch.equal(feats, r.feats)
    row2img = torch.arange(2, device="cuda", dtype=torch.int32).repeat_interleave(3)
    want = ref.relevance(r_feat.reshape(6, 12, 192), row2img)
    assert torch.equal(maps.reshape(6, 3, 45, 51), want)
    assert torch.equal(r_feat, r.r_feat) and torch.equal(r_words, r.r_words)
    assert torch.equal(r.maps.reshape(6, 3, 45, 51), ops.cumsum_maps(want, 2, 3))
    assert torch.equal(r.maps[:, 0], maps[:, 0]) and torch.equal(r.maps[:, 1], maps[:, 0] + maps[:, 1])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_unequal_lens_are_the_valid_rows_of_the_full_run(fx, mode, accumulate):
    r = _run(fx, mode)
    full = r.maps if accumulate else r.eng.explain_batch(fx.x, fx.cap)[0].clone()
    lens = [3, 1]
    maps, r_words, pred, r_feat, tr, enc = r.eng.explain_batch(fx.x, fx.cap, lens=lens, accumulate=accumulate, return_features=True,
                                                               predictions=True)
    assert maps.shape == (2, 3, 3, 45, 51) and torch.equal(pred, r.pred)
    for b, n in enumerate(lens):
        assert torch.equal(maps[b, :n], full[b, :n]) and torch.equal(r_words[b, :n], r.r_words[b, :n]), b
        assert torch.equal(r_feat[b, :n], r.r_feat[b, :n]), b
        assert torch.count_nonzero(maps[b, n:]) == 0 and torch.count_nonzero(r_feat[b, n:]) == 0 and torch.count_nonzero(r_words[b, n:]) == 0
    empty = r.eng.explain_batch(fx.x, fx.cap, lens=[0, 0], accumulate=accumulate)[0]
    assert empty.shape == (2, 3, 3, 45, 51) and torch.count_nonzero(empty) == 0


@pytest.mark.parametrize("mode", MODES)
def test_stream_and_single_image_and_replica(fx, mode):
    r = _run(fx, mode)
    batches = [(fx.x, fx.cap), (fx.x[1:], fx.cap[1:]), (fx.x.flip(0), fx.cap.flip(0), [2, 3])]
    serial = [tuple(t.clone() for t in r.eng.explain_batch(b[0], b[1], lens=b[2] if len(b) > 2 else None, accumulate=True)) for b in batches]
    got = [tuple(t.clone() for t in o) for o in r.eng.explain_stream(batches, depth=2, accumulate=True)]
    assert len(got) == 3
    for (m0, w0), (m1, w1) in zip(serial, got):
        assert torch.equal(m0, m1) and torch.equal(w0, w1)
    assert torch.equal(serial[0][0], r.maps) and torch.equal(serial[0][1], r.r_words)
    # an image alone gives the bytes it gives inside the batch
    assert torch.equal(serial[1][0][0], r.maps[1]) and torch.equal(serial[1][1][0], r.r_words[1])
    rep = r.eng.replica()
    assert rep.cnn is not r.eng.cnn and rep.cnn.packs is r.eng.cnn.packs and rep.vgg is None
    m2, w2 = rep.explain_batch(fx.x, fx.cap, accumulate=True)
    assert torch.equal(m2, r.maps) and torch.equal(w2, r.r_words)


def test_mode_0_differs_from_mode_1_only_in_rounding(fx):
    a, b = _run(fx, 0), _run(fx, 1)
    e = max(rel_err(a.maps[i, t], b.maps[i, t]) for i in range(2) for t in range(3))
    print("mode 0 against mode 1, running-sum maps: %.2e of the maximum" % e)
    assert e < 2e-4                        # each within 1e-4 of fp64


def _args(**kw):
    d = dict(embed_dim=512, hidden_dim=512, encoder='resnet101', weight='', save_path='/tmp', dataset='synthetic', height=45, width=51,
             num_head=8)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_drop_in_from_module_and_from_state_dict(fx):
    from lrp_amd import weights
    from lrp_amd.explainers import engine_cache
    from lrp_amd.explainers.gridtd import ExplainGridTDAttention
    g = fx.g
    wm = weights.make_word_map(int(g["V"]))
    state = {k: torch.from_numpy(v) for k, v in fx.sd.items()}
    state.update(_resnet_keys(fx.net, [1, 2, 1]))

    class Model:                           # the attribute layout of the reference's GridTDModel: .state_dict(), .img_encoder.encoder
        img_encoder = types.SimpleNamespace(encoder=fx.net)

        def state_dict(self):
            return state
    engine_cache.clear()
    ex_m = ExplainGridTDAttention(_args(), wm, model=Model())
    engine_cache.clear()                   # (the model's state dict holds the very tensors of `state`: one key, one engine - built twice here)
    ex_s = ExplainGridTDAttention(_args(), wm, model=dict(state))
    assert ex_m.engine.resnet and ex_s.engine.resnet and ex_m.engine.cnn.conv_mode == 1
    assert ex_m.engine.cnn.plan.convs[0]["module"] is fx.net.conv1             # the model's own module
    assert ex_s.engine.cnn.plan.convs[0]["module"] is not fx.net.conv1         # rebuilt from the tensors
    worst = 0.0
    for b in range(2):
        cap = [int(c) for c in g["caption"][b]]
        maps_m, words_m = ex_m.explain_caption(fx.x[b:b + 1], caption_encode=cap)
        maps_m, words_m = [m.clone() for m in maps_m], [w.clone() for w in words_m]
        maps_s, words_s = ex_s.explain_caption(fx.x[b:b + 1], caption_encode=cap)
        assert len(maps_m) == 3 and maps_m[0].shape == (1, 3, 45, 51)
        assert all(torch.equal(p, q) for p, q in zip(maps_m, maps_s)) and all(torch.equal(p, q) for p, q in zip(words_m, words_s))
        assert ex_m.image_features.shape == (1, 192, 3, 4) and ex_m.num_pixels == 12 and ex_m.alphas.shape == (3, 12)
        assert rel_err(ex_m.image_features[0].cpu(), g["features"][b]) < 1e-4
        for t in range(3):
            e = rel_err(maps_m[t][0].cpu(), g["maps64"][b, t])
            worst = max(worst, e)
            assert e < 1e-4, (b, t, e)
            assert np.abs(words_m[t].cpu().numpy() - g["r_words"][b, t, :t + 1]).max() < 1e-5
        # explain_caption_wordt + explain_cnn, word by word: the same running sums (the reference's .grad quirk)
        ex_s._img_grad = None
        for t in range(3):
            rf, rw = ex_s.explain_caption_wordt(t)
            assert rf.shape == (1, 192, 3, 4) and rel_err(rf[0].cpu(), g["r_feat"][b, t]) < 1e-4 and torch.equal(rw, words_s[t])
            assert torch.equal(ex_s.explain_cnn(rf), maps_s[t])
        pred = ex_s.teacherforce_forward(fx.x[b:b + 1], cap)
        assert pred.shape == (4, int(g["V"])) and rel_err(pred[:3].cpu(), ex_s.predictions.cpu()) < 1e-4
    print("drop-in explain_caption: running-sum maps %.2e of their maximum against fp64" % worst)
    ex_again = ExplainGridTDAttention(_args(), wm, model=dict(state))          # the cache keys the state's tensors: one engine
    assert ex_again.engine.cnn.packs is ex_s.engine.cnn.packs
    engine_cache.clear()


def test_refusals(fx):
    from lrp_amd import weights
    from lrp_amd.explainers import gridtd as G
    eng = _run(fx, 1).eng
    with pytest.raises(ValueError, match=r"12 pixels.*192 channels") as e:
        eng.encode(torch.zeros(1, 3, 64, 64))
    assert "4x4" in str(e.value) and "= 16 pixels" in str(e.value)
    with pytest.raises(ValueError, match="12 pixels"):
        eng.explain_batch(torch.zeros(2, 3, 32, 32), fx.cap)                      # a 2 x 2 feature map
    # a rectangular map of the right pixel count is the decoder's business alone: 51 x 45 images give 4 x 3 = 12 pixels and run
    maps = eng.explain_batch(fx.x.transpose(2, 3).contiguous(), fx.cap)[0]
    assert maps.shape == (2, 3, 3, 51, 45) and eng.cnn.feat_hw == (4, 3) and torch.isfinite(maps).all()
    cap = fx.cap
    for call in (lambda: eng.explain_batch_guided(fx.x, cap), lambda: eng.explain_batch_gradient(fx.x, cap),
                 lambda: eng.explain_batch_gradient(fx.x, cap, cam=True)):
        with pytest.raises(NotImplementedError, match="gradient chain through the ResNet"):
            call()
    for call in (lambda: eng.explain_batch_graph(fx.x, cap), lambda: eng.explain_batch_replay(fx.x, cap)):
        with pytest.raises(NotImplementedError, match="recording"):
            call()
    wm = weights.make_word_map(int(fx.g["V"]))
    state = {k: torch.from_numpy(v) for k, v in fx.sd.items()}
    state.update(_resnet_keys(fx.net, [1, 2, 1]))
    for cls in (G.ExplainiGridTDGuidedGradient, G.ExplainGridTDGuidedGradCam, G.ExplainGridTDGradient, G.ExplainGridTDGradCam):
        with pytest.raises(NotImplementedError, match=cls.__name__ + ".*gradient chain through the ResNet"):
            cls(_args(), wm, model=state)
    with pytest.raises(ValueError, match="live on the GPU"):
        G.GridTDEngine(fx.sd, encoder=_net(1, 8, [1]))


def test_resnet_width_at_448_vs_pieces_and_oracle():
    """C = 2048, P = 196: bottleneck_net(64, [1, 1, 1, 1]) at 1 x 3 x 448 x 448, T = 2 - feats and maps byte for byte against the
    composed pieces, r_feat / r_words against the CPU oracle's decoder (it takes P and C from its inputs) on the engine's features, at
    the bounds of test_gpu_gridtd.py::test_batch_of_images_vs_oracle."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import ops, weights
    from lrp_amd.explainers.gridtd import GridTDEngine
    from oracle import lrp_oracle as O
    V = 503
    net = _net(5, 64, [1, 1, 1, 1]).cuda()
    sd = weights.make_gridtd_resnet_state(seed=9, vocab_size=V)
    x = torch.from_numpy(weights.make_images(21, 1, 448, 448))
    cap = torch.from_numpy(weights.make_captions(22, 1, 2, V))
    eng = GridTDEngine(sd, encoder=net)
    assert eng.encoder_conv_mode == 1 and eng.C == 2048 and eng.P == 196 and not eng._f16()
    maps, r_words, r_feat, tr, enc = eng.explain_batch(x, cap, return_features=True)
    assert maps.shape == (1, 2, 3, 448, 448) and eng.cnn.feat_hw == (14, 14) and torch.isfinite(maps).all() and maps.abs().max() > 0
    ref = ops.ResNetEncoder(net, conv_mode=1)
    feats = ref.forward(x.cuda())
    assert torch.equal(feats, enc["feats"])
    want = ref.relevance(r_feat.reshape(2, 196, 2048), torch.zeros(2, dtype=torch.int32, device="cuda"))
    assert torch.equal(maps.reshape(2, 3, 448, 448), want)
    sdt = O.state_to_torch(sd)
    f = feats[0].cpu().t().reshape(2048, 14, 14).contiguous()
    otr = O.gridtd_trace(sdt, f, f.mean(dim=(1, 2)), cap[0].numpy())
    for t in range(2):
        w_rf, w_rw = O.gridtd_explain_wordt(sdt, otr, t)
        e, d = rel_err(r_feat[0, t].cpu(), w_rf), np.abs(r_words[0, t, :t + 1].cpu().numpy() - w_rw.numpy()).max()
        print("C = 2048, P = 196, word %d: r_feat %.2e of the maximum, r_words %.2e against the oracle" % (t, e, d))
        assert e < 2e-4 and d < 1e-4, (t, e, d)
    with pytest.raises(ValueError, match="196 pixels"):
        eng.encode(torch.zeros(1, 3, 224, 224))
