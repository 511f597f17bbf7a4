"""The AoA LRP explainer on the batched bottleneck-ResNet encoder engine: `AOAResNetEngine(state, encoder=...)` / `AOAEngine(state)` and the drop-in
`ExplainAOAAttention` against the reference's `AOAModel(..., 'resnet101')` + `explain_caption(img, head)` on the small net of
tests/golden/resnet_engine.npz (tests/golden/aoa_resnet.npz: B = 2, T = 3, P = 12 = 3 x 4, C = 192, images 45 x 51), in both encoder
conv modes; the seam byte for byte against the composed pieces; an ODD pixel count (P = 25 = 5 x 5, C = 64: the TINY net of
resnet_grad.npz) and the real width (C = 2048, P = 49 = 7 x 7 at the reference's default 224 x 224) against the CPU oracle's decoder.
Every deviation is printed before it is asserted."""
import os
import re
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
from make_golden_resnet_grad import NETS, grad_net  # noqa: E402

PREFIX = "img_encoder.encoder."
PAIRS = dict(ht="h", ct="c", gt="g", it_act="i", ft_act="f", context="ctx", context_aoa="c_aoa", context_aoa_linear="lin", alphas="alpha")
MODES = [0, 1]


def _net(seed, base, blocks):
    from lrp_amd.LRPtools import lrp_modules
    return bottleneck_net(np.random.RandomState(seed), lrp_modules.resAdd, base, blocks)


def _resnet_keys(net, blocks):
    """the net's tensors under the key names of models/resnet.py (layerN.M.*; bottleneck_net keeps one `layers` container)"""
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
    g = np.load(os.path.join(GOLDEN, "aoa_resnet.npz"))
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "resnet_engine.npz"))["x"])
    net = _net(int(g["net_seed"]), 12, [1, 2, 1]).cuda()
    sd = weights.make_aoa_state(seed=int(g["decoder_seed"]), vocab_size=int(g["V"]), feat_dim=192, with_encoder=False)
    cap = torch.from_numpy(g["caption"])
    return types.SimpleNamespace(g=g, x=x, net=net, sd=sd, cap=cap, head=int(g["heads"][0]), head1=int(g["heads"][1]), runs={})


def _run(fx, mode):
    """one engine and one accumulate=True run of the first stored head per encoder mode, shared by the tests (results are clones)"""
    if mode not in fx.runs:
        from lrp_amd.explainers.aoa import AOAResNetEngine
        eng = AOAResNetEngine(fx.sd, encoder=fx.net, encoder_conv_mode=mode)
        maps, r_words, r_feat, tr, enc = eng.explain_batch(fx.cap, fx.head, images=fx.x, accumulate=True, return_features=True,
                                                           predictions=True)
        torch.cuda.synchronize()
        fx.runs[mode] = types.SimpleNamespace(eng=eng, maps=maps.clone(), r_words=r_words.clone(), r_feat=r_feat.clone(),
                                              tr={k: v.clone() for k, v in tr.items() if torch.is_tensor(v)}, feats=enc["feats"].clone())
    return fx.runs[mode]


@pytest.mark.parametrize("mode", MODES)
def test_trace_vs_reference(fx, mode):
    r, g = _run(fx, mode), fx.g
    eng = r.eng
    assert eng.resnet and eng.cnn.conv_mode == mode and eng.vgg is None and eng.C == 192 and eng.cnn.feat_hw == (3, 4) and not eng._f16()
    assert not any(k.startswith(PREFIX) for k in eng.sd)                  # encoder keys do not go into the decoder's tensors
    errs = {"features": rel_err(r.feats.cpu().view(2, 12, 192).permute(0, 2, 1).reshape(2, 192, 3, 4), g["features"])}
    for ref_name, mine in PAIRS.items():
        errs[ref_name] = rel_err(r.tr[mine].cpu(), g["tr_" + ref_name])
    errs["predictions"] = rel_err(r.tr["pred"].cpu()[:, :, ::97], g["tr_predictions"])
    print("mode %d trace deviations (of the maximum): %s" % (mode, ", ".join("%s %.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e < 1e-4, (k, e)


def _check_rows(mode, tag, r_feat, r_words, g, pre):
    got = r_feat.cpu().view(2, 3, 3, 4, 192).permute(0, 1, 4, 2, 3)                 # (B, T, C, h, w)
    for b in range(2):
        for t in range(3):
            e, e64 = rel_err(got[b, t], g[pre + "r_feat"][b, t]), rel_err(got[b, t], g[pre + "r_feat64"][b, t])
            d = np.abs(r_words[b, t, :t + 1].cpu().numpy() - g[pre + "r_words"][b, t, :t + 1]).max()
            d64 = np.abs(r_words[b, t, :t + 1].cpu().numpy() - g[pre + "r_words64"][b, t, :t + 1]).max()
            print("mode %d %s image %d word %d: r_feat %.2e of the maximum (fp64: %.2e; the reference's fp32 %.2e), r_words %.2e (fp64: %.2e; "
                  "%.2e)" % (mode, tag, b, t, e, e64, float(g["e32_" + pre + "r_feat"]), d, d64, float(g["e32_" + pre + "r_words"])))
            assert e < 1e-4 and e64 < 1e-4, (b, t, e, e64)
            assert d < 1e-5, (b, t, d)
            assert torch.count_nonzero(r_words[b, t, t + 1:]) == 0


@pytest.mark.parametrize("mode", MODES)
def test_decoder_relevance_vs_reference(fx, mode):
    r = _run(fx, mode)
    _check_rows(mode, "head %d" % fx.head, r.r_feat, r.r_words, fx.g, "")


@pytest.mark.parametrize("mode", MODES)
def test_a_second_head_vs_reference(fx, mode):
    r = _run(fx, mode)
    maps, r_words, r_feat, tr, enc = r.eng.explain_batch(fx.cap, fx.head1, images=fx.x, return_features=True)
    _check_rows(mode, "head %d" % fx.head1, r_feat, r_words, fx.g, "h1_")
    assert not torch.equal(r_feat, r.r_feat) and torch.isfinite(maps).all() and maps.abs().max() > 0
    for k in PAIRS.values():                                               # the trace does not depend on the head
        assert torch.equal(tr[k], r.tr[k]), k


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
    """explain_batch == ResNetEncoder(module, mode).forward / .relevance around the decoder's own r_feat; the decoder on images ==
    the decoder on the encoder's features (the bottom-up path); accumulate == cumsum_maps"""
    from lrp_amd import ops
    r = _run(fx, mode)
    eng = r.eng
    maps, r_words, r_feat, tr, enc = eng.explain_batch(fx.cap, fx.head, images=fx.x, return_features=True)
    maps, r_words, r_feat = maps.clone(), r_words.clone(), r_feat.clone()
    ref = ops.ResNetEncoder(fx.net, conv_mode=mode)
    feats = ref.forward(fx.x.cuda())
    assert torch.equal(feats, enc["feats"]) and torch.equal(feats, r.feats)
    row2img = torch.arange(2, device="cuda", dtype=torch.int32).repeat_interleave(3)
    want = ref.relevance(r_feat.reshape(6, 12, 192), row2img)
    assert torch.equal(maps.reshape(6, 3, 45, 51), want)
    assert torch.equal(r_feat, r.r_feat) and torch.equal(r_words, r.r_words)
    assert torch.equal(r.maps.reshape(6, 3, 45, 51), ops.cumsum_maps(want, 2, 3))
    assert torch.equal(r.maps[:, 0], maps[:, 0]) and torch.equal(r.maps[:, 1], maps[:, 0] + maps[:, 1])
    f_feat, f_words = eng.explain_batch(fx.cap, fx.head, features=feats.clone())
    assert f_feat.shape == (2, 3, 12, 192) and torch.equal(f_feat, r_feat) and torch.equal(f_words, r_words)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_unequal_lens_are_the_valid_rows_of_the_full_run(fx, mode, accumulate):
    r = _run(fx, mode)
    full = r.maps if accumulate else r.eng.explain_batch(fx.cap, fx.head, images=fx.x)[0].clone()
    lens = [3, 2]
    maps, r_words, r_feat, tr, enc = r.eng.explain_batch(fx.cap, fx.head, images=fx.x, lens=lens, accumulate=accumulate,
                                                         return_features=True, predictions=True)
    assert maps.shape == (2, 3, 3, 45, 51) and torch.equal(tr["pred"], r.tr["pred"])
    for b, n in enumerate(lens):
        assert torch.equal(maps[b, :n], full[b, :n]) and torch.equal(r_words[b, :n], r.r_words[b, :n]), b
        assert torch.equal(r_feat[b, :n], r.r_feat[b, :n]), b
        assert torch.count_nonzero(maps[b, n:]) == 0 and torch.count_nonzero(r_feat[b, n:]) == 0 and torch.count_nonzero(r_words[b, n:]) == 0
    empty = r.eng.explain_batch(fx.cap, fx.head, images=fx.x, lens=[0, 0], accumulate=accumulate)[0]
    assert empty.shape == (2, 3, 3, 45, 51) and torch.count_nonzero(empty) == 0


@pytest.mark.parametrize("mode", MODES)
def test_stream_and_single_image_and_replica(fx, mode):
    r = _run(fx, mode)
    batches = [(fx.x, fx.cap), (fx.x[1:], fx.cap[1:]), (fx.x.flip(0), fx.cap.flip(0), [2, 3])]
    serial = [tuple(t.clone() for t in r.eng.explain_batch(b[1], fx.head, images=b[0], lens=b[2] if len(b) > 2 else None, accumulate=True))
              for b in batches]
    got = [tuple(t.clone() for t in o) for o in r.eng.explain_stream(batches, fx.head, depth=2, accumulate=True)]
    assert len(got) == 3
    for (m0, w0), (m1, w1) in zip(serial, got):
        assert torch.equal(m0, m1) and torch.equal(w0, w1)
    assert torch.equal(serial[0][0], r.maps) and torch.equal(serial[0][1], r.r_words)
    # an image alone gives the bytes it gives inside the batch
    assert torch.equal(serial[1][0][0], r.maps[1]) and torch.equal(serial[1][1][0], r.r_words[1])
    rep = r.eng.replica()
    assert rep.cnn is not r.eng.cnn and rep.cnn.packs is r.eng.cnn.packs and rep.vgg is None and rep.resnet
    m2, w2 = rep.explain_batch(fx.cap, fx.head, images=fx.x, accumulate=True)
    assert torch.equal(m2, r.maps) and torch.equal(w2, r.r_words)


def test_mode_0_differs_from_mode_1_only_in_rounding(fx):
    a, b = _run(fx, 0), _run(fx, 1)
    e = max(rel_err(a.maps[i, t], b.maps[i, t]) for i in range(2) for t in range(3))
    print("mode 0 against mode 1, running-sum maps: %.2e of the maximum" % e)
    assert e < 2e-4                        # each within 1e-4 of fp64


def _state(fx):
    state = {k: torch.from_numpy(v) for k, v in fx.sd.items()}
    state.update(_resnet_keys(fx.net, [1, 2, 1]))
    return state


@pytest.mark.parametrize("mode", MODES)
def test_engine_from_a_state_dict_equals_the_engine_from_the_module(fx, mode):
    """`AOAEngine(state)` itself routes models/resnet.py key names to the ResNet engine, in mode 1; `AOAResNetEngine` in either mode"""
    from lrp_amd.explainers.aoa import AOAEngine, AOAResNetEngine
    r = _run(fx, mode)
    engines = [AOAResNetEngine(_state(fx), encoder_conv_mode=mode)] + ([AOAEngine(_state(fx))] if mode == 1 else [])
    for eng in engines:
        assert eng.resnet and eng.vgg is None and eng.cnn.conv_mode == mode and eng.cnn.plan.convs[0]["module"] is not fx.net.conv1
        assert not any(k.startswith(PREFIX) for k in eng.sd)
        maps, r_words = eng.explain_batch(fx.cap, fx.head, images=fx.x, accumulate=True)
        assert torch.equal(maps, r.maps) and torch.equal(r_words, r.r_words)
    with pytest.raises(TypeError):                 # `AOAEngine` keeps the constructor it had: the module and the mode go to `AOAResNetEngine`
        AOAEngine(_state(fx), encoder=fx.net)


def _args(**kw):
    d = dict(embed_dim=512, hidden_dim=512, encoder='resnet101', weight='', save_path='/tmp', dataset='synthetic', height=45, width=51,
             num_head=8)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_drop_in_built_three_ways(fx, tmp_path):
    from lrp_amd import weights
    from lrp_amd.explainers import engine_cache
    from lrp_amd.explainers.aoa import ExplainAOAAttention
    g, r = fx.g, _run(fx, 1)
    wm = weights.make_word_map(int(g["V"]))
    state = _state(fx)

    class Model:                           # the attribute layout of the reference's AOAModel: .state_dict(), .img_encoder.encoder
        img_encoder = types.SimpleNamespace(encoder=fx.net)

        def state_dict(self):
            return state
    path = str(tmp_path / "aoa_resnet.pth")
    torch.save({"state_dict": state}, path)
    engine_cache.clear()
    ex_m = ExplainAOAAttention(_args(), wm, model=Model())
    engine_cache.clear()                   # (the model's state dict holds the very tensors of `state`: one key, one engine - built twice here)
    ex_s = ExplainAOAAttention(_args(), wm, model=dict(state))
    ex_w = ExplainAOAAttention(_args(weight=path), wm)
    for ex in (ex_m, ex_s, ex_w):
        assert ex.engine.resnet and ex.engine.cnn.conv_mode == 1 and ex.engine.vgg is None
    assert ex_m.engine.cnn.plan.convs[0]["module"] is fx.net.conv1             # the model's own module
    assert ex_s.engine.cnn.plan.convs[0]["module"] is not fx.net.conv1         # rebuilt from the tensors
    assert ex_m._engine_key() != ExplainAOAAttention(_args(encoder_conv_mode=0), wm, model=Model())._engine_key()
    # args.height / args.width size preprocess_img
    from PIL import Image
    img_path = str(tmp_path / "img.png")
    Image.fromarray(np.random.RandomState(0).randint(0, 255, (60, 70, 3)).astype(np.uint8)).save(img_path)
    assert ex_w.preprocess_img(img_path).shape == (1, 3, 45, 51)
    worst = 0.0
    for b in range(2):
        cap = [int(c) for c in g["caption"][b]]
        res = []
        for ex in (ex_m, ex_s, ex_w):
            maps, words = ex.explain_caption(fx.x[b:b + 1], fx.head, caption_encode=cap)
            res.append(([m.clone() for m in maps], [w.clone() for w in words]))
        (maps_m, words_m), (maps_s, words_s), (maps_w, words_w) = res
        assert len(maps_m) == 3 and maps_m[0].shape == (1, 3, 45, 51)
        for t in range(3):
            # the drop-in's explain_caption is the engine's rows (an image alone gives the bytes it gives inside the batch)
            assert torch.equal(maps_m[t][0], r.maps[b, t]) and torch.equal(words_m[t], r.r_words[b, t, :t + 1]), (b, t)
            assert torch.equal(maps_s[t], maps_m[t]) and torch.equal(maps_w[t], maps_m[t])
            assert torch.equal(words_s[t], words_m[t]) and torch.equal(words_w[t], words_m[t])
            e = rel_err(maps_m[t][0].cpu(), g["maps64"][b, t])
            worst = max(worst, e)
            assert e < 1e-4, (b, t, e)
        ex = ex_s
        assert ex.image_features.shape == (1, 192, 3, 4) and ex.num_pixels == 12 and ex.alphas.shape == (3, 8, 12)
        assert ex.predictions.shape == (3, int(g["V"])) and ex.caption_length == 3
        assert rel_err(ex.image_features[0].cpu(), g["features"][b]) < 1e-4
        # explain_caption_wordt + explain_cnn, word by word: the same running sums (the reference's .grad quirk)
        ex._img_grad = None
        for t in range(3):
            rf, rw = ex.explain_caption_wordt(t, fx.head)
            assert rf.shape == (1, 192, 3, 4) and rel_err(rf[0].cpu(), g["r_feat"][b, t]) < 1e-4 and torch.equal(rw, words_s[t])
            assert torch.equal(ex.explain_cnn(rf), maps_s[t])
        words0 = ex.explain_caption_words(fx.x[b:b + 1], caption_encode=cap)                    # head 0 = the second stored head
        assert fx.head1 == 0 and len(words0) == 3
        for t in range(3):
            assert np.abs(words0[t].cpu().numpy() - g["h1_r_words"][b, t, :t + 1]).max() < 1e-5
        pred = ex.teacherforce_forward(fx.x[b:b + 1], cap)
        assert pred.shape == (4, int(g["V"])) and rel_err(pred[:3].cpu(), ex.predictions.cpu()) < 1e-4
    print("drop-in explain_caption: running-sum maps %.2e of their maximum against fp64" % worst)
    ex_again = ExplainAOAAttention(_args(), wm, model=dict(state))          # the cache keys the state's tensors: one engine
    assert ex_again.engine.cnn.packs is ex_s.engine.cnn.packs
    engine_cache.clear()


def test_refusals(fx):
    from lrp_amd import weights
    from lrp_amd.explainers import aoa as A
    from lrp_amd.explainers import engine_cache
    eng = _run(fx, 1).eng
    cap = fx.cap
    # any image size the encoder accepts: 51 x 45 images give 4 x 3 pixels, 64 x 64 images 4 x 4 = 16
    maps = eng.explain_batch(cap, fx.head, images=fx.x.transpose(2, 3).contiguous())[0]
    assert maps.shape == (2, 3, 3, 51, 45) and eng.cnn.feat_hw == (4, 3) and torch.isfinite(maps).all()
    enc = eng.encode(torch.from_numpy(weights.make_images(3, 1, 64, 64)))
    assert enc["P"] == 16 and enc["key"].shape == (1, 16, 512)
    # a decoder of another width
    from lrp_amd.LRPtools import lrp_modules
    tiny = grad_net(3, lrp_modules.resAdd, NETS["tiny"]).cuda()
    other = A.AOAResNetEngine(fx.sd, encoder=tiny)
    with pytest.raises(ValueError, match=r"64 feature channels.*built for 192 \(img_projector\)"):
        other.encode(fx.x)
    with pytest.raises(ValueError, match=r"64 feature channels.*192"):
        other.explain_batch(cap, 0, images=fx.x)
    with pytest.raises(NotImplementedError, match=r"explain_batch_gradient\(kind='guided_gradcam'\): not built for a ResNet encoder"):
        eng.explain_batch_gradient(cap, fx.head, fx.x, kind="guided_gradcam")
    with pytest.raises(ValueError, match=r"289 pixels.*at most 256"):        # stride 16: 272 x 272 images give 17 x 17
        eng.explain_batch_gradient(cap, fx.head, torch.zeros(2, 3, 272, 272), kind="gradcam")
    for call in (lambda: eng.explain_batch_graph(cap, fx.head, images=fx.x), lambda: eng.explain_batch_replay(cap, fx.head, images=fx.x)):
        with pytest.raises(NotImplementedError, match="recording"):
            call()
    with pytest.raises(ValueError, match="encoder_conv_mode"):
        A.AOAResNetEngine(fx.sd, encoder=fx.net, encoder_conv_mode=2)
    with pytest.raises(ValueError, match="live on the GPU"):
        A.AOAResNetEngine(fx.sd, encoder=_net(1, 8, [1]))
    wm = weights.make_word_map(int(fx.g["V"]))
    engine_cache.clear()
    with pytest.raises(NotImplementedError, match="ExplainAOAGuidedGradCam.*not built for a ResNet encoder"):
        A.ExplainAOAGuidedGradCam(_args(), wm, model=_state(fx))
    engine_cache.clear()


def _oracle_rows(sd, feats, cap, head, r_feat, r_words, what):
    """r_feat / r_words of every (image, word) row against the CPU oracle's AoA decoder on the ENGINE's features, at the bounds of
    tests/test_gpu_aoa.py::test_aoa_batch_vs_oracle"""
    from oracle import lrp_oracle as O
    sdt = O.state_to_torch(sd)
    B, T = cap.shape[0], cap.shape[1] - 1
    for b in range(B):
        otr = O.aoa_trace(sdt, feats[b].cpu(), [int(c) for c in cap[b]])
        for t in range(T):
            w_rf, w_rw = O.aoa_explain_wordt(sdt, otr, t, head)
            e, d = rel_err(r_feat[b, t].cpu(), w_rf), np.abs(r_words[b, t, :t + 1].cpu().numpy() - w_rw.numpy()).max()
            print("%s image %d word %d: r_feat %.2e of the maximum (bound 2e-4), r_words %.2e (bound 1e-4) against the oracle" % (what, b, t, e, d))
            assert e < 2e-4 and d < 1e-4, (b, t, e, d)


@pytest.mark.parametrize("mode", MODES)
def test_odd_pixel_count_vs_oracle_and_pieces(mode):
    """P = 25 = 5 x 5 (odd, no multiple of four), C = 64: the TINY net of resnet_grad.npz on its 2 x 3 x 38 x 34 images, T = 3"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import ops, weights
    from lrp_amd.LRPtools import lrp_modules
    from lrp_amd.explainers.aoa import AOAResNetEngine
    G = np.load(os.path.join(GOLDEN, "resnet_grad.npz"))
    V, head = 503, 3
    net = grad_net(int(G["tiny_seed"]), lrp_modules.resAdd, NETS["tiny"]).cuda()
    x = torch.from_numpy(G["tiny_x"])
    sd = weights.make_aoa_state(seed=4, vocab_size=V, feat_dim=64, with_encoder=False)
    cap = torch.from_numpy(weights.make_captions(5, 2, 3, V))
    eng = AOAResNetEngine(sd, encoder=net, encoder_conv_mode=mode)
    maps, r_words, r_feat, tr, enc = eng.explain_batch(cap, head, images=x, return_features=True)
    assert eng.cnn.feat_hw == (5, 5) and enc["P"] == 25 and eng.C == 64 and tr["alpha"].shape == (2, 3, 8, 25)
    assert maps.shape == (2, 3, 3, 38, 34) and torch.isfinite(maps).all() and maps.abs().max() > 0
    assert (tr["alpha"].sum(-1) - 1).abs().max() < 1e-5
    ref = ops.ResNetEncoder(net, conv_mode=mode)
    feats = ref.forward(x.cuda())
    assert torch.equal(feats, enc["feats"])
    row2img = torch.arange(2, device="cuda", dtype=torch.int32).repeat_interleave(3)
    want = ref.relevance(r_feat.reshape(6, 25, 64), row2img)
    assert torch.equal(maps.reshape(6, 3, 38, 34), want)
    f_feat, f_words = eng.explain_batch(cap, head, features=feats.clone())
    assert torch.equal(f_feat, r_feat) and torch.equal(f_words, r_words)
    acc, _ = eng.explain_batch(cap, head, images=x, accumulate=True, lens=[2, 3])
    assert torch.equal(acc[1].reshape(3, 3, 38, 34), ops.cumsum_maps(want[3:].contiguous(), 1, 3))
    assert torch.equal(acc[0, :2].reshape(2, 3, 38, 34), ops.cumsum_maps(want[:2].contiguous(), 1, 2)) and torch.count_nonzero(acc[0, 2]) == 0
    _oracle_rows(sd, feats, cap, head, r_feat, r_words, "P = 25, C = 64, mode %d," % mode)


def test_resnet_width_at_224_vs_pieces_and_oracle():
    """C = 2048, P = 49 = 7 x 7: bottleneck_net(64, [1, 1, 1, 1]) at 1 x 3 x 224 x 224 (the reference's default args.height / args.width),
    T = 2 - feats and maps byte for byte against the composed pieces, r_feat / r_words against the CPU oracle's decoder on the
    engine's features, and `sample_lrp` running"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import ops, weights
    from lrp_amd.explainers.aoa import AOAResNetEngine
    V, head = 503, 6
    net = _net(5, 64, [1, 1, 1, 1]).cuda()
    sd = weights.make_aoa_state(seed=9, vocab_size=V, feat_dim=2048, with_encoder=False)
    x = torch.from_numpy(weights.make_images(21, 1, 224, 224))
    cap = torch.from_numpy(weights.make_captions(22, 1, 2, V))
    eng = AOAResNetEngine(sd, encoder=net)
    assert eng.encoder_conv_mode == 1 and eng.C == 2048 and not eng._f16()
    maps, r_words, r_feat, tr, enc = eng.explain_batch(cap, head, images=x, return_features=True)
    assert maps.shape == (1, 2, 3, 224, 224) and eng.cnn.feat_hw == (7, 7) and enc["P"] == 49
    assert torch.isfinite(maps).all() and maps.abs().max() > 0
    ref = ops.ResNetEncoder(net, conv_mode=1)
    feats = ref.forward(x.cuda())
    assert torch.equal(feats, enc["feats"])
    want = ref.relevance(r_feat.reshape(2, 49, 2048), torch.zeros(2, dtype=torch.int32, device="cuda"))
    assert torch.equal(maps.reshape(2, 3, 224, 224), want)
    f_feat, f_words = eng.explain_batch(cap, head, features=feats.clone())
    assert torch.equal(f_feat, r_feat) and torch.equal(f_words, r_words)
    _oracle_rows(sd, feats, cap, head, r_feat, r_words, "C = 2048, P = 49,")
    wm = weights.make_word_map(V)
    seq, lps = eng.sample_lrp(eng.encode(images=x), 4, wm['<start>'], wm['<end>'], [])
    assert seq.shape == (1, 4) and lps.shape == (1, 4) and torch.isfinite(lps).all() and int(seq[0, 0]) > 0
