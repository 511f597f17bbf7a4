"""The AoA gradient explainers on the batched bottleneck-ResNet encoder engine: `AOAEngine.explain_batch_gradient`
(kind = "gradient", "guided", "gradcam") and the drop-ins `ExplainAOAGradient`, `ExplainAOAGuidedGradient`, `ExplainAOAGradCam` against the
reference's classes of the same names on a bottleneck ResNet encoder (tests/golden/aoa_resnet_grad.npz: B = 2, T = 3, P = 12 = 3 x 4,
C = 192, images 45 x 51, the net and images of resnet_grad.npz's `engine` set), in both encoder conv modes.  Bounds against fp64:
d_feat < 1e-4 of its maximum and r_words < 5e-5 (those of tests/test_gpu_guided.py / test_gpu_gridtd_resnet_grad.py), maps and Grad-CAM
heat maps < 1e-4 of their maxima.  The fixture's condition (ReLU masks, pool winners) is checked on the engine's own trace first.  Every
deviation is printed before it is asserted."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lrp_amd  # noqa: F401
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet_grad import MARGIN, NETS, grad_net  # noqa: E402
from test_gpu_aoa_resnet import PREFIX, _args, _resnet_keys  # noqa: E402

_CACHE = {}
MODES = [0, 1]
KINDS = (("plain", "gradient"), ("guided", "guided"), ("cams", "gradcam"))


def run(mode):
    """the three batched entries once per encoder mode, shared read-only"""
    if mode not in _CACHE:
        from lrp_amd import weights
        from lrp_amd.LRPtools import lrp_modules
        from lrp_amd.explainers.aoa import AOAResNetEngine
        g = dict(np.load(os.path.join(GOLDEN, "aoa_resnet_grad.npz")))
        x = torch.from_numpy(np.load(os.path.join(GOLDEN, "resnet_grad.npz"))["engine_x"])
        net = grad_net(int(g["net_seed"]), lrp_modules.resAdd, NETS["engine"]).cuda()
        sd = weights.make_aoa_state(seed=int(g["decoder_seed"]), vocab_size=int(g["V"]), feat_dim=192, with_encoder=False)
        eng = AOAResNetEngine(sd, encoder=net, encoder_conv_mode=mode)
        assert eng.cnn.conv_mode == mode and eng.C == 192 and eng.resnet
        cap, head = torch.from_numpy(g["caption"]), int(g["head"])
        r = types.SimpleNamespace(g=g, eng=eng, x=x, cap=cap, head=head, net=net, sd=sd)
        for tag, kind in KINDS:
            maps, r_words, d_feat, tr, enc = eng.explain_batch_gradient(cap, head, x, kind=kind, return_features=True)
            setattr(r, "maps_" + tag, maps.clone())
            setattr(r, "r_words_" + tag, r_words.clone())
            setattr(r, "d_feat_" + tag, d_feat.clone())
        r.feats = enc["feats"].clone()
        torch.cuda.synchronize()
        _CACHE[mode] = r
    return _CACHE[mode]


@pytest.mark.parametrize("mode", MODES)
def test_the_fixture_condition_holds_on_the_engines_trace(mode):
    """every ReLU mask and every pool winner of the engine's trace against the fp64 forward on the CPU.  A flip is a discontinuity of
    the gradient: the comparisons below would then say nothing about the kernels."""
    from lrp_amd.LRPtools import lrp_modules
    r = run(mode)
    g, eng = r.g, r.eng.cnn
    assert float(g["relu_margin"]) >= MARGIN and float(g["pool_margin"]) >= MARGIN
    eng.forward(r.x.cuda())
    net = grad_net(int(g["net_seed"]), lrp_modules.resAdd, NETS["engine"]).double()
    masks = {}
    with torch.no_grad():
        a = F.relu(net.bn1(net.conv1(r.x.double())))
        masks["act", 0] = a > 0
        stem = a
        a = net.maxpool(a)
        for bi, (blk, pb) in enumerate(zip(net.layers, eng.plan.blocks)):
            o = F.relu(blk.bn1(blk.conv1(a)))
            masks["act", pb["conv1"]] = o > 0
            o = F.relu(blk.bn2(blk.conv2(o)))
            masks["act", pb["conv2"]] = o > 0
            a = F.relu(blk.bn3(blk.conv3(o)) + (a if blk.downsample is None else blk.downsample(a)))
            masks["out", bi] = a > 0
    flips = 0
    for (kind, i), want in masks.items():
        got = eng.trace[kind][i] > 0
        flips += int((got.cpu() != want.permute(0, 2, 3, 1).reshape(got.shape)).sum())
    # the pool: the winner of every window with a positive maximum, on the engine's own stem activation
    k, s_, p_ = net.maxpool.kernel_size, net.maxpool.stride, net.maxpool.padding
    mine = eng.trace["act"][0].cpu().double().view(2, stem.shape[2], stem.shape[3], -1).permute(0, 3, 1, 2).clamp(min=0)
    top, win64 = F.max_pool2d(stem, k, s_, p_, return_indices=True)
    _, win = F.max_pool2d(mine, k, s_, p_, return_indices=True)
    winners = int(((win != win64) & (top > 0)).sum())
    assert flips == 0 and winners == 0, (
        f"the fixture's condition is broken: {flips} ReLU mask(s) and {winners} pool winner(s) of the engine's trace differ from the fp64 "
        f"forward (stored margins {float(g['relu_margin']):.1e} / {float(g['pool_margin']):.1e}); nothing is known about the kernels from "
        f"this fixture")


@pytest.mark.parametrize("mode", MODES)
def test_decoder_gradient_vs_reference_fp64(mode):
    r = run(mode)
    g = r.g
    got = r.d_feat_plain.cpu().view(2, 3, 3, 4, 192).permute(0, 1, 4, 2, 3)           # (B, T, C, h, w)
    words = r.r_words_plain.cpu().numpy()
    for b in range(2):
        for t in range(3):
            e = rel_err(got[b, t], g["d_img_feature64"][b, t])
            d = np.abs(words[b, t, :t + 1] - g["r_words64"][b, t, :t + 1]).max()
            print("mode %d image %d word %d: d_feat %.2e of its maximum (the reference's fp32: %.2e, bound 1e-4), r_words %.2e (%.2e, bound "
                  "5e-5)" % (mode, b, t, e, float(g["e32_d_img_feature"]), d, float(g["e32_r_words"])))
            assert e < 1e-4, (b, t, e)
            assert d < 5e-5, (b, t, d)
            assert not words[b, t, t + 1:].any()
    # the three kinds run the same decoder (the reference's classes inherit explain_caption_wordt unchanged)
    for tag in ("guided", "cams"):
        assert torch.equal(getattr(r, "d_feat_" + tag), r.d_feat_plain) and torch.equal(getattr(r, "r_words_" + tag), r.r_words_plain)


@pytest.mark.parametrize("tag", ["plain", "guided"])
@pytest.mark.parametrize("mode", MODES)
def test_maps_vs_reference_fp64(mode, tag):
    r = run(mode)
    got = getattr(r, "maps_" + tag).cpu()
    assert got.shape == (2, 3, 3, 45, 51)
    for b in range(2):
        for t in range(3):
            e = rel_err(got[b, t], r.g["maps_" + tag + "64"][b, t])
            print("mode %d %s image %d word %d: map %.2e of its maximum against fp64 (the reference's fp32: %.2e)  bound 1.0e-04" % (
                mode, tag, b, t, e, float(r.g["e32_maps_" + tag])))
            assert e < 1e-4, (b, t, e)


@pytest.mark.parametrize("mode", MODES)
def test_grad_cam_heat_maps_vs_reference_fp64(mode):
    r = run(mode)
    got = r.maps_cams.cpu()
    assert got.shape == (2, 3, 12)
    for b in range(2):
        for t in range(3):
            e = rel_err(got[b, t], r.g["cams64"][b, t])
            print("mode %d image %d word %d: Grad-CAM heat map %.2e of its maximum against fp64 (the reference's fp32: %.2e)  bound 1.0e-04"
                  % (mode, b, t, e, float(r.g["e32_cams"])))
            assert e < 1e-4, (b, t, e)


@pytest.mark.parametrize("mode", MODES)
def test_maps_are_the_encoder_engines_on_the_same_d_feat(mode):
    """byte for byte: cnn.gradient / cnn.guided_backprop(relus="stem") / grad_cam on the entry's own d_feat; lens = the valid rows"""
    from lrp_amd import ops
    r = run(mode)
    eng = r.eng
    ref = ops.ResNetEncoder(r.net, conv_mode=mode)
    feats = ref.forward(r.x.cuda())
    assert torch.equal(feats, r.feats)
    row2img = torch.arange(2, device="cuda", dtype=torch.int32).repeat_interleave(3)
    d = r.d_feat_plain.reshape(6, 12, 192)
    assert torch.equal(r.maps_plain.reshape(6, 3, 45, 51), ref.gradient(d, row2img))
    assert torch.equal(r.maps_guided.reshape(6, 3, 45, 51), ref.guided_backprop(d, row2img, relus="stem"))
    assert not torch.equal(r.maps_guided.reshape(6, 3, 45, 51), ref.guided_backprop(d, row2img, relus="all"))
    assert torch.equal(r.maps_cams.reshape(6, 12), eng.grad_cam(dict(feats=r.feats), d, row2img))
    for tag, kind in KINDS:
        maps, r_words, d_feat, tr, enc = eng.explain_batch_gradient(r.cap, r.head, r.x, kind=kind, lens=[2, 3], return_features=True)
        full = getattr(r, "maps_" + tag)
        for b, n in enumerate([2, 3]):
            assert torch.equal(maps[b, :n], full[b, :n]) and torch.equal(d_feat[b, :n], r.d_feat_plain[b, :n]), (tag, b)
            assert torch.equal(r_words[b, :n], r.r_words_plain[b, :n])
            assert torch.count_nonzero(maps[b, n:]) == 0 and torch.count_nonzero(r_words[b, n:]) == 0


def test_the_three_gradient_drop_ins(tmp_path):
    from lrp_amd import weights
    from lrp_amd.explainers import aoa as A
    from lrp_amd.explainers import engine_cache
    r = run(1)
    g = r.g
    wm = weights.make_word_map(int(g["V"]))
    state = {k: torch.from_numpy(v) for k, v in r.sd.items()}
    state.update(_resnet_keys(r.net, [1, 2, 1]))

    class Model:                           # the attribute layout of the reference's AOAModel: .state_dict(), .img_encoder.encoder
        img_encoder = types.SimpleNamespace(encoder=r.net)

        def state_dict(self):
            return state
    path = str(tmp_path / "aoa_resnet_grad.pth")
    torch.save({"state_dict": state}, path)
    engine_cache.clear()
    for cls, tag, build in ((A.ExplainAOAGradient, "plain", lambda c: c(_args(), wm, model=Model())),
                            (A.ExplainAOAGuidedGradient, "guided", lambda c: c(_args(), wm, model=dict(state))),
                            (A.ExplainAOAGradCam, "cams", lambda c: c(_args(weight=path), wm))):
        ex = build(cls)
        assert ex.engine.resnet and ex.engine.cnn.conv_mode == 1
        full = getattr(r, "maps_" + tag)
        for b in range(2):
            cap = [int(c) for c in g["caption"][b]]
            maps, words = ex.explain_caption(r.x[b:b + 1], r.head, caption_encode=cap)
            assert len(maps) == 3 and ex.num_pixels == 12 and ex.image_features.shape == (1, 192, 3, 4)
            for t in range(3):
                want = g["cams64"][b, t] if tag == "cams" else g["maps_" + tag + "64"][b, t]
                assert maps[t].shape == ((1, 12) if tag == "cams" else (1, 3, 45, 51))
                assert rel_err(maps[t][0].cpu(), want) < 1e-4, (tag, b, t)
                assert torch.equal(maps[t][0], full[b, t]), (tag, b, t)                    # the drop-in is the engine's rows
                assert np.abs(words[t].cpu().numpy() - g["r_words64"][b, t, :t + 1]).max() < 5e-5
            # word by word: explain_caption_wordt + explain_cnn (a fresh map per word in this family)
            for t in range(3):
                rf, rw = ex.explain_caption_wordt(t, r.head)
                assert rf.shape == (1, 192, 3, 4) and rel_err(rf[0].cpu(), g["d_img_feature64"][b, t]) < 1e-4 and torch.equal(rw, words[t])
                assert torch.equal(ex.explain_cnn(rf), maps[t]), (tag, b, t)
    engine_cache.clear()


def test_guided_gradcam_is_refused():
    from lrp_amd import weights
    from lrp_amd.explainers import aoa as A
    from lrp_amd.explainers import engine_cache
    r = run(1)
    with pytest.raises(NotImplementedError, match=r"explain_batch_gradient\(kind='guided_gradcam'\): not built for a ResNet encoder - .*fixed 16"):
        r.eng.explain_batch_gradient(r.cap, r.head, r.x, kind="guided_gradcam")
    state = {k: torch.from_numpy(v) for k, v in r.sd.items()}
    state.update(_resnet_keys(r.net, [1, 2, 1]))
    assert PREFIX + "conv1.weight" in state
    engine_cache.clear()
    with pytest.raises(NotImplementedError, match="ExplainAOAGuidedGradCam: not built for a ResNet encoder"):
        A.ExplainAOAGuidedGradCam(_args(), weights.make_word_map(int(r.g["V"])), model=state)
    # ... also when the ResNet engine of these weights is already cached (built by another class)
    A.ExplainAOAGradient(_args(), weights.make_word_map(int(r.g["V"])), model=state)
    with pytest.raises(NotImplementedError, match="ExplainAOAGuidedGradCam: not built for a ResNet encoder"):
        A.ExplainAOAGuidedGradCam(_args(), weights.make_word_map(int(r.g["V"])), model=state)
    engine_cache.clear()
