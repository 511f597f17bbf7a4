"""The ResNet encoder engine's gradient chain composed with the gridTD decoder's gradient entries, against the
reference's `ExplainGridTDGradient`, `ExplainiGridTDGuidedGradient` and `ExplainGridTDGradCam` on a bottleneck ResNet encoder
(tests/golden/gridtd_resnet_grad.npz: B = 2, T = 3, P = 12 = 3 x 4, C = 192, images 45 x 51), in both encoder conv modes.
`GridTDEngine` still refuses its own gradient entries on a ResNet (tests/test_gpu_gridtd_resnet.py pins that); what is composed here are
the pieces that are not refused: encode, trace(grad=True), guided_gradient with and without the feature mask, grad_cam, and
`engine.cnn.gradient / guided_backprop`.  Bounds against fp64: d_feat < 1e-4 of its maximum and r_words < 5e-5 (those of
tests/test_gpu_guided.py), maps and cams < 1e-4 of their maxima.  Every deviation is printed before it is asserted."""
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
from make_golden_resnet_grad import NETS, grad_net  # noqa: E402

_CACHE = {}


def run(mode):
    """the composed pieces once per encoder mode, shared read-only"""
    if mode not in _CACHE:
        from lrp_amd import weights
        from lrp_amd.LRPtools import lrp_modules
        from lrp_amd.explainers.gridtd import GridTDEngine
        g = dict(np.load(os.path.join(GOLDEN, "gridtd_resnet_grad.npz")))
        x = torch.from_numpy(np.load(os.path.join(GOLDEN, "resnet_grad.npz"))["engine_x"])
        net = grad_net(int(g["net_seed"]), lrp_modules.resAdd, NETS["engine"]).cuda()
        sd = weights.make_gridtd_resnet_state(seed=int(g["decoder_seed"]), vocab_size=int(g["V"]), feat_dim=192, num_pixels=12)
        eng = GridTDEngine(sd, encoder=net, encoder_conv_mode=mode)
        assert eng.cnn.conv_mode == mode and eng.P == 12 and eng.C == 192
        cap = torch.from_numpy(g["caption"]).cuda()
        enc = eng.encode(x.cuda())
        tr = eng.trace(enc, cap, predictions=False, grad=True)
        r = types.SimpleNamespace(g=g, eng=eng, enc=enc)
        for tag, mask in (("plain", False), ("guided", True)):
            d_feat, r_words, row2img = eng.guided_gradient(enc, tr, None, mask_features=mask)
            setattr(r, "d_feat_" + tag, d_feat.clone())
            setattr(r, "r_words_" + tag, r_words.clone())
        r.row2img = row2img
        r.cams = eng.grad_cam(enc, r.d_feat_plain, row2img).clone()
        r.maps_plain = eng.cnn.gradient(r.d_feat_plain, row2img).clone()
        r.maps_guided = eng.cnn.guided_backprop(r.d_feat_guided, row2img).clone()
        torch.cuda.synchronize()
        _CACHE[mode] = r
    return _CACHE[mode]


MODES = [0, 1]


@pytest.mark.parametrize("tag", ["plain", "guided"])
@pytest.mark.parametrize("mode", MODES)
def test_decoder_gradient_at_resnet_sizes(mode, tag):
    r = run(mode)
    g = r.g
    assert r.row2img.tolist() == [0, 0, 0, 1, 1, 1]
    got = getattr(r, "d_feat_" + tag).cpu().view(2, 3, 3, 4, 192).permute(0, 1, 4, 2, 3)           # (B, T, C, h, w)
    words = getattr(r, "r_words_" + tag).cpu().view(2, 3, 3).numpy()
    for b in range(2):
        for t in range(3):
            e = rel_err(got[b, t], g["d_feat_" + tag + "64"][b, t])
            d = np.abs(words[b, t, :t + 1] - g["r_words_" + tag + "64"][b, t, :t + 1]).max()
            print("mode %d %s image %d word %d: d_feat %.2e of its maximum (the reference's fp32: %.2e, bound 1e-4), r_words %.2e (%.2e, "
                  "bound 5e-5)" % (mode, tag, b, t, e, float(g["e32_d_feat_" + tag]), d, float(g["e32_r_words_" + tag])))
            assert e < 1e-4, (b, t, e)
            assert d < 5e-5, (b, t, d)
            assert not words[b, t, t + 1:].any()
    if tag == "guided":                        # the `features <= 0` gate (models/gridTDmodel.py:1674)
        feats = r.enc["feats"]
        assert not getattr(r, "d_feat_guided").view(2, 3, 12, 192)[(feats <= 0)[:, None].expand(2, 3, 12, 192)].any()


@pytest.mark.parametrize("tag", ["plain", "guided"])
@pytest.mark.parametrize("mode", MODES)
def test_maps_through_the_encoder(mode, tag):
    r = run(mode)
    got = getattr(r, "maps_" + tag).cpu().view(2, 3, 3, 45, 51)
    for b in range(2):
        for t in range(3):
            e = rel_err(got[b, t], r.g["maps_" + tag + "64"][b, t])
            print("mode %d %s image %d word %d: map %.2e of its maximum against fp64 (the reference's fp32: %.2e)  bound 1.0e-04" % (
                mode, tag, b, t, e, float(r.g["e32_maps_" + tag])))
            assert e < 1e-4, (b, t, e)


@pytest.mark.parametrize("mode", MODES)
def test_grad_cam_heat_maps(mode):
    r = run(mode)
    got = r.cams.cpu().view(2, 3, 12)
    for b in range(2):
        for t in range(3):
            e = rel_err(got[b, t], r.g["cams64"][b, t])
            print("mode %d image %d word %d: Grad-CAM heat map %.2e of its maximum against fp64 (the reference's fp32: %.2e)  bound 1.0e-04"
                  % (mode, b, t, e, float(r.g["e32_cams"])))
            assert e < 1e-4, (b, t, e)


def test_the_engine_still_refuses_its_own_gradient_entries():
    r = run(1)
    x = torch.zeros(2, 3, 45, 51)
    cap = torch.from_numpy(r.g["caption"])
    for call in (lambda: r.eng.explain_batch_guided(x, cap), lambda: r.eng.explain_batch_gradient(x, cap)):
        with pytest.raises(NotImplementedError, match="gradient chain through the ResNet"):
            call()
