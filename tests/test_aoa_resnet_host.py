"""Host logic of the AoA engine on a ResNet encoder: the constructor refusals of `AOAResNetEngine` / `AOAEngine` that need no device, the
routing of an AoA state dict by its encoder keys, the refusals of the entry points and drop-ins that are decided before the device, and
the stored conditions of tests/golden/aoa_resnet.npz and aoa_resnet_grad.npz."""
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import lrp_amd  # noqa: F401
from lrp_amd import ops, weights
from lrp_amd.LRPtools import lrp_modules
from lrp_amd.explainers import aoa as A
from lrp_amd.explainers import engine_base
from lrp_amd.explainers.aoa import AOAEngine, AOAResNetEngine
from lrp_amd.explainers.gridtd import GridTDEngine

from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet import bottleneck_net  # noqa: E402
from test_gridtd_resnet_host import net_and_state  # noqa: E402

PREFIX = "img_encoder.encoder."


def test_constructor_signatures():
    """`AOAEngine` keeps the constructor tests/golden/explainer_api.json records; the encoder's two parameters are `AOAResNetEngine`'s"""
    assert str(inspect.signature(AOAEngine.__init__)) == "(self, state, num_head=8, device='cuda')"
    assert issubclass(AOAResNetEngine, AOAEngine) and set(vars(AOAResNetEngine)) <= {"__init__", "__doc__", "__module__"}
    p = inspect.signature(AOAResNetEngine.__init__).parameters
    assert list(p) == ["self", "state", "num_head", "device", "encoder", "encoder_conv_mode"]
    assert p["num_head"].default == 8 and p["device"].default == "cuda" and p["encoder"].default is None
    assert p["encoder_conv_mode"].default == 1
    with pytest.raises(TypeError):
        AOAEngine(state={}, encoder_conv_mode=0)


@pytest.mark.parametrize("mode", [2, 3, -1, True, None, "1"])
def test_constructor_refuses_a_bad_encoder_conv_mode(mode):
    with pytest.raises(ValueError, match=r"^AOAResNetEngine: encoder_conv_mode .* modes 0 \(fp32 MFMA\) and 1 \(exact bf16 split\)$"):
        AOAResNetEngine({}, encoder_conv_mode=mode)


def test_both_engines_refuse_through_one_helper_with_their_own_name():
    assert AOAEngine._init_encoder is GridTDEngine._init_encoder is engine_base.EngineBase._init_encoder
    with pytest.raises(ValueError) as a:
        AOAResNetEngine({}, encoder_conv_mode=2)
    with pytest.raises(ValueError) as g:
        GridTDEngine({}, encoder_conv_mode=2)
    assert str(g.value) == "GridTDEngine: encoder_conv_mode 2: the ResNet encoder engine has modes 0 (fp32 MFMA) and 1 (exact bf16 split)"
    assert str(a.value) == str(g.value).replace("GridTDEngine", "AOAResNetEngine")


def test_constructor_refuses_nets_the_engine_does_not_run_without_a_device():
    class Basic(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(8, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8)
            self.conv2, self.bn2 = nn.Conv2d(8, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8)
            self.relu = nn.ReLU(inplace=True)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(3, 8, 7, 2, 3, bias=False), nn.BatchNorm2d(8)
            self.relu, self.maxpool = nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1)
            self.layer1 = nn.Sequential(Basic())
    with pytest.raises(ValueError, match="BasicBlock"):
        AOAResNetEngine({}, encoder=Net().eval())
    with pytest.raises(ValueError, match="not a bottleneck ResNet"):
        AOAResNetEngine({}, encoder=nn.Sequential(nn.Conv2d(3, 8, 3)))
    net = bottleneck_net(np.random.RandomState(3), lrp_modules.resAdd, 8, [1, 1])
    net.layers[1].conv2.dilation = (2, 2)
    with pytest.raises(ValueError, match="dilation"):
        AOAResNetEngine({}, encoder=net)
    net = bottleneck_net(np.random.RandomState(3), lrp_modules.resAdd, 8, [1, 1])
    net.layers[0].conv2.groups = 2
    with pytest.raises(ValueError, match="groups=2"):
        AOAResNetEngine({}, encoder=net)


def test_constructor_refuses_a_module_that_is_not_on_the_gpu_before_any_device_work():
    net = bottleneck_net(np.random.RandomState(1), lrp_modules.resAdd, 8, [1])
    for cls in (AOAResNetEngine, GridTDEngine):
        with pytest.raises(ValueError, match="live on the GPU"):
            cls({}, encoder=net)


def test_an_aoa_state_dict_is_routed_by_its_encoder_keys():
    _, enc_sd = net_and_state(prefix=PREFIX)
    dec = weights.make_aoa_state(seed=1, vocab_size=307, feat_dim=128, with_encoder=False)
    assert not any(k.startswith(PREFIX) for k in dec) and dec["img_projector.weight"].shape == (512, 128, 1, 1)
    assert not engine_base.resnet_encoder_keys(dec)
    assert not engine_base.resnet_encoder_keys(weights.make_aoa_state(seed=1, vocab_size=307))          # VGG16: numbered layers
    state = dict(dec, **enc_sd)
    assert engine_base.resnet_encoder_keys(state) and A.resnet_encoder_keys is engine_base.resnet_encoder_keys
    net = ops.bottleneck_resnet_from_state(state, PREFIX)                 # what the engine builds from such a state
    assert net.feat_dim == 128 and len(ops.match_bottleneck_resnet(net).blocks) == 5
    # a malformed ResNet state is refused by the builder, from the constructor, before any device work
    del state[PREFIX + "layer2.0.bn2.running_var"]
    with pytest.raises(ValueError, match=r"'img_encoder\.encoder\.layer2\.0\.bn2\.running_var'"):
        AOAEngine(state)


def _host_engine(resnet=True):
    """an AOAEngine with its encoder fields set by hand: what the entry points read before they touch the device"""
    eng = AOAEngine.__new__(AOAEngine)
    eng.resnet, eng.vgg = resnet, None
    eng.cnn = types.SimpleNamespace(feature_shape=lambda H, W: (-(-H // 32), -(-W // 32), 2048))
    eng.C, eng.H, eng.device = 2048, 512, torch.device("cpu")
    return eng


def test_entry_points_refuse_before_the_device():
    eng = _host_engine()
    cap, x = torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 3, 224, 224)
    with pytest.raises(NotImplementedError, match=r"AOAEngine\.explain_batch_gradient\(kind='guided_gradcam'\): not built for a ResNet "
                                                  r"encoder - .*fixed 16.*stride of 32"):
        eng.explain_batch_gradient(cap, 0, x, kind="guided_gradcam")
    with pytest.raises(NotImplementedError, match=r"AOAEngine\.explain_batch_graph: not built for a ResNet encoder - .*recording is missing"):
        eng.explain_batch_graph(cap, 0, images=x)
    with pytest.raises(NotImplementedError, match=r"AOAEngine\.explain_batch_replay: not built for a ResNet encoder - .*recording.*is missing"):
        eng.explain_batch_replay(cap, 0, images=x)
    # Grad-CAM: lrpx_gradcam holds a heat map of at most 256 pixels - 544 x 544 gives 17 x 17 = 289
    with pytest.raises(ValueError, match=r"289 pixels.*at most 256"):
        eng.explain_batch_gradient(cap, 0, torch.zeros(1, 3, 544, 544), kind="gradcam")
    # the encoder's channels against img_projector's input width: both numbers are named
    eng.C = 512
    with pytest.raises(ValueError, match=r"2048 feature channels.*built for 512 \(img_projector\)"):
        eng.encode(x)
    with pytest.raises(ValueError, match=r"images must be \(B, 3, H, W\)"):
        eng.encode(torch.zeros(3, 224, 224))


def test_the_texts_of_the_graph_refusals_are_gridtds():
    want_graph = "the ResNet engine's trace has not been captured in a HIP graph (the recording is missing)"
    want_replay = ("the recording of the ResNet engine's step (_lib.Recording has only been built and checked around the VGG16 chain's "
                   "calls) is missing")
    assert engine_base.EngineBase._NO_GRAPH == want_graph and engine_base.EngineBase._NO_RECORDING == want_replay
    g = GridTDEngine.__new__(GridTDEngine)
    g.resnet = True
    x, cap = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, dtype=torch.int64)
    with pytest.raises(NotImplementedError) as e:
        g.explain_batch_graph(x, cap)
    assert str(e.value) == "GridTDEngine.explain_batch_graph: not built for a ResNet encoder - " + want_graph
    with pytest.raises(NotImplementedError) as e:
        g.explain_batch_replay(x, cap)
    assert str(e.value) == "GridTDEngine.explain_batch_replay: not built for a ResNet encoder - " + want_replay


def test_the_guided_gradcam_drop_in_refuses_a_resnet_before_anything_is_uploaded():
    from lrp_amd.explainers import engine_cache
    _, enc_sd = net_and_state(prefix=PREFIX)
    state = {k: torch.from_numpy(v) for k, v in weights.make_aoa_state(seed=1, vocab_size=307, feat_dim=128, with_encoder=False).items()}
    state.update(enc_sd)
    args = types.SimpleNamespace(embed_dim=512, hidden_dim=512, encoder='resnet101', weight='', save_path='/tmp', dataset='synthetic',
                                 height=45, width=51, num_head=8)
    engine_cache.clear()
    with pytest.raises(NotImplementedError, match="ExplainAOAGuidedGradCam: not built for a ResNet encoder - .*fixed 16"):
        A.ExplainAOAGuidedGradCam(args, weights.make_word_map(307), model=state)
    engine_cache.clear()


def test_engine_key_tells_a_resnet_engine_and_its_mode_from_a_vgg16_one():
    _, enc_sd = net_and_state(prefix=PREFIX)
    dec = {k: torch.from_numpy(v) for k, v in weights.make_aoa_state(seed=1, vocab_size=307, feat_dim=128, with_encoder=False).items()}
    res = dict(dec, **enc_sd)

    def key(model, **kw):
        ex = A.ExplainAOAAttention.__new__(A.ExplainAOAAttention)
        ex.num_head, ex.model = 8, model
        ex.args = types.SimpleNamespace(weight='', **kw)
        return ex._engine_key()
    assert key(res)[-1] == ("resnet", 1) and key(res, encoder_conv_mode=0)[-1] == ("resnet", 0)
    assert key(res) != key(res, encoder_conv_mode=0) and key(res) == key(res, encoder_conv_mode=1)
    assert key(dec)[-1] == 8 and key(dec) == key(dec, encoder_conv_mode=0)              # no ResNet: the key of before, whatever the mode


def test_lrp_fixture_meets_its_stored_conditions():
    g = np.load(os.path.join(GOLDEN, "aoa_resnet.npz"))
    assert g["caption"].shape == (2, 4) and g["features"].shape == (2, 192, 3, 4) and g["maps64"].shape == (2, 3, 3, 45, 51)
    assert g["tr_alphas"].shape == (2, 3, 8, 12) and g["heads"].tolist() == [5, 0]
    assert int(g["net_seed"]) == int(np.load(os.path.join(GOLDEN, "resnet_engine.npz"))["seed"])
    assert int(g["caption_seed"]) == int(g["decoder_seed"]) + 1
    assert np.array_equal(g["caption"], weights.make_captions(int(g["caption_seed"]), 2, 3, int(g["V"])))
    for k in ("r_feat", "h1_r_feat", "maps"):
        assert float(g["e32_" + k]) < 1e-5, k
    for k in ("r_words", "h1_r_words"):
        assert float(g["e32_" + k]) < 3e-6, k
    # the stored distances are those of the stored arrays
    for k in ("r_feat", "h1_r_feat", "r_words", "h1_r_words"):
        e = np.abs(g[k].astype(np.float64) - g[k + "64"]).max() / np.abs(g[k + "64"]).max()
        assert abs(e - float(g["e32_" + k])) <= 1e-3 * float(g["e32_" + k]) + 1e-12, k
    e = max(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()
            for a, b in zip(g["maps"].reshape(6, -1), g["maps64"].reshape(6, -1)))
    assert abs(e - float(g["e32_maps"])) <= 1e-3 * float(g["e32_maps"])
    for b in range(2):
        for t in range(3):
            assert not g["r_words64"][b, t, t + 1:].any() and np.abs(g["r_words64"][b, t, :t + 1]).max() == pytest.approx(1.0)
    assert np.abs(g["r_feat64"] - g["h1_r_feat64"]).max() > 1e-3 * np.abs(g["r_feat64"]).max()          # two heads, two results


def test_gradient_fixture_meets_its_stored_conditions():
    from make_golden_resnet_grad import MARGIN
    g = np.load(os.path.join(GOLDEN, "aoa_resnet_grad.npz"))
    rg = np.load(os.path.join(GOLDEN, "resnet_grad.npz"))
    assert int(g["net_seed"]) == int(rg["engine_seed"]) and int(g["head"]) == 5
    assert float(g["relu_margin"]) >= MARGIN and float(g["pool_margin"]) >= MARGIN
    assert float(g["relu_margin"]) == float(rg["engine_relu_margin"]) and float(g["pool_margin"]) == float(rg["engine_pool_margin"])
    for k in ("d_img_feature", "r_words", "maps_plain", "maps_guided", "cams"):
        assert float(g["e32_" + k]) < 1e-5, k
    assert g["d_img_feature64"].shape == (2, 3, 192, 3, 4) and g["maps_plain64"].shape == (2, 3, 3, 45, 51) and g["cams64"].shape == (2, 3, 12)
    assert g["d_img_feature64"].dtype == np.float64
    # the reference's hooks clamp at the stem's ReLU alone: its path IS the stem-only restatement, far from the other two
    assert float(g["hook_vs_stem"]) < 1e-5 and float(g["hook_vs_all"]) > 0.1 and float(g["hook_vs_plain"]) > 0.1
    assert np.abs(g["maps_plain64"] - g["maps_guided64"]).max() > 0.1 * np.abs(g["maps_plain64"]).max()
    assert g["cams64"].min() >= 0 and g["cams64"].max() <= 1
