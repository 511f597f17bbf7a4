"""Host logic of the gridTD engine on a ResNet encoder: `ops.bottleneck_resnet_from_state` - the module builder for
models/resnet.py key names -, `weights.make_gridtd_resnet_state`, and the constructor refusals of `GridTDEngine` that need no device."""
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import lrp_amd  # noqa: F401
from lrp_amd import ops, weights
from lrp_amd.LRPtools import lrp_modules
from lrp_amd.explainers.gridtd import GridTDEngine

from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet import bottleneck_net  # noqa: E402


def net_and_state(seed=7, base=8, blocks=(2, 1, 2), prefix=""):
    """bottleneck_net (one `layers` container) and its state dict under the key names of models/resnet.py: layerN.M.*"""
    net = bottleneck_net(np.random.RandomState(seed), lrp_modules.resAdd, base, list(blocks))
    first = np.cumsum([0] + list(blocks))
    sd = {}
    for k, v in net.state_dict().items():
        m = re.match(r"layers\.(\d+)\.(.*)", k)
        if m:
            i = int(m.group(1))
            n = int(np.searchsorted(first, i, side="right")) - 1
            k = "layer{}.{}.{}".format(n + 1, i - first[n], m.group(2))
        sd[prefix + k] = v
    return net, sd


@pytest.mark.parametrize("prefix", ["", "img_encoder.encoder."])
def test_from_state_rebuilds_the_forward_bit_for_bit(prefix):
    net, sd = net_and_state(prefix=prefix)
    sd["embedding.weight"] = torch.zeros(3, 4)                        # keys outside the prefix are not the builder's
    if prefix == "":
        del sd["embedding.weight"]
    got = ops.bottleneck_resnet_from_state(sd, prefix)
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((2, 3, 45, 51)).astype(np.float32))
    with torch.no_grad():
        want, have = net(x), got(x)
    assert want.shape == (2, 8 * 4 * 4, 3, 4) and torch.equal(want, have)
    assert not got.training and got.feat_dim == 128
    assert [len(getattr(got, n)) for n in ("layer1", "layer2", "layer3")] == [2, 1, 2]
    assert not hasattr(got, "fc")                                     # the class's unused head is ignored


def test_from_state_takes_numpy_arrays_and_the_matcher_accepts_the_result():
    net, sd = net_and_state()
    got = ops.bottleneck_resnet_from_state({k: v.numpy() for k, v in sd.items()})
    plan = ops.match_bottleneck_resnet(got)
    want = ops.match_bottleneck_resnet(net)
    assert [(c["cin"], c["cout"], c["geom"], c["producer"]) for c in plan.convs] == \
        [(c["cin"], c["cout"], c["geom"], c["producer"]) for c in want.convs]
    assert [b["downsample"] is None for b in plan.blocks] == [False, True, False, False, True]
    assert plan.pool == (3, 3, 2, 2, 1, 1)
    assert all(isinstance(b.add, nn.Module) for n in got.layer_names for b in getattr(got, n))


def _drop(sd, key):
    sd = dict(sd)
    del sd[key]
    return sd


@pytest.mark.parametrize("edit, key", [
    (lambda sd: _drop(sd, "layer2.0.bn2.running_var"), "layer2.0.bn2.running_var"),
    (lambda sd: _drop(sd, "conv1.weight"), "conv1.weight"),
    (lambda sd: _drop(sd, "layer2.0.downsample.0.weight"), "layer2.0.downsample.0.weight"),
    (lambda sd: dict(sd, **{"layer1.0.conv4.weight": torch.zeros(4, 4, 1, 1)}), "layer1.0.conv4.weight"),
    (lambda sd: dict(sd, **{"features.0.weight": torch.zeros(4, 3, 3, 3)}), "features.0.weight"),
    (lambda sd: dict(sd, **{"layer1.1.conv2.weight": torch.zeros(8, 16, 3, 3)}), "layer1.1.conv2.weight"),
    (lambda sd: dict(sd, **{"layer3.0.bn3.bias": torch.zeros(7)}), "layer3.0.bn3.bias"),
    (lambda sd: {k: v for k, v in sd.items() if not k.startswith("layer2.")}, "layer2.0.conv1.weight"),
    (lambda sd: {k: v for k, v in sd.items() if not k.startswith("layer1.0.")}, "layer1.0.conv1.weight"),
    (lambda sd: {k: v for k, v in sd.items() if not k.startswith("layer")}, "layer1.0.conv1.weight"),
])
def test_from_state_refuses_malformed_keys(edit, key):
    _, sd = net_and_state()
    with pytest.raises(ValueError) as e:
        ops.bottleneck_resnet_from_state(edit(sd))
    assert repr(key) in str(e.value), str(e.value)


def test_from_state_names_the_key_with_its_prefix():
    _, sd = net_and_state(prefix="img_encoder.encoder.")
    del sd["img_encoder.encoder.bn1.weight"]
    with pytest.raises(ValueError, match=r"'img_encoder\.encoder\.bn1\.weight'"):
        ops.bottleneck_resnet_from_state(sd, "img_encoder.encoder.")


def test_make_gridtd_resnet_state_shapes():
    sd = weights.make_gridtd_resnet_state(seed=3, vocab_size=307, feat_dim=192, num_pixels=12)
    assert not any(k.startswith("img_encoder.") for k in sd)
    vgg = weights.make_gridtd_state(seed=3, vocab_size=307)
    assert sorted(sd) == sorted(k for k in vgg if not k.startswith("img_encoder."))
    assert sd["img_projector.weight"].shape == (512, 192, 1, 1) and sd["global_img_feature_proj.weight"].shape == (512, 192)
    for k in ("W_v_proj", "W_s_proj", "W_g_proj"):
        assert sd["AdaAttention." + k + ".weight"].shape == (12, 512)
    assert sd["AdaAttention.w_h.weight"].shape == (1, 12) and sd["fc.weight"].shape == (307, 512)
    assert all(v.dtype == np.float32 for v in sd.values())
    full = weights.make_gridtd_resnet_state()                          # defaults: resnet50 / resnet101 at 448 x 448
    assert full["img_projector.weight"].shape == (512, 2048, 1, 1) and full["AdaAttention.W_v_proj.weight"].shape == (196, 512)
    again = weights.make_gridtd_resnet_state(seed=3, vocab_size=307, feat_dim=192, num_pixels=12)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)


def test_make_gridtd_state_is_unchanged_by_the_shared_decoder_part():
    """the VGG state draws the same stream as before: its decoder part now comes from the helper both generators share"""
    sd = weights.make_gridtd_state(seed=0, vocab_size=307)
    rs = np.random.RandomState(0)
    for kind, idx, cin, cout in weights.vgg16_layers():
        if kind == "conv":
            w = (rs.standard_normal(size=(cout, cin, 3, 3)) * np.sqrt(2.0 / (cout * 9))).astype(np.float32)
            assert np.array_equal(sd["img_encoder.encoder.%d.weight" % idx], w)
    b = 1.0 / np.sqrt(512)
    assert np.array_equal(sd["img_projector.weight"], rs.uniform(-b, b, size=(512, 512, 1, 1)).astype(np.float32))


@pytest.mark.parametrize("mode", [2, 3, -1, True, None, "1"])
def test_constructor_refuses_a_bad_encoder_conv_mode(mode):
    with pytest.raises(ValueError, match="encoder_conv_mode"):
        GridTDEngine({}, encoder_conv_mode=mode)


def test_constructor_refuses_a_basic_block_net_without_a_device():
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
        GridTDEngine({}, encoder=Net().eval())
    with pytest.raises(ValueError, match="not a bottleneck ResNet"):
        GridTDEngine({}, encoder=nn.Sequential(nn.Conv2d(3, 8, 3)))
