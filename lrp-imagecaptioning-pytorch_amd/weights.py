"""Deterministic synthetic weights / inputs for the LRP hot path.

The reference loads a checkpoint `state_dict` (models/gridTDmodel.py:717-718,
models/aoamodel.py:762-763).  There is no network here, so BASELINE.md asks for
random-init weights of the same architecture.  Everything is drawn from a seeded
`numpy.random.RandomState` (a frozen legacy stream: identical numbers on every numpy
version / machine), keyed by the reference's own `state_dict` names, so the very same
dict can be loaded into the reference's `GridTDModel` / `AOAModel` (golden generation)
and into this package's engine.

Distributions follow the reference's initialisers:
  * VGG16 conv: kaiming-normal fan_out, zero bias          (models/vgg.py:48-53)
  * nn.Linear / nn.Conv2d 1x1 / nn.LSTMCell: U(-1/sqrt(fan), 1/sqrt(fan)) (PyTorch defaults)
  * nn.Embedding: N(0, 1)
"""
from collections import OrderedDict
import math

import numpy as np

# models/vgg.py:81 cfgs['D'] with the trailing pool removed (models/gridTDmodel.py:34)
VGG16_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512]
SPECIAL_TOKENS = ("<pad>", "<unk>", "<start>", "<end>")


def vgg16_layers():
    """[(kind, sequential_index, cin, cout)] in forward order; kind in {'conv','pool'}.
    Sequential indices match `vgg.make_layers` (models/vgg.py:62-75): conv, relu, ..., pool."""
    layers, idx, cin = [], 0, 3
    for v in VGG16_CFG:
        if v == 'M':
            layers.append(('pool', idx, cin, cin))
            idx += 1
        else:
            layers.append(('conv', idx, cin, v))
            idx += 2  # conv + relu
            cin = v
    return layers


def _uniform(rs, shape, bound):
    return rs.uniform(-bound, bound, size=shape).astype(np.float32)


def _normal(rs, shape, std):
    return (rs.standard_normal(size=shape) * std).astype(np.float32)


def _vgg_state(rs, prefix, bias_std):
    sd = OrderedDict()
    for kind, idx, cin, cout in vgg16_layers():
        if kind != 'conv':
            continue
        std = math.sqrt(2.0 / (cout * 9))
        sd[f"{prefix}{idx}.weight"] = _normal(rs, (cout, cin, 3, 3), std)
        if bias_std > 0:
            sd[f"{prefix}{idx}.bias"] = _normal(rs, (cout,), bias_std)
        else:
            sd[f"{prefix}{idx}.bias"] = np.zeros((cout,), np.float32)
    return sd


def _linear(rs, sd, name, out_f, in_f, bias=True):
    b = 1.0 / math.sqrt(in_f)
    sd[name + ".weight"] = _uniform(rs, (out_f, in_f), b)
    if bias:
        sd[name + ".bias"] = _uniform(rs, (out_f,), b)


def _lstm(rs, sd, name, in_f, hid):
    b = 1.0 / math.sqrt(hid)
    sd[name + ".weight_ih"] = _uniform(rs, (4 * hid, in_f), b)
    sd[name + ".weight_hh"] = _uniform(rs, (4 * hid, hid), b)
    sd[name + ".bias_ih"] = _uniform(rs, (4 * hid,), b)
    sd[name + ".bias_hh"] = _uniform(rs, (4 * hid,), b)


def make_gridtd_state(seed=0, vocab_size=9586, embed_dim=512, hidden_dim=512, feat_dim=512,
                      num_pixels=196, vgg_bias_std=0.0):
    """state_dict (numpy float32) for the reference `GridTDModel` (models/gridTDmodel.py:111-130)."""
    rs = np.random.RandomState(seed)
    sd = _vgg_state(rs, "img_encoder.encoder.", vgg_bias_std)
    return _gridtd_decoder_state(rs, sd, vocab_size, embed_dim, hidden_dim, feat_dim, num_pixels)


def make_gridtd_resnet_state(seed=0, vocab_size=9586, embed_dim=512, hidden_dim=512, feat_dim=2048, num_pixels=196):
    """The decoder part of `make_gridtd_state` for a ResNet encoder of `feat_dim` channels and a feature map of `num_pixels` pixels
    (resnet50 / resnet101: 2048 channels, 14 x 14 at 448 x 448; models/gridTDmodel.py:26-31,127): no `img_encoder.encoder.` keys - the
    encoder comes as a module (`GridTDEngine(state, encoder=...)`) or its keys are added by the caller.  The draws start at the seed:
    they are not the tail of `make_gridtd_state`'s stream."""
    return _gridtd_decoder_state(np.random.RandomState(seed), OrderedDict(), vocab_size, embed_dim, hidden_dim, feat_dim, num_pixels)


def make_gridtd_bu_state(seed=0, vocab_size=9586, embed_dim=512, hidden_dim=512, feat_dim=2048, num_pixels=36):
    """state_dict (numpy float32) for the reference `GridTDModelBU` (models/gridTDmodel.py:1868-1886; bottom-up region features, no
    encoder): `img_projector` is a Linear(feat_dim, hidden) - a 2-D weight - and `global_img_feature_proj` a Linear(hidden, embed): the
    global feature is taken from the mean of the PROJECTED regions (:1912-1915)."""
    return _gridtd_decoder_state(np.random.RandomState(seed), OrderedDict(), vocab_size, embed_dim, hidden_dim, feat_dim, num_pixels,
                                 bottom_up=True)


def _gridtd_decoder_state(rs, sd, vocab_size, embed_dim, hidden_dim, feat_dim, num_pixels, bottom_up=False):
    b = 1.0 / math.sqrt(feat_dim)
    sd["img_projector.weight"] = _uniform(rs, (hidden_dim, feat_dim) if bottom_up else (hidden_dim, feat_dim, 1, 1), b)
    sd["img_projector.bias"] = _uniform(rs, (hidden_dim,), b)
    _linear(rs, sd, "global_img_feature_proj", embed_dim, hidden_dim if bottom_up else feat_dim)
    _lstm(rs, sd, "LanguageLSTM", 2 * hidden_dim, hidden_dim)
    _lstm(rs, sd, "AdaLSTM.lstm_cell", 2 * embed_dim + hidden_dim, hidden_dim)
    _linear(rs, sd, "AdaLSTM.x_gate", hidden_dim, 2 * embed_dim + hidden_dim)
    _linear(rs, sd, "AdaLSTM.h_gate", hidden_dim, hidden_dim)
    _linear(rs, sd, "AdaAttention.W_v_proj", num_pixels, hidden_dim)
    _linear(rs, sd, "AdaAttention.W_s_proj", num_pixels, hidden_dim)
    _linear(rs, sd, "AdaAttention.W_g_proj", num_pixels, hidden_dim, bias=False)
    _linear(rs, sd, "AdaAttention.w_h", 1, num_pixels, bias=False)
    sd["embedding.weight"] = _normal(rs, (vocab_size, embed_dim), 1.0)
    _linear(rs, sd, "fc", vocab_size, hidden_dim)
    return sd


def make_adaatt_state(seed=0, vocab_size=9586, embed_dim=512, hidden_dim=512, feat_dim=512, num_pixels=196, encoder="vgg16",
                      vgg_bias_std=0.0):
    """state_dict (numpy float32) for the reference `AdaptiveAttentionCaptioningModel` (models/adaptiveattention.py:103-121; the
    single-LSTM adaptive-attention model), in the key order of its `state_dict()`.  encoder="vgg16": the VGG16 keys under
    `img_encoder.encoder.` come first; encoder=None: no `img_encoder.` keys (a ResNet encoder comes as a module or its keys are added by
    the caller; region-style features need none), and the draws start at the seed.
    Order of the draws: [VGG16 convs,] img_projector (weight, bias), global_img_feature_proj, AdaLSTM.lstm_cell (`_lstm`: weight_ih,
    weight_hh, bias_ih, bias_hh; input 2 * embed_dim), AdaLSTM.x_gate, AdaLSTM.h_gate, AdaAttention.W_v_proj, W_s_proj, W_g_proj, w_h,
    embedding (`_normal`, std 1), fc."""
    if encoder not in ("vgg16", None):
        raise ValueError("make_adaatt_state: encoder must be 'vgg16' or None, got {!r}".format(encoder))
    rs = np.random.RandomState(seed)
    sd = _vgg_state(rs, "img_encoder.encoder.", vgg_bias_std) if encoder == "vgg16" else OrderedDict()
    b = 1.0 / math.sqrt(feat_dim)
    sd["img_projector.weight"] = _uniform(rs, (hidden_dim, feat_dim, 1, 1), b)
    sd["img_projector.bias"] = _uniform(rs, (hidden_dim,), b)
    _linear(rs, sd, "global_img_feature_proj", embed_dim, feat_dim)
    _lstm(rs, sd, "AdaLSTM.lstm_cell", 2 * embed_dim, hidden_dim)
    _linear(rs, sd, "AdaLSTM.x_gate", hidden_dim, 2 * embed_dim)
    _linear(rs, sd, "AdaLSTM.h_gate", hidden_dim, hidden_dim)
    _linear(rs, sd, "AdaAttention.W_v_proj", num_pixels, hidden_dim)
    _linear(rs, sd, "AdaAttention.W_s_proj", num_pixels, hidden_dim)
    _linear(rs, sd, "AdaAttention.W_g_proj", num_pixels, hidden_dim, bias=False)
    _linear(rs, sd, "AdaAttention.w_h", 1, num_pixels, bias=False)
    sd["embedding.weight"] = _normal(rs, (vocab_size, embed_dim), 1.0)
    _linear(rs, sd, "fc", vocab_size, hidden_dim)
    return sd


def make_aoa_state(seed=0, vocab_size=11027, embed_dim=512, hidden_dim=512, feat_dim=512,
                   vgg_bias_std=0.0, with_encoder=True):
    """state_dict (numpy float32) for the reference `AOAModel` (models/aoamodel.py:116-142).
    `with_encoder=False` gives the bottom-up variant's decoder-side tensors only (feat_dim=2048,
    models/aoamodel.py:1795-1797: `img_projector` is then a Linear(feat_dim, hidden))."""
    rs = np.random.RandomState(seed)
    sd = _vgg_state(rs, "img_encoder.encoder.", vgg_bias_std) if with_encoder else OrderedDict()
    b = 1.0 / math.sqrt(feat_dim)
    sd["img_projector.weight"] = _uniform(rs, (hidden_dim, feat_dim, 1, 1), b)
    sd["img_projector.bias"] = _uniform(rs, (hidden_dim,), b)
    sd["embedding.weight"] = _normal(rs, (vocab_size, embed_dim), 1.0)
    _lstm(rs, sd, "LanguageLSTM", hidden_dim + embed_dim, hidden_dim)
    _linear(rs, sd, "decoder_k_proj", hidden_dim, hidden_dim)
    _linear(rs, sd, "decoder_v_proj", hidden_dim, hidden_dim)
    _linear(rs, sd, "decoder_multihead_attention.q_proj", hidden_dim, hidden_dim)
    _linear(rs, sd, "decoder_aoa_linear_gate", hidden_dim, hidden_dim)
    _linear(rs, sd, "decoder_aoa_linear", hidden_dim, hidden_dim)
    _linear(rs, sd, "fc", vocab_size, hidden_dim)
    return sd


def sharpen_attention(state, factor):
    """A copy of `state` whose attention logits are `factor` times as large: `AdaAttention.w_h.weight` for gridTD / AdaAtt (the logits
    are w_h tanh(.), no bias), `decoder_multihead_attention.q_proj.{weight,bias}` for AoA (the logits are q k / sqrt(dk)).  Random-init
    attention is uniform to a few percent: the 20 largest of 784 patch sums of such a map are decided by rounding (gap between the 20th
    and 21st 1e-4 .. 1e-6 of the largest); the experiments' attention arms are tested on sharpened states."""
    keys = [k for k in ("AdaAttention.w_h.weight", "decoder_multihead_attention.q_proj.weight", "decoder_multihead_attention.q_proj.bias")
            if k in state]
    if not keys or (keys[0].startswith("AdaAttention") and len(keys) != 1) or (keys[0].startswith("decoder_") and len(keys) != 2):
        raise ValueError("sharpen_attention: the state holds neither AdaAttention.w_h.weight (gridTD, AdaAtt) nor "
                         "decoder_multihead_attention.q_proj.weight / .bias (AoA) alone")
    out = OrderedDict(state)
    for k in keys:
        out[k] = (np.asarray(state[k], np.float32) * np.float32(factor)).astype(np.float32)
    return out


def scale_fc(state, factor):
    """A copy of `state` whose word scores depend `factor` times as strongly on the decoder's state (`fc.weight`; `fc.bias`, which
    favours the same words at every step, stays).  Random-init scores are flat: the candidates of a beam search then lie 1e-5 apart.
    The diverse-beam-search goldens are drawn on scaled states, where selections rest on a gap a test can stand on."""
    out = OrderedDict(state)
    out["fc.weight"] = (np.asarray(state["fc.weight"], np.float32) * np.float32(factor)).astype(np.float32)
    return out


def make_word_map(vocab_size):
    """Synthetic word map with the reference's special-token layout (dataset/wordmap_*.json:
    <pad>=0, <unk>=V-3, <start>=V-2, <end>=V-1)."""
    wm = OrderedDict()
    wm["<pad>"] = 0
    for i in range(1, vocab_size - 3):
        wm[f"w{i}"] = i
    wm["<unk>"] = vocab_size - 3
    wm["<start>"] = vocab_size - 2
    wm["<end>"] = vocab_size - 1
    return wm


def make_images(seed, batch, height=224, width=224):
    """Synthetic pre-processed images ~N(0,1), NCHW float32."""
    rs = np.random.RandomState(seed)
    return rs.standard_normal(size=(batch, 3, height, width)).astype(np.float32)


def make_captions(seed, batch, length, vocab_size):
    """Teacher-forced token ids: column 0 is <start>, then `length` words ~U[1, V-4]
    (BASELINE.md §3).  Returns int64 (batch, length+1) — the layout of the reference's
    `beam_caption_encode` (models/gridTDmodel.py:937)."""
    rs = np.random.RandomState(seed)
    cap = rs.randint(1, vocab_size - 3, size=(batch, length + 1)).astype(np.int64)
    cap[:, 0] = vocab_size - 2
    return cap


def make_bu_features(seed, batch, regions=36, feat_dim=2048):
    """Synthetic bottom-up region features ~relu(N(0,1))."""
    rs = np.random.RandomState(seed)
    return np.maximum(rs.standard_normal(size=(batch, regions, feat_dim)), 0).astype(np.float32)
