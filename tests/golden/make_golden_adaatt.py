#!/usr/bin/env python3
"""Golden vectors of the single-LSTM adaptive-attention model (models/adaptiveattention.py): the reference's own
`AdaptiveAttentionCaptioningModel` and `ExplainAdaptiveAttention`, loaded from `weights.make_adaatt_state`, under the harness shims of
make_golden.py.  Writes tests/golden/adaatt.npz and - the vgg_map_* arrays, which would take the file past the 1 MiB a committed
file may have - tests/golden/adaatt_maps.npz; arrays only (np.savez_compressed):

  seed, V, feat_seed; state_keys / state_shapes: key names and shapes of `AdaptiveAttentionCaptioningModel.state_dict()` (VGG16 encoder);
  small_*: B = 2 images, each run alone by the reference.  A stub `img_encoder` returns drawn non-negative features
      (weights.make_bu_features(feat_seed, 2, 12, 192): C = 192, 3 x 4 = 12 pixels) and their mean; `img_projector`,
      `global_img_feature_proj` and `AdaAttention = AdaptiveAttention(512, 12)` are sized to them
      (weights.make_adaatt_state(seed, V, feat_dim=192, num_pixels=12, encoder=None)).  T = 3, every word:
      small_caption, small_tr_<name> (the arrays get_hidden_parameters keeps, :639-650; predictions every 97th word), small_r_feat
      (B, T, P, C), small_r_words (B, T, T), small_r_words64, small_r_glob (B, T, E) and small_r_proj (B, T, P, H) -
      `r_global_img_feature` and `r_img_feature_proj` read off the explainer after each word -, small_e32_<quantity> =
      max |fp32 - fp64| / max |fp64| of the reference alone;
  long_*: B = 1 (features feat_seed + 1), T = 26, words 23 - 25, same shape: long_caption, long_words, long_tr_*, long_r_feat (3, P, C),
      long_r_words (3, T), long_r_words64, long_r_glob, long_r_proj, long_e32_*;
  vgg_*: the whole model with the VGG16 encoder (weights.make_adaatt_state(seed, V)) on weights.make_images(seed, 1), 224 x 224 (P = 196,
      C = 512), T = 3, `explain_caption` end to end: vgg_caption, vgg_tr_*, vgg_r_feat (T, P, C / 4) - every 4th channel -, vgg_r_words
      (T, T), vgg_r_words64, vgg_e32_r_feat / vgg_e32_r_words (decoder quantities, fp32 against an fp64 run of the reference),
      vgg_map_stats_<t> / vgg_map_sub4_<t> as make_golden.py's gen_gridtd stores them, vgg_map_full_2;
  decode_*: `greedy_search` ids (max_cap_length 6) and `beam_search(beam_size=3, max_cap_length=20)` ids on the vgg image;
      decode_margin: the smallest (top1 - top2) / |top1| over the score rows they decided on.

    python tests/golden/make_golden_adaatt.py [--first-seed N]

Conditions on the draw (on the reference alone; searched from --first-seed): every e32_r_feat < 1e-5, every e32_r_words < 3e-6,
decode_margin > 1e-4.  Run where the reference is available only; the GPU tests read the .npz."""
import argparse
import contextlib
import io
import os
import tempfile

import numpy as np
import torch
import torch.nn as nn

from make_golden import _patch_explainer, install_stubs, load_pkg, make_args, ref_vgg_patch, stats, sub4, to_torch_sd

HERE = os.path.dirname(os.path.abspath(__file__))
V, H, P, C = 9586, 512, 12, 192
TRACE = ("predictions", "alphas", "betas", "ht", "ct", "gt", "it_act", "ft_act", "st", "context", "context_hat")
LONG_T, LONG_WORDS = 26, (23, 24, 25)


def small_model(ada, weights, seed, dtype):
    """the reference model sized for 12 pixels of 192 channels; its encoder is replaced per image (`explain_features`)"""
    m = ada.AdaptiveAttentionCaptioningModel(H, H, V, 'vgg16')
    m.encoder_raw_dim = C
    m.img_projector = nn.Conv2d(C, H, kernel_size=1, stride=1)
    m.global_img_feature_proj = nn.Linear(C, H)
    m.AdaAttention = ada.AdaptiveAttention(H, P)
    m.img_encoder = nn.Identity()
    m.load_state_dict(to_torch_sd(weights.make_adaatt_state(seed=seed, vocab_size=V, feat_dim=C, num_pixels=P, encoder=None)))
    return m.to(dtype).eval()


def vgg_model(ada, weights, seed, dtype):
    m = ada.AdaptiveAttentionCaptioningModel(H, H, V, 'vgg16')
    m.load_state_dict(to_torch_sd(weights.make_adaatt_state(seed=seed, vocab_size=V)))
    return m.to(dtype).eval()


def explain_words(ada, model, wm, img, cap, words, dtype, cnn=False):
    """one image: the trace and, for the listed words, r_feat (P, C), r_words, r_glob, r_proj; cnn: `explain_caption` end to end instead
    (every word; also the maps)"""
    T = len(cap) - 1
    out = {}
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        ex = ada.ExplainAdaptiveAttention(make_args(tmp), wm, model=model)
        _patch_explainer(ex, img, cap)
        got = {"r_feat": [], "r_words": [], "r_glob": [], "r_proj": []}
        orig = ex.explain_caption_wordt

        def wrapped(t):
            rf, rw = orig(t)
            assert rf.dtype == dtype and rw.dtype == dtype
            c = rf.shape[1]
            got["r_feat"].append(rf.detach().reshape(c, -1).t().clone().numpy())
            row = np.zeros(T, rw.detach().numpy().dtype)
            row[:t + 1] = rw.detach().numpy()
            got["r_words"].append(row)
            got["r_glob"].append(ex.r_global_img_feature.detach().clone().numpy())
            got["r_proj"].append(ex.r_img_feature_proj.detach().clone().numpy())
            return rf, rw
        ex.explain_caption_wordt = wrapped
        if cnn:
            maps, _ = ex.explain_caption("synthetic.jpg")
            out["maps"] = [m.detach() for m in maps]
        else:
            with torch.no_grad():
                ex.get_hidden_parameters("synthetic")
                for t in words:
                    wrapped(t)
        for k in TRACE:
            v = getattr(ex, k).detach()
            out["tr_" + k] = (v[:, ::97] if k == "predictions" else v).numpy()
    out.update({k: np.stack(v) for k, v in got.items()})
    return out


def run_features(ada, weights, seed, dtype, feats, caps, words):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        model, wm, out = small_model(ada, weights, seed, dtype), weights.make_word_map(V), {}
        for b in range(feats.shape[0]):
            F = torch.from_numpy(feats[b]).to(dtype)                                      # (P, C)

            class StubEnc(nn.Module):
                feat_dim = C

                def forward(self, img):
                    return F.t().contiguous().reshape(1, C, 3, 4), F.mean(0)
            model.img_encoder = StubEnc()
            r = explain_words(ada, model, wm, np.zeros((1, 3, 8, 8), np.float32), caps[b], words, dtype)
            for k, v in r.items():
                out.setdefault(k, []).append(v)
        return {k: np.stack(v) for k, v in out.items()}
    finally:
        torch.set_default_dtype(old)


def run_vgg(ada, weights, seed, dtype, img, cap, cnn):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        model = vgg_model(ada, weights, seed, dtype)
        return explain_words(ada, model, weights.make_word_map(V), img.astype(np.float64 if dtype == torch.float64 else np.float32), cap,
                             range(len(cap) - 1), dtype, cnn=cnn)
    finally:
        torch.set_default_dtype(old)


def e32_of(r32, r64, keys=("r_feat", "r_words", "r_glob", "r_proj")):
    return {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max() / np.abs(r64[k]).max()) for k in keys}


def decode(ada, weights, seed, img):
    """the model's own decoding loops (fp32) and the smallest top-two margin of the score rows they decide on"""
    model, wm, margins = vgg_model(ada, weights, seed, torch.float32), weights.make_word_map(V), []

    def hook(mod, inp, outp):
        top = outp.detach().reshape(-1, V).topk(2, -1).values
        margins.append(float(((top[:, 0] - top[:, 1]) / top[:, 0].abs()).min()))
    handle = model.fc.register_forward_hook(hook)
    orig_div = torch.Tensor.__truediv__

    def div14(a, b):          # `beam_idx = top_words / vocab_size` (:414): integer division in the PyTorch 1.4 the reference pins
        if torch.is_tensor(a) and not a.is_floating_point() and isinstance(b, int):
            return torch.div(a, b, rounding_mode="floor")
        return orig_div(a, b)
    g, x = {}, torch.from_numpy(img)
    try:
        with torch.no_grad():
            _, seqs = model.greedy_search(x, wm, max_cap_length=6)
            g["greedy"] = np.array(seqs, np.int64)
            torch.Tensor.__truediv__ = div14
            try:
                _, sen = model.beam_search(x, wm, beam_size=3, max_cap_length=20)
            finally:
                torch.Tensor.__truediv__ = orig_div
            g["beam"], g["beam_size"], g["beam_steps"] = np.array(sen, np.int64), np.int64(3), np.int64(20)
    finally:
        handle.remove()
    g["margin"] = np.float64(min(margins))
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-seed", type=int, default=0)
    first = ap.parse_args().first_seed
    install_stubs()
    weights = load_pkg()
    ref_vgg_patch()
    import models.adaptiveattention as ada
    for seed in range(first, first + 64):
        feat_seed = seed + 3
        fs, fl = weights.make_bu_features(feat_seed, 2, P, C), weights.make_bu_features(feat_seed + 1, 1, P, C)
        cs, cl = weights.make_captions(seed + 1, 2, 3, V), weights.make_captions(seed + 2, 1, LONG_T, V)
        s32 = run_features(ada, weights, seed, torch.float32, fs, cs, range(3))
        s64 = run_features(ada, weights, seed, torch.float64, fs, cs, range(3))
        es = e32_of(s32, s64)
        print("seed %d small: e32 %s" % (seed, ", ".join("%s %.2e" % kv for kv in sorted(es.items()))), flush=True)
        if not (es["r_feat"] < 1e-5 and es["r_words"] < 3e-6):
            continue
        l32 = run_features(ada, weights, seed, torch.float32, fl, cl, LONG_WORDS)
        l64 = run_features(ada, weights, seed, torch.float64, fl, cl, LONG_WORDS)
        el = e32_of(l32, l64)
        print("seed %d long: e32 %s" % (seed, ", ".join("%s %.2e" % kv for kv in sorted(el.items()))), flush=True)
        if not (el["r_feat"] < 1e-5 and el["r_words"] < 3e-6):
            continue
        img, cv = weights.make_images(seed, 1), weights.make_captions(seed + 1, 1, 3, V)[0]
        v32 = run_vgg(ada, weights, seed, torch.float32, img, cv, cnn=True)
        v64 = run_vgg(ada, weights, seed, torch.float64, img, cv, cnn=False)
        ev = e32_of(v32, v64)
        print("seed %d vgg: e32 %s" % (seed, ", ".join("%s %.2e" % kv for kv in sorted(ev.items()))), flush=True)
        if not (ev["r_feat"] < 1e-5 and ev["r_words"] < 3e-6):
            continue
        dec = decode(ada, weights, seed, img)
        print("seed %d decode: margin %.2e" % (seed, dec["margin"]), flush=True)
        if not dec["margin"] > 1e-4:
            continue
        sd = weights.make_adaatt_state(seed=seed, vocab_size=V)
        want = {k: tuple(v.shape) for k, v in vgg_model(ada, weights, seed, torch.float32).state_dict().items()}
        assert list(sd) == list(want) and {k: tuple(v.shape) for k, v in sd.items()} == want
        g = dict(seed=np.int64(seed), V=np.int64(V), feat_seed=np.int64(feat_seed), state_keys=np.array(list(want)),
                 state_shapes=np.array([list(s) + [0] * (4 - len(s)) for s in want.values()], np.int64),
                 small_caption=cs, long_caption=cl, long_words=np.array(LONG_WORDS, np.int64), vgg_caption=cv)
        for name, r32, r64, e in (("small", s32, s64, es), ("long", l32, l64, el)):
            g.update({"%s_%s" % (name, k): v.astype(np.float32) for k, v in r32.items()})
            g[name + "_r_words64"] = r64["r_words"]
            g.update({"%s_e32_%s" % (name, k): np.float64(v) for k, v in e.items()})
        for k in list(g):                     # one image: drop the batch axis of the long set
            if k.startswith("long_") and k not in ("long_caption", "long_words") and not k.startswith("long_e32_"):
                g[k] = g[k][0]
        T = len(cv) - 1
        maps = v32.pop("maps")
        g.update({"vgg_" + k: v.astype(np.float32) for k, v in v32.items() if k.startswith("tr_")})
        g["vgg_r_feat"] = np.ascontiguousarray(v32["r_feat"][:, :, ::4].astype(np.float32))
        g["vgg_r_words"], g["vgg_r_words64"] = v32["r_words"].astype(np.float32), v64["r_words"]
        g["vgg_e32_r_feat"], g["vgg_e32_r_words"] = np.float64(ev["r_feat"]), np.float64(ev["r_words"])
        for t in range(T):
            g["vgg_map_stats_%d" % t] = stats(maps[t])
            g["vgg_map_sub4_%d" % t] = sub4(maps[t]).numpy()
        g["vgg_map_full_%d" % (T - 1)] = maps[T - 1].numpy()
        g.update({"decode_" + k: v for k, v in dec.items()})
        # two files, each under the 1 MiB a committed file may have: the pixel maps of the vgg set travel apart from the rest
        maps_g = {k: g.pop(k) for k in list(g) if k.startswith("vgg_map_")}
        maps_g["seed"] = g["seed"]
        for name, part in (("adaatt.npz", g), ("adaatt_maps.npz", maps_g)):
            path = os.path.join(HERE, name)
            np.savez_compressed(path, **part)
            print("%s: %d bytes on disk; %s" % (name, os.path.getsize(path), {k: np.asarray(v).shape for k, v in part.items()}))
            assert os.path.getsize(path) < 1 << 20, "a committed fixture stays under 1 MiB"
        return
    raise SystemExit("no seed met the conditions")


if __name__ == "__main__":
    main()
