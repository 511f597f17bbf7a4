#!/usr/bin/env python3
"""Golden vectors of the gradient family of the single-LSTM adaptive-attention model (models/adaptiveattention.py:851-1258): the
reference's own `ExplainAdaptiveGradient`, `ExplainiAdaptiveGuidedGradient` and `ExplainAdaptiveGradCam` under the harness shims of
make_golden.py.  The classes build their model and load `args.weight` themselves: they are fed through a patched `torch.load` (and, for
the stub encoder, a patched model constructor).  Writes, arrays only (np.savez_compressed), each file under the 1 MiB a committed file
may have:

  tests/golden/adaatt_grad.npz
      seed, V, feat_seed;
      small_*: the `small` set of make_golden_adaatt.py (stub encoder, B = 2, P = 12, C = 192, T = 3, every word): small_caption,
          small_d_feat (B, T, P, C), small_r_words (B, T, T), small_r_words64 (an fp64 run), small_e32_d_feat / small_e32_r_words =
          max |fp32 - fp64| / max |fp64| of the reference alone;
      long_*: B = 1 (features feat_seed + 1), T = 26, words 23 - 25: long_caption, long_words, long_d_feat (3, P, C), long_r_words (3, T),
          long_r_words64, long_e32_*;
      vgg_*: the whole model with the VGG16 encoder on weights.make_images(seed, 1), 224 x 224, T = 3, `explain_caption` end to end:
          vgg_caption, vgg_d_feat (T, P, C / 4) - every 4th channel -, vgg_r_words (T, T), vgg_r_words64, vgg_e32_*, vgg_cam (T, P) - the
          Grad-CAM class's heat maps;
      guided_equals_gradient: 1 - the generator asserts that the guided class's `explain_caption_wordt` returns tensors `torch.equal`
          to the gradient class's for every word of every set (the two masks :1130 / :1148 select nothing);
  tests/golden/adaatt_grad_maps.npz:        seed, vgg_gradient_map_stats_<t>, vgg_gradient_map_sub4_<t>, vgg_gradient_map_full_2
  tests/golden/adaatt_grad_guided_maps.npz: seed, vgg_guided_map_stats_<t>, vgg_guided_map_sub4_<t>, vgg_guided_map_full_2
      (as make_golden.py's gen_gradient / gen_guided store them).

    python tests/golden/make_golden_adaatt_grad.py [--first-seed N]

Conditions on the draw (on the reference alone; searched from --first-seed): every e32_d_feat < 1e-5, every e32_r_words < 3e-6, and at
least one vgg word whose Grad-CAM map has a positive maximum.  Run where the reference is available only; the tests read the .npz."""
import argparse
import contextlib
import io
import os
import tempfile

import numpy as np
import torch
import torch.nn as nn

from make_golden import _patch_explainer, install_stubs, load_pkg, make_args, ref_vgg_patch, stats, sub4, to_torch_sd
from make_golden_adaatt import C, LONG_T, LONG_WORDS, P, V, small_model

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = ("ExplainAdaptiveGradient", "ExplainiAdaptiveGuidedGradient")


def build(ada, cls_name, wm, sd, tmp, model=None):
    """the reference's class through its own constructor: `torch.load(args.weight)` gives `sd`; model: the stub-encoder model the
    constructor is to pick up in place of a fresh VGG16 one"""
    real_load, real_model = torch.load, ada.AdaptiveAttentionCaptioningModel
    torch.load = lambda *a, **k: {"state_dict": to_torch_sd(sd)}
    if model is not None:
        ada.AdaptiveAttentionCaptioningModel = lambda *a, **k: model
    try:
        return getattr(ada, cls_name)(make_args(tmp), wm)
    finally:
        torch.load, ada.AdaptiveAttentionCaptioningModel = real_load, real_model


def decoder_words(ex, T, words, dtype):
    """`explain_caption_wordt` for the listed words of the explainer's traced caption -> d_feat (n, P, C), r_words (n, T)"""
    d_feat, r_words = [], []
    for t in words:
        rf, rw = ex.explain_caption_wordt(t)
        assert rf.dtype == dtype and rw.dtype == dtype
        d_feat.append(rf.detach().reshape(rf.shape[1], -1).t().clone().numpy())
        row = np.zeros(T, rw.detach().numpy().dtype)
        row[:t + 1] = rw.detach().numpy()
        r_words.append(row)
    return dict(d_feat=np.stack(d_feat), r_words=np.stack(r_words))


def run_features(ada, weights, seed, dtype, feats, caps, words):
    """the stub-encoder sets, one image at a time; both classes, whose decoder results must be equal bit for bit"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        sd = weights.make_adaatt_state(seed=seed, vocab_size=V, feat_dim=C, num_pixels=P, encoder=None)
        model, wm, out = small_model(ada, weights, seed, dtype), weights.make_word_map(V), {}
        for b in range(feats.shape[0]):
            F = torch.from_numpy(feats[b]).to(dtype)                                      # (P, C)

            class StubEnc(nn.Module):
                feat_dim = C

                def forward(self, img):
                    return F.t().contiguous().reshape(1, C, 3, 4), F.mean(0)
            model.img_encoder = StubEnc()
            got = []
            for cls_name in CLASSES:
                with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
                    ex = build(ada, cls_name, wm, sd, tmp, model=model)
                    _patch_explainer(ex, np.zeros((1, 3, 8, 8), np.float32), caps[b])
                    ex.get_hidden_parameters("synthetic")
                    ex.image_feature_proj = ex.image_feature_proj.transpose(1, 2)         # what `explain_caption` does (:1041)
                    got.append(decoder_words(ex, len(caps[b]) - 1, words, dtype))
            assert all(np.array_equal(got[0][k], got[1][k]) for k in got[0]), "the guided class's decoder part differs from the gradient class's"
            for k, v in got[0].items():
                out.setdefault(k, []).append(v)
        return {k: np.stack(v) for k, v in out.items()}
    finally:
        torch.set_default_dtype(old)


def run_vgg(ada, weights, seed, dtype, img, cap, cls_name, cnn):
    """the whole model: `explain_caption` end to end (cnn) or the decoder part alone; -> d_feat, r_words[, maps]"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        T, wm = len(cap) - 1, weights.make_word_map(V)
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
            ex = build(ada, cls_name, wm, weights.make_adaatt_state(seed=seed, vocab_size=V), tmp)
            ex.model.eval()
            _patch_explainer(ex, img.astype(np.float64 if dtype == torch.float64 else np.float32), cap)
            if not cnn:
                with torch.no_grad():
                    ex.get_hidden_parameters("synthetic")
                    ex.image_feature_proj = ex.image_feature_proj.transpose(1, 2)
                    return decoder_words(ex, T, range(T), dtype)
            got, orig = dict(d_feat=[], r_words=[]), ex.explain_caption_wordt

            def wrapped(t):
                rf, rw = orig(t)
                got["d_feat"].append(rf.detach().reshape(rf.shape[1], -1).t().clone().numpy())
                row = np.zeros(T, np.float32)
                row[:t + 1] = rw.detach().numpy()
                got["r_words"].append(row)
                return rf, rw
            ex.explain_caption_wordt = wrapped
            maps, _ = ex.explain_caption("synthetic.jpg")
        out = {k: np.stack(v) for k, v in got.items()}
        out["maps"] = [m.detach() for m in maps]
        return out
    finally:
        torch.set_default_dtype(old)


def e32_of(r32, r64):
    return {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max() / np.abs(r64[k]).max()) for k in ("d_feat", "r_words")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-seed", type=int, default=0)
    first = ap.parse_args().first_seed
    install_stubs()
    weights = load_pkg()
    ref_vgg_patch()
    import models.adaptiveattention as ada
    f32, f64 = torch.float32, torch.float64
    for seed in range(first, first + 64):
        feat_seed = seed + 3
        fs, fl = weights.make_bu_features(feat_seed, 2, P, C), weights.make_bu_features(feat_seed + 1, 1, P, C)
        cs, cl = weights.make_captions(seed + 1, 2, 3, V), weights.make_captions(seed + 2, 1, LONG_T, V)
        sets, ok = {}, True
        for name, feats, caps, words in (("small", fs, cs, range(3)), ("long", fl, cl, LONG_WORDS)):
            r32, r64 = run_features(ada, weights, seed, f32, feats, caps, words), run_features(ada, weights, seed, f64, feats, caps, words)
            e = e32_of(r32, r64)
            print("seed %d %s: e32 %s" % (seed, name, ", ".join("%s %.2e" % kv for kv in sorted(e.items()))), flush=True)
            sets[name] = (r32, r64, e)
            if not (e["d_feat"] < 1e-5 and e["r_words"] < 3e-6):
                ok = False
                break
        if not ok:
            continue
        img, cv = weights.make_images(seed, 1), weights.make_captions(seed + 1, 1, 3, V)[0]
        T = len(cv) - 1
        v32 = run_vgg(ada, weights, seed, f32, img, cv, "ExplainAdaptiveGradient", cnn=True)
        v64 = run_vgg(ada, weights, seed, f64, img, cv, "ExplainAdaptiveGradient", cnn=False)
        ev = e32_of(v32, v64)
        print("seed %d vgg: e32 %s" % (seed, ", ".join("%s %.2e" % kv for kv in sorted(ev.items()))), flush=True)
        if not (ev["d_feat"] < 1e-5 and ev["r_words"] < 3e-6):
            continue
        cam = run_vgg(ada, weights, seed, f32, img, cv, "ExplainAdaptiveGradCam", cnn=True)
        cams = np.stack([m.numpy().reshape(-1) for m in cam["maps"]])
        print("seed %d vgg: Grad-CAM maxima %s" % (seed, cams.max(1)), flush=True)
        if not cams.max() > 0:
            continue
        gd = run_vgg(ada, weights, seed, f32, img, cv, "ExplainiAdaptiveGuidedGradient", cnn=True)
        for other in (cam, gd):
            assert all(np.array_equal(v32[k], other[k]) for k in ("d_feat", "r_words")), "the three classes share one decoder gradient"
        g = dict(seed=np.int64(seed), V=np.int64(V), feat_seed=np.int64(feat_seed), small_caption=cs, long_caption=cl,
                 long_words=np.array(LONG_WORDS, np.int64), vgg_caption=cv, guided_equals_gradient=np.int64(1))
        for name, (r32, r64, e) in sets.items():
            sel = (lambda v: v[0]) if name == "long" else (lambda v: v)           # one image: drop the batch axis of the long set
            g[name + "_d_feat"], g[name + "_r_words"] = sel(r32["d_feat"]).astype(np.float32), sel(r32["r_words"]).astype(np.float32)
            g[name + "_r_words64"] = sel(r64["r_words"])
            g.update({"%s_e32_%s" % (name, k): np.float64(v) for k, v in e.items()})
        g["vgg_d_feat"] = np.ascontiguousarray(v32["d_feat"][:, :, ::4].astype(np.float32))
        g["vgg_r_words"], g["vgg_r_words64"] = v32["r_words"].astype(np.float32), v64["r_words"]
        g["vgg_e32_d_feat"], g["vgg_e32_r_words"] = np.float64(ev["d_feat"]), np.float64(ev["r_words"])
        g["vgg_cam"] = cams.astype(np.float32)
        parts = [("adaatt_grad.npz", g)]
        for kind, r in (("gradient", v32), ("guided", gd)):
            m = dict(seed=g["seed"])
            for t in range(T):
                m["vgg_%s_map_stats_%d" % (kind, t)] = stats(r["maps"][t])
                m["vgg_%s_map_sub4_%d" % (kind, t)] = sub4(r["maps"][t]).numpy()
            m["vgg_%s_map_full_%d" % (kind, T - 1)] = r["maps"][T - 1].numpy()
            parts.append(("adaatt_grad_maps.npz" if kind == "gradient" else "adaatt_grad_guided_maps.npz", m))
        for name, part in parts:
            path = os.path.join(HERE, name)
            np.savez_compressed(path, **part)
            print("%s: %d bytes on disk; %s" % (name, os.path.getsize(path), {k: np.asarray(v).shape for k, v in part.items()}))
            assert os.path.getsize(path) < 1 << 20, "a committed fixture stays under 1 MiB"
        return
    raise SystemExit("no seed met the conditions")


if __name__ == "__main__":
    main()
