#!/usr/bin/env python3
"""Golden vectors of the gridTD LRP explainer on the BOTTOM-UP model, `GridTDModelBU` (models/gridTDmodel.py:1863-2464; 36 x 2048 region
features, no encoder).  The reference has no bottom-up explainer; the oracle is built from the reference's own code:

  1. a reference `GridTDModelBU` loaded from `weights.make_gridtd_bu_state` gives proj_pre, Vp, avg and glob_pre from the features
     (`forward`, :1912-1915: the global feature is relu(global_img_feature_proj(mean_k relu(img_projector(F))[k])));
  2. a reference `GridTDModel` as a stub shares the BU model's `global_img_feature_proj`, both LSTMs, `AdaAttention`, `embedding` and
     `fc`; its `img_encoder` returns Vp as (1, H, 6, 6) and avg, `encoder_raw_dim = H`, `img_projector` is an identity 1 x 1 conv;
  3. `ExplainGridTDAttention.get_hidden_parameters` and `explain_caption_wordt(t)` run on the stub, verbatim: the trace is the
     bottom-up model's;
  4. after each word `ex.r_global_img_feature` and `ex.r_img_feature_proj` (:1041-1044, :1114) are read - decoder-only quantities;
  5. the stub's own r_img_feature is discarded (the identity projector under the epsilon rule is not the identity);
  6. r_words is the reference's as returned;
  7. the tail is three uses of the reference's own `lrp_linear_eps`, in the order `GridTDModelBU.forward` dictates:
         r_avg     = eps(r_glob, avg, glob_pre, W_gp)
         r_vp[k]   = r_proj[k] + eps(r_avg, Vp[k] / P, avg, eye(H))
         r_feat[k] = eps(r_vp[k], F[k], proj_pre[k], W_proj)

Writes tests/golden/gridtd_bu.npz - arrays only (np.savez_compressed):

  seed, V, feat_seed; state_keys / state_shapes: the key names and shapes of `GridTDModelBU.state_dict()`;
  pair_*: B = 2, T = 3; image 1's last 16 regions are zero (as dataset/dataloader.py:105-108 pads): pair_nonzero (regions kept per
      image; the features are weights.make_bu_features(feat_seed, 2) with the rest zeroed), pair_caption, pair_tr_* (the trace arrays
      make_golden_gridtd_resnet.py stores, predictions every 97th word), pair_r_feat (B, P, C, T) fp32 - WORD LAST: a feature that is
      zero gives T zeros in a row, which the compression folds -, pair_r_words (B, T, T) fp32, pair_r_words64,
      pair_e32_<quantity> = max |fp32 - fp64| / max |fp64|;
  long_*: B = 1, T = 26, 8 non-zero regions (weights.make_bu_features(feat_seed + 1, 1)): long_caption, long_words = [23, 24, 25],
      long_r_feat (P, C, 3) - word last too -, long_r_words (3, T), long_e32_r_feat, long_e32_r_words;
  decode_*: `GridTDModelBU`'s own methods on the pair features: greedy_search ids at max_cap_length 6, beam_search (beam 3) of image 0,
      sample_lrp ids and log-probabilities (8 steps), forwardlrp_context predictions of every 97th word (8 steps, caption seed + 6),
      their arg-max ids, decode_skip (ids exempt from the re-weighting) and decode_margin: the smallest (top1 - top2) / |top1| over
      every score row the four loops decided on.

    python tests/golden/make_golden_gridtd_bu.py [--first-seed N]

Conditions on the draw (reference alone), searched from --first-seed: pair_e32_r_feat < 1e-5 and long_e32_r_feat < 1e-5;
e32_r_words < 3e-6 (make_golden_gridtd_resnet.py's condition: a 1e-5 bound on r_words then measures the engine, not the reference's
rounding); decode_margin > 1e-4 (bit-exact ids then do not measure rounding).  Same harness shims as make_golden.py; run where the
reference is available only."""
import argparse
import os
import tempfile

import numpy as np
import torch
import torch.nn as nn

from make_golden import _patch_explainer, install_stubs, load_pkg, make_args, ref_vgg_patch, to_torch_sd

HERE = os.path.dirname(os.path.abspath(__file__))
V, H, P, C = 9586, 512, 36, 2048
TRACE = ("predictions", "alphas", "betas", "h1t", "c1t", "h2t", "c2t", "g1t", "g2t", "i1t_act", "f1t_act", "i2t_act", "f2t_act", "st",
         "context", "context_hat")
PAIR_NONZERO, LONG_NONZERO = (36, 20), (8,)
LONG_T, LONG_WORDS = 26, (23, 24, 25)


def features(weights, feat_seed, nonzero):
    f = weights.make_bu_features(feat_seed, len(nonzero), P, C)
    for b, n in enumerate(nonzero):
        f[b, n:] = 0
    return f


def models(gtd, weights, seed, dtype):
    """(the bottom-up model, the GridTDModel stub that shares its decoder)"""
    bu = gtd.GridTDModelBU(H, H, V, 'bu')
    bu.load_state_dict(to_torch_sd(weights.make_gridtd_bu_state(seed=seed, vocab_size=V)))
    bu = bu.to(dtype).eval()
    stub = gtd.GridTDModel(H, H, V, 'vgg16')
    stub.encoder_raw_dim = H
    stub.img_projector = nn.Conv2d(H, H, 1)
    stub.img_projector.weight.data = torch.eye(H).reshape(H, H, 1, 1)
    stub.img_projector.bias.data = torch.zeros(H)
    for name in ("global_img_feature_proj", "LanguageLSTM", "AdaLSTM", "AdaAttention", "embedding", "fc"):
        setattr(stub, name, getattr(bu, name))
    return bu, stub.to(dtype).eval()


def explain(gtd, bu, stub, wm, F, cap, words, dtype):
    """one image: the trace and, for the listed words, r_feat (P, C) and r_words of the construction above"""
    T = len(cap) - 1
    F = torch.from_numpy(F).to(dtype)
    with torch.no_grad():
        proj_pre = bu.img_projector(F)                       # (P, H)
        Vp = bu.relu(proj_pre)
        avg = torch.mean(Vp, dim=0)
        glob_pre = bu.global_img_feature_proj(avg)

    class StubEnc(nn.Module):
        feat_dim = H

        def forward(self, img):
            return Vp.t().contiguous().reshape(1, H, 6, 6), avg
    stub.img_encoder = StubEnc()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        ex = gtd.ExplainGridTDAttention(make_args(tmp), wm, model=stub)
        _patch_explainer(ex, np.zeros((1, 3, 8, 8), np.float32), cap)
        with torch.no_grad():
            ex.get_hidden_parameters("synthetic")
        assert ex.image_feature_proj.dtype == dtype
        assert torch.equal(ex.image_feature_proj.reshape(H, P).t(), Vp), "the identity projector of the stub is exact"
        for k in TRACE:
            v = getattr(ex, k).detach()
            out["tr_" + k] = (v[:, ::97] if k == "predictions" else v).numpy()
        eps, eye = ex.lrp_linear_eps, torch.eye(H)
        r_feat, r_words = [], []
        for t in words:
            with torch.no_grad():
                _, rw = ex.explain_caption_wordt(t)
                r_glob, r_proj = ex.r_global_img_feature.clone(), ex.r_img_feature_proj.clone()
                r_avg = eps(r_glob, avg, glob_pre, bu.global_img_feature_proj.weight)
                rf = torch.zeros(P, C)
                for k in range(P):
                    r_vp = r_proj[k] + eps(r_avg, Vp[k] / P, avg, eye)
                    rf[k] = eps(r_vp, F[k], proj_pre[k], bu.img_projector.weight)
            assert rf.dtype == dtype and rw.dtype == dtype
            r_feat.append(rf.numpy())
            row = np.zeros(T, rf.numpy().dtype)
            row[:t + 1] = rw.numpy()
            r_words.append(row)
    out["r_feat"], out["r_words"] = np.stack(r_feat), np.stack(r_words)
    return out


def run(gtd, weights, seed, dtype, feats, caps, words):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        bu, stub = models(gtd, weights, seed, dtype)
        wm = weights.make_word_map(V)
        out = {}
        for b in range(feats.shape[0]):
            for k, v in explain(gtd, bu, stub, wm, feats[b], caps[b], words, dtype).items():
                out.setdefault(k, []).append(v)
        return {k: np.stack(v) for k, v in out.items()}
    finally:
        torch.set_default_dtype(old)


def e32_of(r32, r64):
    return {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max() / np.abs(r64[k]).max()) for k in r32}


def decode(gtd, weights, seed, feats):
    """the bottom-up model's own decoding loops (fp32) and the smallest top-two margin of the score rows they decide on"""
    bu, _ = models(gtd, weights, seed, torch.float32)
    wm = weights.make_word_map(V)
    rev = {v: k for k, v in wm.items()}
    F = torch.from_numpy(feats)
    margins = []

    def hook(mod, inp, outp):
        top = outp.detach().reshape(-1, V).topk(2, -1).values
        margins.append(float(((top[:, 0] - top[:, 1]) / top[:, 0].abs()).min()))
    handle = bu.fc.register_forward_hook(hook)
    orig_div = torch.Tensor.__truediv__

    def div14(a, b):          # `beam_idx = top_words / vocab_size` (:2206): integer division in the PyTorch 1.4 the reference pins
        if torch.is_tensor(a) and not a.is_floating_point() and isinstance(b, int):
            return torch.div(a, b, rounding_mode="floor")
        return orig_div(a, b)
    g = {}
    try:
        with torch.no_grad():
            _, seqs = bu.greedy_search(F, wm, max_cap_length=6)
            g["greedy"] = np.array(seqs, np.int64)
            torch.Tensor.__truediv__ = div14
            try:
                _, sen = bu.beam_search(F[:1], wm, beam_size=3, max_cap_length=20)
            finally:
                torch.Tensor.__truediv__ = orig_div
            g["beam"], g["beam_size"], g["beam_steps"] = np.array(sen, np.int64), np.int64(3), np.int64(20)
            seq, lps, ml = bu.sample_lrp(F, rev, wm, [8 + 1] * F.shape[0], {})
            g["sample_seq"], g["sample_logprobs"], g["sample_len"] = seq.numpy().astype(np.int64), lps.numpy().astype(np.float32), np.int64(ml)
            caps = weights.make_captions(seed + 6, F.shape[0], 8, V)
            lengths = [8 + 1, 8 - 1]
            p, wp, L = bu.forwardlrp_context(F, torch.from_numpy(caps), lengths, rev)
            g["fl_caption"], g["fl_lengths"], g["fl_L"] = caps, np.array(lengths), np.int64(L)
            g["fl_pred_sub"], g["fl_wpred_sub"] = p[:, :, ::97].numpy(), wp[:, :, ::97].numpy()
            g["fl_pred_argmax"], g["fl_wpred_argmax"] = p.argmax(-1).numpy(), wp.argmax(-1).numpy()
    finally:
        handle.remove()
    g["skip"] = np.array([wm[k] for k in ('<start>', '<end>', '<pad>', '<unk>')], np.int64)
    g["margin"] = np.float64(min(margins))
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-seed", type=int, default=0)
    first = ap.parse_args().first_seed
    install_stubs()
    weights = load_pkg()
    ref_vgg_patch()
    import models.gridTDmodel as gtd
    for seed in range(first, first + 64):
        feat_seed = seed + 3
        fp, fl = features(weights, feat_seed, PAIR_NONZERO), features(weights, feat_seed + 1, LONG_NONZERO)
        cp, cl = weights.make_captions(seed + 1, 2, 3, V), weights.make_captions(seed + 2, 1, LONG_T, V)
        p32 = run(gtd, weights, seed, torch.float32, fp, cp, range(3))
        p64 = run(gtd, weights, seed, torch.float64, fp, cp, range(3))
        ep = e32_of(p32, p64)
        print("seed %d pair: e32 %s" % (seed, ", ".join("%s %.2e" % kv for kv in sorted(ep.items()))), flush=True)
        if not (ep["r_feat"] < 1e-5 and ep["r_words"] < 3e-6):
            continue
        dec = decode(gtd, weights, seed, fp)
        print("seed %d decode: margin %.2e" % (seed, dec["margin"]), flush=True)
        if not dec["margin"] > 1e-4:
            continue
        l32 = run(gtd, weights, seed, torch.float32, fl, cl, LONG_WORDS)
        l64 = run(gtd, weights, seed, torch.float64, fl, cl, LONG_WORDS)
        el = e32_of(l32, l64)
        print("seed %d long: e32 r_feat %.2e r_words %.2e" % (seed, el["r_feat"], el["r_words"]), flush=True)
        if not (el["r_feat"] < 1e-5 and el["r_words"] < 3e-6):
            continue
        sd = weights.make_gridtd_bu_state(seed=seed, vocab_size=V)
        want = {k: tuple(v.shape) for k, v in models(gtd, weights, seed, torch.float32)[0].state_dict().items()}
        assert {k: tuple(v.shape) for k, v in sd.items()} == want
        g = dict(seed=np.int64(seed), V=np.int64(V), feat_seed=np.int64(feat_seed), state_keys=np.array(list(want)),
                 state_shapes=np.array([list(s) + [0] * (2 - len(s)) for s in want.values()], np.int64),
                 pair_nonzero=np.array(PAIR_NONZERO, np.int64), pair_caption=cp, long_nonzero=np.array(LONG_NONZERO, np.int64),
                 long_caption=cl, long_words=np.array(LONG_WORDS, np.int64))
        g.update({"pair_" + k: v.astype(np.float32) for k, v in p32.items()})
        g["pair_r_feat"] = np.ascontiguousarray(g["pair_r_feat"].transpose(0, 2, 3, 1))              # (B, P, C, T)
        g["pair_r_words64"] = p64["r_words"]
        g.update({"pair_e32_" + k: np.float64(v) for k, v in ep.items()})
        g["long_r_feat"] = np.ascontiguousarray(l32["r_feat"][0].astype(np.float32).transpose(1, 2, 0))  # (P, C, 3)
        g["long_r_words"] = l32["r_words"][0].astype(np.float32)
        g["long_e32_r_feat"], g["long_e32_r_words"] = np.float64(el["r_feat"]), np.float64(el["r_words"])
        g.update({"decode_" + k: v for k, v in dec.items()})
        path = os.path.join(HERE, "gridtd_bu.npz")
        np.savez_compressed(path, **g)
        print("gridtd_bu.npz: %d bytes on disk; %s" % (os.path.getsize(path), {k: np.asarray(v).shape for k, v in g.items()}))
        return
    raise SystemExit("no seed met the conditions")


if __name__ == "__main__":
    main()
