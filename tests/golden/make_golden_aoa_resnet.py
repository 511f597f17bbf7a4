#!/usr/bin/env python3
"""Golden vectors of the AoA LRP explainer on a bottleneck ResNet encoder: the REFERENCE's `AOAModel(512, 512, 8, V, 'resnet101')` and its
`ExplainAOAAttention.explain_caption(img, head_idx)` (models/aoamodel.py:31-51, :748-1181), with `models.resnet.resnet101` rebound to
return the small net of resnet_engine.npz (base 12, blocks [1, 2, 1], that fixture's seed: 192 feature channels).  That fixture's
2 x 3 x 45 x 51 images give a 3 x 4 feature map: P = 12 (the AoA attention takes any number of pixels: nothing of the decoder is
replaced).  Per image a T = 3 word caption, once in fp32 and once on .double() copies (default dtype float64 for the call).  The twin of
make_golden_gridtd_resnet.py.  Writes tests/golden/aoa_resnet.npz - arrays only:

  caption (B, T+1); heads (2,); features (B, C, h, w); tr_* (B, ...) the trace arrays make_golden.gen_aoa stores (predictions every
  97th word); for heads[0]: r_feat / r_feat64 (B, T, C, h, w), r_words / r_words64 (B, T, T), row t holds t + 1 entries, maps / maps64
  (B, T, 3, H, W), the running sums `explain_caption` returns; for heads[1]: h1_r_feat / h1_r_feat64, h1_r_words / h1_r_words64;
  e32_<quantity> = max |fp32 - fp64| / max |fp64| (maps: per map, as the tests bound it); net_seed, decoder_seed, caption_seed, V.

    python tests/golden/make_golden_aoa_resnet.py

The decoder state is `weights.make_aoa_state(feat_dim=192, with_encoder=False)` plus the net's keys.  The net's seed is the fixture's.
The decoder / caption seed is searched from --first-seed until e32 < 1e-5 on r_feat (both heads) and on the maps and e32 < 3e-6 on
r_words (both heads), and stored: the tests hold r_words to 1e-5 of the reference's fp32 values, and on a draw where the reference's
own fp32 is further than that from its fp64 the bound would measure the reference's rounding, not the engine's (the condition, and the
reason, of make_golden_gridtd_resnet.py).  Same harness shims as make_golden.py; run where the reference is available only."""
import argparse
import os
import tempfile

import numpy as np
import torch

from make_golden import _patch_explainer, install_stubs, load_pkg, make_args
from make_golden_resnet import bottleneck_net

HERE = os.path.dirname(os.path.abspath(__file__))
NET = dict(base=12, blocks=[1, 2, 1], feat_dim=192)
T, V = 3, 11027
HEADS = (5, 0)
PREFIX = "img_encoder.encoder."
TRACE = ("predictions", "alphas", "ht", "ct", "gt", "it_act", "ft_act", "context", "context_aoa", "context_aoa_linear")


def with_feat_dim(net):
    net.feat_dim = NET["feat_dim"]
    return net


def aoa_state(weights, dec_seed, net):
    """decoder tensors of `weights.make_aoa_state` + the net's tensors under the encoder prefix"""
    sd = {k: torch.from_numpy(v.copy()) for k, v in weights.make_aoa_state(
        seed=dec_seed, vocab_size=V, feat_dim=NET["feat_dim"], with_encoder=False).items()}
    sd.update({PREFIX + k: v for k, v in net.state_dict().items()})
    return sd


def run(aoa, rn, weights, net_seed, dec_seed, x, caps, dtype):
    """the reference's explainer on every image of x -> {name: (B, ...) array}"""
    def small_net(pretrained=True, **kw):
        return with_feat_dim(bottleneck_net(np.random.RandomState(net_seed), rn.Add, NET["base"], NET["blocks"]))
    real = rn.resnet101
    rn.resnet101 = small_net
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        model = aoa.AOAModel(512, 512, 8, V, 'resnet101')
        model.load_state_dict(aoa_state(weights, dec_seed, small_net()))
        model = model.to(dtype).eval()
        wm = weights.make_word_map(V)
        out = {}
        for b in range(x.shape[0]):
            one = {}
            with tempfile.TemporaryDirectory() as tmp:
                ex = aoa.ExplainAOAAttention(make_args(tmp, encoder='resnet101', height=x.shape[2], width=x.shape[3]), wm, model=model)
                _patch_explainer(ex, x[b:b + 1].astype(np.float64 if dtype == torch.float64 else np.float32), caps[b])
                orig = aoa.ExplainAOAAttention.explain_caption_wordt
                for n, hd in enumerate(HEADS):
                    feats = []

                    def wrapped(t, head_idx, feats=feats):
                        rf, rw = orig(ex, t, head_idx)
                        feats.append(rf.clone())
                        return rf, rw
                    ex.explain_caption_wordt = wrapped
                    maps, rws = ex.explain_caption("synthetic.jpg", hd)
                    assert ex.image_features.dtype == dtype and maps[0].dtype == dtype and ex.num_pixels == 12
                    tag = "" if n == 0 else "h1_"
                    one[tag + "r_feat"] = np.stack([f.detach().numpy()[0] for f in feats])
                    rw = np.zeros((T, T), one[tag + "r_feat"].dtype)
                    for t in range(T):
                        rw[t, :t + 1] = rws[t].detach().numpy()
                    one[tag + "r_words"] = rw
                    if n == 0:
                        one["maps"] = np.stack([m.detach().numpy()[0] for m in maps])
            one["features"] = ex.image_features.detach().numpy()[0]
            for k in TRACE:
                v = getattr(ex, k).detach()
                one["tr_" + k] = (v[:, ::97] if k == "predictions" else v).numpy()
            for k, v in one.items():
                out.setdefault(k, []).append(v)
        return {k: np.stack(v) for k, v in out.items()}
    finally:
        torch.set_default_dtype(old)
        rn.resnet101 = real


F64 = ("r_feat", "r_words", "maps", "h1_r_feat", "h1_r_words")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-seed", type=int, default=0)
    first = ap.parse_args().first_seed
    install_stubs()
    weights = load_pkg()
    import models.aoamodel as aoa
    import models.resnet as rn
    fx = np.load(os.path.join(HERE, "resnet_engine.npz"))
    x, net_seed = fx["x"], int(fx["seed"])
    for seed in range(first, first + 64):
        caps = weights.make_captions(seed + 1, x.shape[0], T, V)
        r32 = run(aoa, rn, weights, net_seed, seed, x, caps, torch.float32)
        r64 = run(aoa, rn, weights, net_seed, seed, x, caps, torch.float64)
        e32 = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max() / np.abs(r64[k]).max()) for k in r32}
        e32["maps"] = max(float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())
                          for a, b in zip(r32["maps"].reshape(-1, *x.shape[1:]), r64["maps"].reshape(-1, *x.shape[1:])))   # per map
        print("decoder / caption seed %d: e32 %s" % (seed, ", ".join("%s %.2e" % kv for kv in sorted(e32.items()))), flush=True)
        if max(e32["r_feat"], e32["h1_r_feat"], e32["maps"]) < 1e-5 and max(e32["r_words"], e32["h1_r_words"]) < 3e-6:
            g = dict(net_seed=np.int64(net_seed), decoder_seed=np.int64(seed), caption_seed=np.int64(seed + 1), V=np.int64(V), caption=caps,
                     heads=np.array(HEADS, np.int64))
            g.update({k: v.astype(np.float32) for k, v in r32.items()})
            g.update({k + "64": r64[k] for k in F64})
            g.update({"e32_" + k: np.float64(v) for k, v in e32.items()})
            path = os.path.join(HERE, "aoa_resnet.npz")
            np.savez_compressed(path, **g)
            print("aoa_resnet.npz:", os.path.getsize(path), "bytes on disk;", {k: np.asarray(v).shape for k, v in g.items()})
            return
    raise SystemExit("no decoder / caption seed met the e32 conditions")


if __name__ == "__main__":
    main()
