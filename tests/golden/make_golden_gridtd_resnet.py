#!/usr/bin/env python3
"""Golden vectors of the gridTD LRP explainer on a bottleneck ResNet encoder: the REFERENCE's `GridTDModel('resnet101')` and its
`ExplainGridTDAttention.explain_caption` (models/gridTDmodel.py:23-37, :705-1156), with `models.resnet.resnet101` rebound to return the
small net of resnet_engine.npz (base 12, blocks [1, 2, 1], that fixture's seed: 192 feature channels) and `AdaAttention` replaced by
`AdaptiveAttention(512, 12)` before the state is loaded (the reference fixes 196 pixels, :127; the 2 x 3 x 45 x 51 images of
resnet_engine.npz give a 3 x 4 feature map).  Per image a T = 3 word caption, once in fp32 and once on .double() copies (as
make_golden.gen_t20_f64: default dtype float64 for the call).  Writes tests/golden/gridtd_resnet.npz - arrays only:

  caption (B, T+1); features (B, C, h, w); tr_* (B, ...) the trace arrays make_golden.gen_gridtd stores (predictions every 97th word);
  r_feat / r_feat64 (B, T, C, h, w); r_words / r_words64 (B, T, T), row t holds t + 1 entries; maps / maps64 (B, T, 3, H, W), the
  running sums `explain_caption` returns; e32_<quantity> = max |fp32 - fp64| / max |fp64|; net_seed, decoder_seed, caption_seed.

    python tests/golden/make_golden_gridtd_resnet.py

The net's seed is the fixture's (its Add / pool conditioning depends on the forward alone and holds here as it does there).  The
decoder / caption seed is searched from --first-seed until e32 < 1e-5 on r_feat and on the maps, and stored.  One more condition on
the draw: e32 < 3e-6 on r_words.  The tests hold r_words to 1e-5 of the reference's fp32 values (tests/test_gpu_gridtd.py's bound);
r_words are sums of 512 signed terms divided by their largest, and on some draws the reference's own fp32 is 2.6e-5 from its fp64
there (seed 0) - a fixture on which the bound would measure the reference's rounding, not the engine's.  Same harness shims as
make_golden.py; run where the reference is available only."""
import argparse
import os
import tempfile

import numpy as np
import torch

from make_golden import _patch_explainer, install_stubs, load_pkg, make_args
from make_golden_resnet import bottleneck_net

HERE = os.path.dirname(os.path.abspath(__file__))
NET = dict(base=12, blocks=[1, 2, 1], feat_dim=192, num_pixels=12)
T, V = 3, 9586
PREFIX = "img_encoder.encoder."
TRACE = ("predictions", "alphas", "betas", "h1t", "c1t", "h2t", "c2t", "g1t", "g2t", "i1t_act", "f1t_act", "i2t_act", "f2t_act", "st",
         "context", "context_hat")


def run(gtd, rn, weights, net_seed, dec_seed, x, caps, dtype):
    """the reference's explainer on every image of x -> {name: (B, ...) array}"""
    def small_net(pretrained=True, **kw):
        net = bottleneck_net(np.random.RandomState(net_seed), rn.Add, NET["base"], NET["blocks"])
        net.feat_dim = NET["feat_dim"]
        return net
    rn.resnet101 = small_net
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        model = gtd.GridTDModel(512, 512, V, 'resnet101')
        model.AdaAttention = gtd.AdaptiveAttention(512, NET["num_pixels"])
        sd = {k: torch.from_numpy(v.copy()) for k, v in weights.make_gridtd_resnet_state(
            seed=dec_seed, vocab_size=V, feat_dim=NET["feat_dim"], num_pixels=NET["num_pixels"]).items()}
        sd.update({PREFIX + k: v for k, v in small_net().state_dict().items()})
        model.load_state_dict(sd)
        model = model.to(dtype).eval()
        wm = weights.make_word_map(V)
        out = {}
        for b in range(x.shape[0]):
            with tempfile.TemporaryDirectory() as tmp:
                ex = gtd.ExplainGridTDAttention(make_args(tmp, encoder='resnet101', height=x.shape[2], width=x.shape[3]), wm, model=model)
                _patch_explainer(ex, x[b:b + 1].astype(np.float64 if dtype == torch.float64 else np.float32), caps[b])
                feats = []
                orig = ex.explain_caption_wordt

                def wrapped(t, orig=orig, feats=feats):
                    rf, rw = orig(t)
                    feats.append(rf.clone())
                    return rf, rw
                ex.explain_caption_wordt = wrapped
                maps, rws = ex.explain_caption("synthetic.jpg")
            assert ex.image_features.dtype == dtype and maps[0].dtype == dtype
            one = {"features": ex.image_features.detach().numpy()[0]}
            for k in TRACE:
                v = getattr(ex, k).detach()
                one["tr_" + k] = (v[:, ::97] if k == "predictions" else v).numpy()
            one["r_feat"] = np.stack([f.detach().numpy()[0] for f in feats])
            rw = np.zeros((T, T), one["r_feat"].dtype)
            for t in range(T):
                rw[t, :t + 1] = rws[t].detach().numpy()
            one["r_words"] = rw
            one["maps"] = np.stack([m.detach().numpy()[0] for m in maps])
            for k, v in one.items():
                out.setdefault(k, []).append(v)
        return {k: np.stack(v) for k, v in out.items()}
    finally:
        torch.set_default_dtype(old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-seed", type=int, default=0)
    first = ap.parse_args().first_seed
    install_stubs()
    weights = load_pkg()
    import models.gridTDmodel as gtd
    import models.resnet as rn
    fx = np.load(os.path.join(HERE, "resnet_engine.npz"))
    x, net_seed = fx["x"], int(fx["seed"])
    for seed in range(first, first + 64):
        caps = weights.make_captions(seed + 1, x.shape[0], T, V)
        r32 = run(gtd, rn, weights, net_seed, seed, x, caps, torch.float32)
        r64 = run(gtd, rn, weights, net_seed, seed, x, caps, torch.float64)
        e32 = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max() / np.abs(r64[k]).max()) for k in r32}
        e_maps = max(float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())
                     for a, b in zip(r32["maps"].reshape(-1, *x.shape[1:]), r64["maps"].reshape(-1, *x.shape[1:])))
        e32["maps"] = e_maps                  # per map, as the tests bound it
        print("decoder / caption seed %d: e32 %s" % (seed, ", ".join("%s %.2e" % kv for kv in sorted(e32.items()))), flush=True)
        if e32["r_feat"] < 1e-5 and e32["maps"] < 1e-5 and e32["r_words"] < 3e-6:
            g = dict(net_seed=np.int64(net_seed), decoder_seed=np.int64(seed), caption_seed=np.int64(seed + 1), V=np.int64(V), caption=caps)
            g.update({k: v.astype(np.float32) for k, v in r32.items()})
            g.update({k + "64": r64[k] for k in ("r_feat", "r_words", "maps")})
            g.update({"e32_" + k: np.float64(v) for k, v in e32.items()})
            np.savez_compressed(os.path.join(HERE, "gridtd_resnet.npz"), **g)
            print("gridtd_resnet.npz:", sum(np.asarray(v).nbytes for v in g.values()), "bytes;", {k: np.asarray(v).shape for k, v in g.items()})
            return
    raise SystemExit("no decoder / caption seed met e32 < 1e-5")


if __name__ == "__main__":
    main()
