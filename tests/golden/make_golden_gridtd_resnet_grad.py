#!/usr/bin/env python3
"""Golden vectors of the gridTD gradient explainers on a bottleneck ResNet encoder: the REFERENCE's
`ExplainGridTDGradient`, `ExplainiGridTDGuidedGradient` and `ExplainGridTDGradCam` (models/gridTDmodel.py:1214-1771) on the set-up of
make_golden_gridtd_resnet.py - `models.resnet.resnet101` rebound to a small net (base 12, blocks [1, 2, 1]: 192 feature channels),
`AdaptiveAttention(512, 12)` in place of the fixed 196 pixels, 2 x 3 x 45 x 51 images, a T = 3 word caption per image - once in fp32
and once with float64 as the default dtype.  The net and the images are those of resnet_grad.npz's `engine` set (`grad_net`: the
BatchNorms that feed an Add redrawn, so the Add ReLUs cut; its stored seed and x), whose forward already meets the ReLU / pool margins
of make_golden_resnet_grad.py - they depend on the forward alone and are recomputed and stored here.  The decoder / caption seed is
searched from --first-seed until the reference's fp32 is within 1e-5 of its fp64 on every stored quantity.  Writes
tests/golden/gridtd_resnet_grad.npz - arrays only:

  caption (B, T+1); d_feat_plain64 / d_feat_guided64 (B, T, C, h, w), the decoder gradients `explain_caption_wordt` returns (the
  Grad-CAM class runs the plain decoder: its d_feat is asserted equal); r_words_plain64 / r_words_guided64 (B, T, T), row t holds
  t + 1 entries; maps_plain64 / maps_guided64 (B, T, 3, H, W); cams64 (B, T, P); e32_<quantity> = the worst
  max |fp32 - fp64| / max |fp64| over the (image, word) rows (the fp32 arrays themselves would take the file past the size limit of a
  committed fixture); relu_margin, pool_margin; net_seed, decoder_seed, caption_seed, V.

    python tests/golden/make_golden_gridtd_resnet_grad.py

`ExplainGridTDGuidedGradCam` is left out: the reference cannot run it on a ResNet - it expands the cam with a fixed upscale = 16
(:1826), which is not the image's size at stride 32, and `expand_as` fails.  Same harness shims as make_golden.py; run where the
reference is available only."""
import argparse
import os
import tempfile

import numpy as np
import torch

from make_golden import _patch_explainer, install_stubs, load_pkg, make_args
from make_golden_gridtd_resnet import NET, PREFIX, T, V
from make_golden_resnet_grad import MARGIN, NETS, grad_net, margins

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = (("plain", "ExplainGridTDGradient"), ("guided", "ExplainiGridTDGuidedGradient"), ("cam", "ExplainGridTDGradCam"))


def run(gtd, rn, weights, net_seed, dec_seed, x, caps, dtype):
    """the three explainers on every image of x -> {name: (B, ...) array}"""
    small_net = lambda pretrained=True, **kw: _with_feat_dim(grad_net(net_seed, rn.Add, NETS["engine"]))
    real_load, real_resnet = torch.load, rn.resnet101
    sd = {k: torch.from_numpy(v.copy()) for k, v in weights.make_gridtd_resnet_state(
        seed=dec_seed, vocab_size=V, feat_dim=NET["feat_dim"], num_pixels=NET["num_pixels"]).items()}
    sd.update({PREFIX + k: v for k, v in small_net().state_dict().items()})

    def load_small(model, state):                # the classes build their own model and load args.weight (:1221-1223): the attention
        model.AdaAttention = gtd.AdaptiveAttention(512, NET["num_pixels"])          # of 12 pixels goes in just before the state does
        return torch.nn.Module.load_state_dict(model, state)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    rn.resnet101, gtd.GridTDModel.load_state_dict, torch.load = small_net, load_small, lambda *a, **k: {"state_dict": sd}
    try:
        wm = weights.make_word_map(V)
        out = {}
        for b in range(x.shape[0]):
            one = {}
            for tag, cls in CLASSES:
                with tempfile.TemporaryDirectory() as tmp:
                    ex = getattr(gtd, cls)(make_args(tmp, encoder='resnet101', height=x.shape[2], width=x.shape[3]), wm)
                    ex.model = ex.model.to(dtype).eval()
                    _patch_explainer(ex, x[b:b + 1].astype(np.float64 if dtype == torch.float64 else np.float32), caps[b])
                    feats = []
                    orig = ex.explain_caption_wordt

                    def wrapped(t, orig=orig, feats=feats):
                        rf, rw = orig(t)
                        feats.append(rf.detach().clone())
                        return rf, rw
                    ex.explain_caption_wordt = wrapped
                    maps, rws = ex.explain_caption("synthetic.jpg")
                assert ex.image_features.dtype == dtype and maps[0].dtype == dtype and ex.num_pixels == NET["num_pixels"]
                d_feat = np.stack([f.numpy()[0] for f in feats])
                rw = np.zeros((T, T), d_feat.dtype)
                for t in range(T):
                    rw[t, :t + 1] = rws[t].detach().numpy()
                if tag == "cam":
                    assert np.array_equal(d_feat, one["d_feat_plain"]) and np.array_equal(rw, one["r_words_plain"])
                    one["cams"] = np.stack([m.detach().numpy().reshape(-1) for m in maps])
                else:
                    one["d_feat_" + tag], one["r_words_" + tag] = d_feat, rw
                    one["maps_" + tag] = np.stack([m.detach().numpy()[0] for m in maps])
            for k, v in one.items():
                out.setdefault(k, []).append(v)
        return {k: np.stack(v) for k, v in out.items()}
    finally:
        torch.set_default_dtype(old)
        rn.resnet101, torch.load = real_resnet, real_load
        del gtd.GridTDModel.load_state_dict


def _with_feat_dim(net):
    net.feat_dim = NET["feat_dim"]
    return net


def worst_row(a32, a64):
    """max over the (image, word) rows of max |fp32 - fp64| / max |fp64| (a row of r_words is normalised: its maximum is 1)"""
    rows32, rows64 = a32.reshape((-1,) + a32.shape[2:]), a64.reshape((-1,) + a64.shape[2:])
    return max(float(np.abs(p.astype(np.float64) - q).max() / max(np.abs(q).max(), 1e-300)) for p, q in zip(rows32, rows64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-seed", type=int, default=0)
    first = ap.parse_args().first_seed
    install_stubs()
    weights = load_pkg()
    import models.gridTDmodel as gtd
    import models.resnet as rn
    fx = np.load(os.path.join(HERE, "resnet_grad.npz"))
    x, net_seed = fx["engine_x"], int(fx["engine_seed"])
    relu_m, pool_m = margins(grad_net(net_seed, rn.Add, NETS["engine"]).double(), torch.from_numpy(x).double())
    assert relu_m >= MARGIN and pool_m >= MARGIN, (relu_m, pool_m)
    for seed in range(first, first + 64):
        caps = weights.make_captions(seed + 1, x.shape[0], T, V)
        r32 = run(gtd, rn, weights, net_seed, seed, x, caps, torch.float32)
        r64 = run(gtd, rn, weights, net_seed, seed, x, caps, torch.float64)
        e32 = {k: worst_row(r32[k], r64[k]) for k in r32}
        print("decoder / caption seed %d: e32 %s" % (seed, ", ".join("%s %.2e" % kv for kv in sorted(e32.items()))), flush=True)
        if max(e32.values()) < 1e-5:
            g = dict(net_seed=np.int64(net_seed), decoder_seed=np.int64(seed), caption_seed=np.int64(seed + 1), V=np.int64(V), caption=caps,
                     relu_margin=np.float64(relu_m), pool_margin=np.float64(pool_m))
            g.update({k + "64": v for k, v in r64.items()})
            g.update({"e32_" + k: np.float64(v) for k, v in e32.items()})
            path = os.path.join(HERE, "gridtd_resnet_grad.npz")
            np.savez_compressed(path, **g)
            print("gridtd_resnet_grad.npz:", os.path.getsize(path), "bytes on disk;", {k: np.asarray(v).shape for k, v in g.items()})
            return
    raise SystemExit("no decoder / caption seed met e32 < 1e-5")


if __name__ == "__main__":
    main()
