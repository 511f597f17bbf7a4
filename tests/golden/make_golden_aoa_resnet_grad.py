#!/usr/bin/env python3
"""Golden vectors of the AoA gradient explainers on a bottleneck ResNet encoder: the REFERENCE's `ExplainAOAGradient`,
`ExplainAOAGuidedGradient` and `ExplainAOAGradCam` (models/aoamodel.py:1257-1711), head HEAD, on the set-up of make_golden_aoa_resnet.py
- `models.resnet.resnet101` rebound to a small net (base 12, blocks [1, 2, 1]: 192 feature channels), 2 x 3 x 45 x 51 images, a
T = 3 word caption per image - once in fp32 and once with float64 as the default dtype.  The net and the images are those of
resnet_grad.npz's `engine` set (`grad_net`: the BatchNorms that feed an Add redrawn, so the Add ReLUs cut; its stored seed and x),
whose forward already meets the ReLU / pool margins of make_golden_resnet_grad.py - they depend on the forward alone and are asserted
and stored again here.  The decoder / caption seed is searched from --first-seed until the reference's fp32 is within 1e-5 of its fp64
on every stored quantity.  Writes tests/golden/aoa_resnet_grad.npz - arrays only:

  caption (B, T+1); head; d_img_feature64 (B, T, C, h, w), the decoder gradient `explain_caption_wordt` returns (all three classes
  run the same decoder: asserted equal); r_words64 (B, T, T), row t holds t + 1 entries; maps_plain64 / maps_guided64
  (B, T, 3, H, W); cams64 (B, T, P); e32_<quantity> = the worst max |fp32 - fp64| / max |fp64| over the (image, word) rows (the fp32
  arrays themselves would take the file past the size limit of a committed fixture); relu_margin, pool_margin; hook_vs_stem /
  hook_vs_all / hook_vs_plain: the reference's hook path (`ExplainAOAGuidedGradient.register_hooks`, :1596-1613, on a deep copy as its
  `explain_cnn` does) against the autograd restatements of make_golden_resnet_grad.chain, worst max |difference| / max |hook path|
  over the (image, word) rows in fp64; net_seed, decoder_seed, caption_seed, V.

    python tests/golden/make_golden_aoa_resnet_grad.py

`ExplainAOAGuidedGradCam` is left out: the reference cannot run it on a ResNet - it expands the cam with a fixed upscale = 16 (:1743),
which is not the image's size at stride 32, and `expand_as` fails; `guided_gradcam_fails` below runs the class and returns the error it
raises (printed by main; scikit-image's one call is served by the oracle's restatement as in make_golden.gen_guided_gradcam).  Same
harness shims as make_golden.py; run where the reference is available only."""
import argparse
import copy
import os
import sys
import tempfile

import numpy as np
import torch

from make_golden import _patch_explainer, install_stubs, load_pkg, make_args
from make_golden_aoa_resnet import NET, T, V, aoa_state, with_feat_dim
from make_golden_gridtd_resnet_grad import worst_row
from make_golden_resnet_grad import MARGIN, NETS, chain, grad_net, margins

HERE = os.path.dirname(os.path.abspath(__file__))
HEAD = 5
CLASSES = (("plain", "ExplainAOAGradient"), ("guided", "ExplainAOAGuidedGradient"), ("cam", "ExplainAOAGradCam"))


def explainers(aoa, rn, weights, net_seed, dec_seed, x, caps, dtype, classes):
    """yields (image, tag, explainer) for the classes on every image, models.resnet.resnet101 and torch.load rebound for the call"""
    small_net = lambda pretrained=True, **kw: with_feat_dim(grad_net(net_seed, rn.Add, NETS["engine"]))
    real_load, real_resnet = torch.load, rn.resnet101
    sd = aoa_state(weights, dec_seed, small_net())
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    rn.resnet101, torch.load = small_net, lambda *a, **k: {"state_dict": sd}
    try:
        wm = weights.make_word_map(V)
        for b in range(x.shape[0]):
            for tag, cls in classes:
                with tempfile.TemporaryDirectory() as tmp:
                    ex = getattr(aoa, cls)(make_args(tmp, encoder='resnet101', height=x.shape[2], width=x.shape[3]), wm)
                    ex.model = ex.model.to(dtype).eval()
                    _patch_explainer(ex, x[b:b + 1].astype(np.float64 if dtype == torch.float64 else np.float32), caps[b])
                    yield b, tag, ex
    finally:
        torch.set_default_dtype(old)
        rn.resnet101, torch.load = real_resnet, real_load


def run(aoa, rn, weights, net_seed, dec_seed, x, caps, dtype):
    """the three explainers on every image of x -> {name: (B, ...) array}"""
    out, one = {}, {}
    for b, tag, ex in explainers(aoa, rn, weights, net_seed, dec_seed, x, caps, dtype, CLASSES):
        feats = []
        orig = ex.explain_caption_wordt

        def wrapped(t, head_idx, orig=orig, feats=feats):
            rf, rw = orig(t, head_idx)
            feats.append(rf.detach().clone())
            return rf, rw
        ex.explain_caption_wordt = wrapped
        maps, rws = ex.explain_caption("synthetic.jpg", HEAD)
        assert ex.image_features.dtype == dtype and maps[0].dtype == dtype and ex.num_pixels == 12
        d_feat = np.stack([f.numpy()[0] for f in feats])
        rw = np.zeros((T, T), d_feat.dtype)
        for t in range(T):
            rw[t, :t + 1] = rws[t].detach().numpy()
        if tag == "plain":
            one = {"d_img_feature": d_feat, "r_words": rw}
        else:
            assert np.array_equal(d_feat, one["d_img_feature"]) and np.array_equal(rw, one["r_words"])
        if tag == "cam":
            one["cams"] = np.stack([m.detach().numpy().reshape(-1) for m in maps])
            for k, v in one.items():
                out.setdefault(k, []).append(v)
        else:
            one["maps_" + tag] = np.stack([m.detach().numpy()[0] for m in maps])
    return {k: np.stack(v) for k, v in out.items()}


def hook_distances(aoa, net64, x, d_feat64):
    """the reference's hook path on every (image, word) row against the stem-only, every-ReLU and plain restatements (fp64)"""
    worst = {"stem": 0., "all": 0., "plain": 0.}
    hooked = 0
    for b in range(d_feat64.shape[0]):
        xs = torch.from_numpy(x[b:b + 1]).double()
        for t in range(d_feat64.shape[1]):
            g = torch.from_numpy(d_feat64[b, t][None])
            enc = copy.deepcopy(net64)                                   # explain_cnn, models/aoamodel.py:1621-1640
            enc.zero_grad()
            aoa.ExplainAOAGuidedGradient.register_hooks(None, enc)
            hooked = sum(1 for m in enc.modules() if isinstance(m, torch.nn.ReLU) and m._backward_hooks)
            sample = xs.clone()
            sample.requires_grad = True
            with torch.enable_grad():
                enc(sample).backward(g.clone(), retain_graph=True)
            ref = sample.grad.detach().clone()
            for k, relus in (("stem", "stem"), ("all", "all"), ("plain", None)):
                worst[k] = max(worst[k], ((chain(net64, xs, g, relus) - ref).abs().max() / ref.abs().max()).item())
    n_relu = sum(1 for m in net64.modules() if isinstance(m, torch.nn.ReLU))
    return worst, hooked, n_relu


def guided_gradcam_fails(aoa, rn, weights, net_seed, dec_seed, x, caps):
    """runs the reference's ExplainAOAGuidedGradCam on the first image; returns the exception it raises (None: it ran)"""
    from oracle import lrp_oracle as O
    expand = lambda a, upscale=2, multichannel=False, **kw: O.pyramid_expand(torch.from_numpy(np.asarray(a)), upscale).double().numpy()
    sys.modules["skimage.transform"].pyramid_expand = expand
    sys.modules["skimage"].transform = sys.modules["skimage.transform"]
    for b, tag, ex in explainers(aoa, rn, weights, net_seed, dec_seed, x[:1], caps, torch.float32, (("ggc", "ExplainAOAGuidedGradCam"),)):
        try:
            ex.explain_caption("synthetic.jpg", HEAD)
        except Exception as e:      # noqa: BLE001  (whatever the reference raises is the finding)
            return e
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-seed", type=int, default=0)
    first = ap.parse_args().first_seed
    install_stubs()
    weights = load_pkg()
    import models.aoamodel as aoa
    import models.resnet as rn
    fx = np.load(os.path.join(HERE, "resnet_grad.npz"))
    x, net_seed = fx["engine_x"], int(fx["engine_seed"])
    net64 = grad_net(net_seed, rn.Add, NETS["engine"]).double().eval()
    relu_m, pool_m = margins(net64, torch.from_numpy(x).double())
    assert relu_m >= MARGIN and pool_m >= MARGIN, (relu_m, pool_m)
    for seed in range(first, first + 64):
        caps = weights.make_captions(seed + 1, x.shape[0], T, V)
        r32 = run(aoa, rn, weights, net_seed, seed, x, caps, torch.float32)
        r64 = run(aoa, rn, weights, net_seed, seed, x, caps, torch.float64)
        e32 = {k: worst_row(r32[k], r64[k]) for k in r32}
        print("decoder / caption seed %d: e32 %s" % (seed, ", ".join("%s %.2e" % kv for kv in sorted(e32.items()))), flush=True)
        if max(e32.values()) < 1e-5:
            hook, hooked, n_relu = hook_distances(aoa, net64, x, r64["d_img_feature"])
            print("register_hooks hooks %d of %d ReLU modules; hook path against stem-only %.2e, every ReLU %.2e, plain %.2e" % (
                hooked, n_relu, hook["stem"], hook["all"], hook["plain"]))
            err = guided_gradcam_fails(aoa, rn, weights, net_seed, seed, x, caps)
            print("ExplainAOAGuidedGradCam on this set-up: %s" % ("ran" if err is None else "%s: %s" % (type(err).__name__, err)))
            g = dict(net_seed=np.int64(net_seed), decoder_seed=np.int64(seed), caption_seed=np.int64(seed + 1), V=np.int64(V), caption=caps,
                     head=np.int64(HEAD), relu_margin=np.float64(relu_m), pool_margin=np.float64(pool_m))
            g.update({k + "64": v for k, v in r64.items()})
            g.update({"e32_" + k: np.float64(v) for k, v in e32.items()})
            g.update({"hook_vs_" + k: np.float64(v) for k, v in hook.items()})
            path = os.path.join(HERE, "aoa_resnet_grad.npz")
            np.savez_compressed(path, **g)
            print("aoa_resnet_grad.npz:", os.path.getsize(path), "bytes on disk;", {k: np.asarray(v).shape for k, v in g.items()})
            return
    raise SystemExit("no decoder / caption seed met e32 < 1e-5")


if __name__ == "__main__":
    main()
