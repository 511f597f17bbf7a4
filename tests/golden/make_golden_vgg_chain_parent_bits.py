#!/usr/bin/env python3
"""Bits of the VGG16 chains of csrc/lrpx_vgg.hip - forward trace, relevance, gradient, guided backprop - in every conv mode, for seeded
inputs, recorded once from a build whose bits are to be kept: tests/test_gpu_vgg_chain_parent_bits.py runs the same cases on the build
at hand and requires the same bits.  Writes tests/golden/vgg_chain_parent_bits.json.

    LRPX_LIB_PATH=<liblrpx.so of that commit> python tests/golden/make_golden_vgg_chain_parent_bits.py --commit <its hash>

Needs a GPU.  One Vgg16 context (seeded weights with non-zero biases), two seeded 224 x 224 images - the only size the chains are built
for.  CONFIGS: conv modes 0 - 3 through the context's conv_mode, modes 2 and 3 with forward_f16 = 1 as well (six traces), and mode 1 a
second time with lrpx_set_b6_wino(0), where the direct kernels and the K-split detour of the 14 x 14 relevance layers run instead of
the Winograd kernel.  Per config: the features and every tensor of trace_views(), then relevance, gradient and guided_backprop for the
three MAPSETS, the smallest that reach every branch of the flows:

    none    map2img = None, two maps (the null-pointer path)
    group2  [0, 0, 1, 1]             (tile group 2)
    odd     [1, 0, 1]                (n_maps % n_img != 0: tile group off)

and the relevance of `group2` once more through layer_ms: the layers with a non-zero time.  Every case runs twice; one that the
recording build does not repeat is left out and named (none is expected: these chains have no atomics other than maxima).  Stored: a
sha256 of the seeded inputs (a changed CPU draw is told apart from a changed library) and the sha256 of every output's bytes."""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
JSON = os.path.join(HERE, "vgg_chain_parent_bits.json")
SEED = 29

# (name, conv_mode, forward_f16, lrpx_set_b6_wino mask or None for the default)
CONFIGS = [("mode0", 0, 0, None), ("mode1", 1, 0, None), ("mode1_direct", 1, 0, 0), ("mode2", 2, 0, None), ("mode2_f16", 2, 1, None),
           ("mode3", 3, 0, None), ("mode3_f16", 3, 1, None)]
MAPSETS = [("none", None), ("group2", [0, 0, 1, 1]), ("odd", [1, 0, 1])]
CHAINS = ("relevance", "gradient", "guided_backprop")
TIMED = "group2"


def config_name(cfg):
    return cfg[0]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_INPUTS = {}


def inputs():
    """CPU tensors, drawn once: dict(w, b, img, feat[mapset]: (n_maps, 196, 512) at the encoder output, digest)"""
    if not _INPUTS:
        from lrp_amd import weights
        sd = weights.make_gridtd_state(seed=SEED, vocab_size=16, vgg_bias_std=0.05)
        names = [k for k in sd if k.startswith("img_encoder.encoder.") and k.endswith(".weight")]
        _INPUTS["w"] = [torch.from_numpy(sd[k]) for k in names]
        _INPUTS["b"] = [torch.from_numpy(sd[k.replace(".weight", ".bias")]) for k in names]
        _INPUTS["img"] = torch.from_numpy(weights.make_images(SEED + 1, 2))
        g = torch.Generator().manual_seed(SEED + 2)
        _INPUTS["feat"] = {n: torch.randn(2 if m is None else len(m), 196, 512, generator=g) for n, m in MAPSETS}
        h = hashlib.sha256()
        for t in _INPUTS["w"] + _INPUTS["b"] + [_INPUTS["img"]] + [_INPUTS["feat"][n] for n, _ in MAPSETS]:
            h.update(t.contiguous().numpy().tobytes())
        _INPUTS["digest"] = h.hexdigest()
    return _INPUTS


def context(ops):
    d = inputs()
    return ops.Vgg16([w.cuda() for w in d["w"]], [b.cuda() for b in d["b"]])


def run(ops, vgg, cfg):
    """every case of one config, each twice -> ({case: sha256}, [cases whose second run gave other bits; "trace": the forward's],
    [layers with a time]); a chain output that is not finite everywhere is an error"""
    _, mode, f16, wino = cfg
    d = inputs()
    vgg.conv_mode, vgg.forward_f16 = mode, f16
    prev = ops.set_b6_wino(wino) if wino is not None else None
    out, unstable = {}, []
    try:
        img = d["img"].cuda()
        feats = vgg.forward(img)
        torch.cuda.synchronize()
        acts, zs = vgg.trace_views()
        out["features"] = sha(feats)
        for l, t in enumerate(acts):
            out["act%d" % l] = sha(t)
        for l, t in enumerate(zs):
            if t is not None:
                out["zpos%d" % l] = sha(t)
        first = vgg.trace.clone()
        vgg.forward(img)
        torch.cuda.synchronize()
        if not same_bits(first, vgg.trace):
            unstable.append("trace")
        del first
        timed_layers = None
        for ms_name, m2i in MAPSETS:
            m = None if m2i is None else torch.tensor(m2i, dtype=torch.int32, device="cuda")
            feat = d["feat"][ms_name].cuda()
            for chain in CHAINS:
                # relevance enters the encoder where the features are: non-negative, like the decoders'
                x = feat.clamp(min=0) if chain == "relevance" else feat
                a = getattr(vgg, chain)(x, m).clone()
                b = getattr(vgg, chain)(x, m)
                torch.cuda.synchronize()
                key = "%s_%s" % (chain, ms_name)
                assert torch.isfinite(a).all() and a.abs().max() > 0, (cfg[0], key)
                out[key] = sha(a)
                if not same_bits(a, b):
                    unstable.append(key)
                if chain == "relevance" and ms_name == TIMED:
                    ms = (C.c_float * 17)()
                    t = vgg.relevance(x, m, layer_ms=ms)
                    torch.cuda.synchronize()
                    if not same_bits(a, t):
                        unstable.append(key + "_timed")
                    timed_layers = [l for l in range(17) if ms[l] != 0.0]
    finally:
        if prev is not None:
            ops.set_b6_wino(prev)
        vgg.conv_mode = vgg.forward_f16 = None
    return out, unstable, timed_layers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under LRPX_LIB_PATH was built from")
    ap.add_argument("--out", default=JSON)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lrp_amd  # noqa: F401
    from lrp_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_vgg_chain_parent_bits: needs a GPU")
    vgg = context(ops)
    g = {"recorded_from_commit": a.commit, "inputs": inputs()["digest"], "configs": {}, "not_recorded": []}
    for cfg in CONFIGS:
        out, unstable, timed = run(ops, vgg, cfg)
        for k in unstable:                         # a case the recording build itself does not repeat proves nothing
            g["not_recorded"].append(config_name(cfg) + "/" + k)
            for name in [n for n in out if n == k or (k == "trace" and re.match(r"features|act|zpos", n))]:
                del out[name]
        g["configs"][config_name(cfg)] = {"sha256": out, "timed_layers": timed}
        print(config_name(cfg), len(out), "outputs, timed layers", timed, "not repeated:", unstable or "none", flush=True)
    with open(a.out, "w") as f:
        json.dump(g, f, indent=1, sort_keys=True)
        f.write("\n")
    print(os.path.basename(a.out) + ":", os.path.getsize(a.out), "bytes; library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
