#!/usr/bin/env python3
"""Output digests of the runtime-geometry conv engine's entries (lrpx_conv_geom, _ex, _ex_b6, _ab, _ab_b6 and the two packers;
csrc/conv_geom_kernel.h) at the edges of its tiling, recorded once from a build whose bytes are to be kept - tests/test_gpu_conv_geom_bytes.py
runs the same cases on the build at hand and requires every sha256 to be the recorded one.  Writes tests/golden/conv_geom_bytes.json:
digests only, with the commit the recorded library was built from.

    LRPX_LIB_PATH=<liblrpx.so of that commit> python tests/golden/make_golden_conv_geom_bytes.py --commit <its hash>

Needs a GPU.  Per shape = geometry x K x n_oc the inputs are drawn on the CPU from one seeded torch.Generator; their digest is stored
too, so that a changed draw is told apart from a changed kernel.

Geometries (kernel, stride, padding) on an 11 x 9 input map (odd, not square: the stride-2 classes differ in size, and the 1x1 stride-2
conv has classes no tap reaches); contraction channels K (kr of the alpha-beta entries) 4 (below one chunk), 36, 52 (no multiples of 32,
the W+ / W- boundary inside a chunk); n_oc 4 (one partial column block), 36 (the second wave column partial), 72 (blockIdx.y = 1 and a
wave whose columns lie wholly beyond n_oc).  Transposed direction: three maps on two images, map2img [1, 0, 1] - 3 Hc Wc pixels per
class, never a multiple of 64 - or, without map2img, two maps on two images; forward direction: two images.  Every output buffer is
pre-filled with one fixed bit pattern."""
import argparse
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
JSON = os.path.join(HERE, "conv_geom_bytes.json")
GEOMS = {"pw": (1, 1, 0), "pws2": (1, 2, 0), "c3": (3, 1, 1), "c3s2": (3, 2, 1), "c7s2": (7, 2, 3)}       # (kernel, stride, padding)
KS, N_OCS, HW = (4, 36, 52), (4, 36, 72), (11, 9)
N_IMG, N_MAPS, MAP2IMG = 2, 3, [1, 0, 1]
PACK_SHAPE = (52, 36)                    # (K, n_oc) whose packed images are digested, per geometry
FILL = 0x7FC12345                        # a NaN: what a launch leaves unwritten shows in the digest
SHAPES = [("%s_%d_%d" % (gname, k, n_oc), g, k, n_oc) for gname, g in GEOMS.items() for k in KS for n_oc in N_OCS]


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def inputs(name, geom, k, n_oc):
    """the CPU tensors of one shape, NHWC rows: FWD contracts k input channels into n_oc, BWD k = cout channels into n_oc = cin"""
    ksz, s, p = geom
    (h, w), oh, ow = HW, (HW[0] + 2 * p - ksz) // s + 1, (HW[1] + 2 * p - ksz) // s + 1
    g = torch.Generator().manual_seed(9000 + 131 * ksz + 17 * s + 3 * k + n_oc)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    c = dict(name=name, geom=(ksz, ksz, s, s, p, p), k=k, n_oc=n_oc, hw=(h, w), ohw=(oh, ow))
    c["w_fwd"] = rn(n_oc, k, ksz, ksz)                              # (cout, cin, kh, kw)
    c["x_fwd"], c["bias"] = rn(N_IMG, h * w, k), rn(n_oc)
    w_bwd = rn(k, n_oc, ksz, ksz)
    c["w_bwd"], c["w_dual"] = w_bwd, torch.cat([w_bwd.clamp(min=0), w_bwd.clamp(max=0)], 0)      # the rows [W+ ; W-]
    c["r"], c["x"], c["addend"] = rn(N_MAPS, oh * ow, k), rn(N_IMG, h * w, n_oc), rn(N_MAPS, h * w, n_oc)
    c["q"] = torch.rand(N_IMG, oh * ow, k, generator=g) + 0.5
    c["q2"] = -(torch.rand(N_IMG, oh * ow, k, generator=g) + 0.5)
    c["digest"] = sha(*(c[n] for n in ("w_fwd", "x_fwd", "bias", "w_bwd", "r", "x", "addend", "q", "q2")))
    return c


def run_shape(c, ops, _lib):
    """{case: sha256 of the output bytes} of every entry on one shape, in a fixed order"""
    d = {n: c[n].cuda() for n in ("w_fwd", "x_fwd", "bias", "w_bwd", "w_dual", "r", "x", "addend", "q", "q2")}
    m2i = torch.tensor(MAP2IMG, dtype=torch.int32, device="cuda")
    (h, w), (oh, ow), k, n_oc, geom = c["hw"], c["ohw"], c["k"], c["n_oc"], c["geom"]
    F, B = _lib.GEOM_FWD, _lib.GEOM_BWD
    res = {}

    def out(n, pix):
        return torch.full((n * pix * n_oc,), FILL, dtype=torch.int32, device="cuda").view(torch.float32).view(n, pix, n_oc)
    packs = {}
    for b6, pack in ((False, ops.conv_geom_pack), (True, ops.conv_geom_pack_bf16x3)):
        packs[b6] = {"fwd": pack(d["w_fwd"], F), "bwd": pack(d["w_bwd"], B), "dual": pack(d["w_dual"], B)}
        if (k, n_oc) == PACK_SHAPE:
            res["pack%s_fwd" % ("_b6" if b6 else "")] = sha(packs[b6]["fwd"])
            res["pack%s_bwd" % ("_b6" if b6 else "")] = sha(packs[b6]["bwd"])
    pk = packs[False]
    res["geom_fwd_bias"] = sha(ops.conv_geom(d["x_fwd"], pk["fwd"], F, N_IMG, (h, w), (oh, ow), geom, k, n_oc, bias=d["bias"], out=out(N_IMG, oh * ow)))
    res["geom_fwd"] = sha(ops.conv_geom(d["x_fwd"], pk["fwd"], F, N_IMG, (h, w), (oh, ow), geom, k, n_oc, out=out(N_IMG, oh * ow)))
    res["geom_bwd"] = sha(ops.conv_geom(d["r"][:N_IMG].contiguous(), pk["bwd"], B, N_IMG, (h, w), (oh, ow), geom, k, n_oc, x=d["x"],
                                        out=out(N_IMG, h * w)))
    for b6 in (False, True):
        tag, pk = ("_b6" if b6 else ""), packs[b6]
        res["ex%s_fwd_bias" % tag] = sha(ops.conv_geom_ex(d["x_fwd"], pk["fwd"], F, N_IMG, (h, w), (oh, ow), geom, k, n_oc, bias=d["bias"],
                                                          out=out(N_IMG, oh * ow), b6=b6))
        for use_q in (False, True):
            for use_add in (False, True):
                for use_m2i in (False, True):
                    n = N_MAPS if use_m2i else N_IMG
                    got = ops.conv_geom_ex(d["r"][:n].contiguous(), pk["bwd"], B, n, (h, w), (oh, ow), geom, k, n_oc, x=d["x"],
                                           q=d["q"] if use_q else None, addend=d["addend"][:n].contiguous() if use_add else None,
                                           map2img=m2i if use_m2i else None, n_img=N_IMG, out=out(n, h * w), b6=b6)
                    res["ex%s_bwd_q%d_add%d_m2i%d" % (tag, use_q, use_add, use_m2i)] = sha(got)
        for use_add in (False, True):
            add = d["addend"] if use_add else None
            kw = dict(addend=add, map2img=m2i, n_img=N_IMG, b6=b6)
            for scale in (1., 2.):
                got = ops.conv_geom_ab(d["r"], pk["bwd"], N_MAPS, (h, w), (oh, ow), geom, k, n_oc, d["x"], d["q"], scale=scale,
                                       out=out(N_MAPS, h * w), **kw)
                res["ab%s_single_s%g_add%d" % (tag, scale, use_add)] = sha(got)
            got = ops.conv_geom_ab(d["r"], pk["dual"], N_MAPS, (h, w), (oh, ow), geom, k, n_oc, d["x"], d["q"], q2=d["q2"], scale=2., scale2=-1.,
                                   out=out(N_MAPS, h * w), **kw)
            res["ab%s_dual_add%d" % (tag, use_add)] = sha(got)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under LRPX_LIB_PATH was built from")
    ap.add_argument("--out", default=JSON)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lrp_amd  # noqa: F401
    from lrp_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_conv_geom_bytes: needs a GPU")
    g = {"recorded_from_commit": a.commit, "fill": "0x%08X" % FILL, "shapes": {}}
    for name, geom, k, n_oc in SHAPES:
        c = inputs(name, geom, k, n_oc)
        g["shapes"][name] = {"inputs": c["digest"], "outputs": run_shape(c, ops, _lib)}
    with open(a.out, "w") as f:
        json.dump(g, f, indent=0, sort_keys=True)
        f.write("\n")
    print(os.path.basename(a.out) + ":", os.path.getsize(a.out), "bytes;", len(SHAPES), "shapes,",
          sum(len(s["outputs"]) for s in g["shapes"].values()), "digests, library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
