#!/usr/bin/env python3
"""Outputs of every conv-mode-1 kernel on the conv_f16x3.h tiling (the B6 rows of csrc/conv_kernels.def: relevance, pooled input, forward
DUAL and PLAIN, guided) for seeded CPU inputs, recorded once from a build whose bits are to be kept - tests/test_gpu_b6_ring_bits.py
runs the same cases on the build at hand and requires the same bits.  Writes tests/golden/b6_ring_parent_bits.json.

    LRPX_LIB_PATH=<liblrpx.so of that commit> python tests/golden/make_golden_b6_ring_parent_bits.py --commit <its hash>

Needs a GPU.  The kernels stream their weight fragments through a queue of 9 steps (taps) per 16-channel K-chunk, a few steps ahead of
the MFMAs; K = 16, 32 and 48 are one, two and three chunks (9 / 18 / 27 steps): the prologue alone, the wrap across a chunk boundary and
an odd number of chunks, each ending in the clamped tail.  The cases are the smallest that reach every row once:

    one or two maps; three where a 224-pixel tile straddles maps (28 x 28, 14 x 14)
    n_oc 64 (a 128-channel workgroup with two waves that own no channel block), 32 / 96 / 160 / 192 elsewhere
    pooled input: arg-max positions drawn uniformly, so every window position wins somewhere
    one relevance case with an Inf and a NaN in S

S is the signed heavy-tailed draw of tests/test_gpu_b6_wino.py, randn * exp(4 randn); x is ReLU'd; w * 0.05.  Stored per case: the row of
conv_kernels.def that ran, a sha256 of the inputs (a changed CPU draw is told apart from a changed kernel), a sha256 of the output bytes
and the first 16 channels of three sampled pixel rows (as the hex of their bytes), which say whether a changed output changed everywhere."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
JSON = os.path.join(HERE, "b6_ring_parent_bits.json")

# (row of conv_kernels.def, kind, hw, map2img, K, n_oc); kind: rel / pool / fwd / plain / guided / pool_guided, "+nan": an Inf and a NaN in S
CASES = [
    ("b6_224_rel", "rel", 224, [0], 16, 64),
    ("b6_112_rel", "rel", 112, [0], 32, 96),
    ("b6_112n_rel", "rel", 112, [0, 0], 48, 32),
    ("b6_56_rel", "rel", 56, [0, 1], 48, 64),
    ("b6_28_rel", "rel", 28, [0, 1, 0], 32, 160),
    ("b6_14_rel", "rel", 14, [0, 1, 0], 16, 64),
    ("b6_14_rel", "rel+nan", 14, [0, 1, 0], 48, 64),
    ("b6_224_pool", "pool", 224, [0], 32, 64),
    ("b6_112_pool", "pool", 112, [0], 16, 128),
    ("b6_56_pool", "pool", 56, [0, 1], 48, 64),
    ("b6_28_pool", "pool", 28, [0, 1, 0], 32, 64),
    ("b6_224_fwd", "fwd", 224, [0], 16, 64),
    ("b6_112_fwd", "fwd", 112, [0], 32, 64),
    ("b6_56_fwd", "fwd", 56, [0, 1], 48, 64),
    ("b6_28_fwd", "fwd", 28, [0, 1, 2], 16, 64),
    ("b6_14_fwd", "fwd", 14, [0, 1, 2], 48, 192),
    ("b6_56_plain", "plain", 56, [0], 32, 64),
    ("b6_28_plain", "plain", 28, [0, 1, 2], 48, 64),
    ("b6_14_plain", "plain", 14, [0, 1, 2], 16, 96),
    ("b6_112n_guided", "guided", 112, [0], 16, 64),
    ("b6_56_guided", "guided", 56, [0, 1], 32, 64),
    ("b6_28_guided", "guided", 28, [0, 1, 0], 16, 64),
    ("b6_14_guided", "guided", 14, [0, 1, 0], 48, 64),
    ("b6_224_pool_guided", "pool_guided", 224, [0], 48, 64),
    ("b6_112_pool_guided", "pool_guided", 112, [0], 32, 96),
    ("b6_56_pool_guided", "pool_guided", 56, [0, 1], 16, 64),
    ("b6_28_pool_guided", "pool_guided", 28, [0, 1, 0], 48, 64),
]
SAMPLED_ROWS = 3


def name(case):
    return "%s_%s_m%d_k%d_oc%d" % (case[0], case[1].replace("+", "_"), len(case[3]), case[4], case[5])


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


_INPUTS = {}


def inputs(case):
    """the CPU tensors of one case, drawn once and never changed: dict(in, w, x, am, bias, digest)"""
    key = name(case)
    if key in _INPUTS:
        return _INPUTS[key]
    row, kind, hw, m2i, K, n_oc = case
    n_maps, n_img = len(m2i), max(m2i) + 1
    g = torch.Generator().manual_seed(91000 + CASES.index(case))
    base = kind.split("+")[0]
    pooled = base in ("pool", "pool_guided")
    p_in = (hw // 2) ** 2 if pooled else hw * hw
    d = {"am": None, "bias": None, "x": None}
    if base in ("fwd", "plain"):
        d["in"] = torch.randn(n_maps, p_in, K, generator=g).clamp(min=0)              # activations, NHWC
        d["w"] = torch.randn(n_oc, K, 3, 3, generator=g) * 0.05                         # (cout, cin): PACK_FWD
        if base == "fwd":
            d["bias"] = 0.05 * torch.randn(n_oc // 2, generator=g)
    else:
        d["in"] = torch.randn(n_maps, p_in, K, generator=g) * torch.exp(4 * torch.randn(n_maps, p_in, K, generator=g))
        d["w"] = torch.randn(K, n_oc, 3, 3, generator=g) * 0.05                         # (cout, cin) of the layer: the transposed conv
        d["x"] = torch.randn(n_img, hw * hw, n_oc, generator=g).clamp(min=0)
        if pooled:
            d["am"] = torch.randint(0, 4, (n_img, p_in, K), generator=g).to(torch.uint8)      # per IMAGE, as the forward trace leaves it
            assert all((d["am"] == q).any() for q in range(4))
    if kind.endswith("+nan"):
        # in the last map, away from its border: neither reaches a pixel of another map's result
        flat = d["in"][n_maps - 1].view(hw, hw, K)
        flat[hw // 2, hw // 2, 3] = float("inf")
        flat[hw // 2 - 3, hw // 2 + 3, K - 1] = float("nan")
    d["digest"] = sha(*[t for t in (d["in"], d["w"], d["x"], d["am"], d["bias"]) if t is not None])
    _INPUTS[key] = d
    return d


def describe(ops, case, maps=None):
    """(conv_mfma arguments, keyword arguments, outputs) of one case on the GPU; maps: the subset of the case's maps to run"""
    from lrp_amd import _lib
    row, kind, hw, m2i, K, n_oc = case
    base = kind.split("+")[0]
    d = inputs(case)
    sel = list(range(len(m2i))) if maps is None else list(maps)
    n_maps = len(sel)
    inp = d["in"][sel].contiguous().cuda()
    kw = dict(bf16x6=1)
    if base == "fwd":
        cout = n_oc // 2
        w = d["w"][:cout]
        wp = ops.pack_weights_bf16x3(torch.cat([w, w.clamp(min=0)]).cuda(), n_oc, K, _lib.PACK_FWD)
        outs = [torch.full((n_maps, hw * hw, cout), float("nan"), device="cuda") for _ in range(2)]
        kw.update(oc_split=cout, bias=d["bias"].cuda(), out0=outs[0], out1=outs[1])
        epi = _lib.EPI_FWD_DUAL
    elif base == "plain":
        wp = ops.pack_weights_bf16x3(d["w"].cuda(), n_oc, K, _lib.PACK_FWD)
        outs = [torch.full((n_maps, hw * hw, n_oc), float("nan"), device="cuda")]
        kw.update(oc_split=n_oc, out0=outs[0])
        epi = _lib.EPI_PLAIN
    else:
        guided = base in ("guided", "pool_guided")
        wp = ops.pack_weights_bf16x3(d["w"].cuda(), K, n_oc, _lib.PACK_BWD_PLAIN if guided else _lib.PACK_BWD_POS)
        outs = [torch.full((n_maps, hw * hw, n_oc), float("nan"), device="cuda")]
        kw.update(oc_split=n_oc, x=d["x"].cuda(), map2img=torch.tensor([m2i[i] for i in sel], dtype=torch.int32, device="cuda"))
        kw["out0" if guided else "out1"] = outs[0]
        if d["am"] is not None:
            kw["pool_am"] = d["am"].cuda()                     # (indexed through map2img, like x)
        epi = _lib.EPI_GUIDED if guided else _lib.EPI_REL_MUL
    return (inp, wp, n_maps, hw, K, n_oc, 9, epi), kw, outs


def kernel_row(ops, args, kw):
    from lrp_amd import _lib
    buf = C.create_string_buffer(128)
    _lib.check(_lib.load().lrpx_conv_kernel_name(C.byref(ops.conv_desc(*args, **kw)), buf, len(buf)))
    return buf.value.decode().split()[0]


def run(ops, case, maps=None):
    """the case's outputs (one tensor per map and output, concatenated along the channels) on the CPU, and the row that ran"""
    args, kw, outs = describe(ops, case, maps)
    row = kernel_row(ops, args, kw)
    ops.conv_mfma(*args, **kw)
    torch.cuda.synchronize()
    return torch.cat([o.cpu() for o in outs], dim=-1), row


def sampled(out):
    """(map, pixel) -> hex of the bytes of the row's first 16 channels, at three fixed places of the output"""
    n_maps, pix, _ = out.shape
    where = [(0, 0), ((n_maps - 1) // 2, pix // 2 + 3), (n_maps - 1, pix - 1)][:SAMPLED_ROWS]
    return {"%d,%d" % (m, p): out[m, p, :16].contiguous().numpy().tobytes().hex() for m, p in where}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under LRPX_LIB_PATH was built from")
    ap.add_argument("--out", default=JSON)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lrp_amd  # noqa: F401
    from lrp_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_b6_ring_parent_bits: needs a GPU")
    prev = ops.set_b6_wino(0)            # (no Winograd weights are passed either: the direct rows)
    g = {"recorded_from_commit": a.commit, "cases": {}}
    try:
        for case in CASES:
            out, row = run(ops, case)
            assert row == case[0], (name(case), row)
            assert not torch.isnan(out).all(), name(case)
            if not case[1].endswith("+nan"):
                assert torch.isfinite(out).all(), name(case)
            assert same_bits(out, run(ops, case)[0]), name(case) + ": the recording build does not repeat itself"
            g["cases"][name(case)] = {"row": row, "inputs": inputs(case)["digest"], "sha256": sha(out), "rows": sampled(out)}
    finally:
        ops.set_b6_wino(prev)
    with open(a.out, "w") as f:
        json.dump(g, f, indent=1, sort_keys=True)
        f.write("\n")
    print(os.path.basename(a.out) + ":", os.path.getsize(a.out), "bytes;", len(CASES), "cases, library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
