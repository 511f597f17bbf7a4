#!/usr/bin/env python3
"""Outputs of the Winograd relevance conv (csrc/conv_wino_b6.h) for seeded CPU inputs, recorded once from a build whose bits are to be
kept - tests/test_gpu_b6_wino_bits.py runs the same cases on the build at hand and requires the same bits, in both stagings.  Writes
tests/golden/wino_parent_bits.npz.

    LRPX_LIB_PATH=<liblrpx.so of that commit> python tests/golden/make_golden_wino_parent_bits.py --commit <its hash>

Needs a GPU.  The kernel stages K in chunks of 16 through two LDS buffers, one chunk ahead; the shapes run its prologue, its steady
state and its drain, on both buffers:

    14 x 14, map2img [0, 1, 0], K 16, n_oc 64    one chunk: prologue and drain only
    14 x 14, map2img [0, 1, 0], K 32, n_oc 64    two chunks
    14 x 14, map2img [0, 0],    K 48, n_oc 128   three chunks (odd), two channel blocks, the second map starts inside a wave
    28 x 28, map2img [0],       K 64, n_oc 128   four chunks
    56 x 56, map2img [0],       K 32, n_oc 64    two chunks, 784 tiles: the last workgroup is ragged

Inputs as tests/test_gpu_b6_wino_share.py draws them: S standard normal with a distinct value at every (map, y, x, channel), x ReLU'd,
w * 0.05.  Stored per case: a sha256 of the inputs (a changed CPU draw is told apart from a changed kernel), a sha256 of the output
bytes and one fp64 sum per pixel row (map, pixel), which says where a changed output changed; the output itself for the three 14 x 14
cases only, so that the file stays well below the size limit of a committed file.  The recording build ran every case with both
stagings (lrpx_set_b6_wino 15 and 7) and gave the same bits."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "wino_parent_bits.npz")
# (hw, map2img, K, n_oc)
SHAPES = [(14, [0, 1, 0], 16, 64), (14, [0, 1, 0], 32, 64), (14, [0, 0], 48, 128), (28, [0], 64, 128), (56, [0], 32, 64)]
STAGINGS = (15, 7)                       # lrpx_set_b6_wino: every thread fetches its whole patch / column sharing
STORE_ARRAYS_UP_TO_HW = 14


def name(shape):
    return "hw%d_m%d_k%d_oc%d" % (shape[0], len(shape[1]), shape[2], shape[3])


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def distinct_normal(shape, g):
    """standard normal draws, re-drawn where two elements came out equal: every element is another value"""
    s = torch.randn(shape, generator=g)
    flat = s.view(-1)
    while True:
        srt, idx = flat.sort()
        dup = idx[1:][srt[1:] == srt[:-1]]
        if dup.numel() == 0:
            return s
        flat[dup] = torch.randn(dup.numel(), generator=g)


_CASES = {}


def inputs(shape):
    """(x, w, s, digest) of one shape, drawn once on the CPU and never changed"""
    hw, m2i, K, n_oc = shape
    key = name(shape)
    if key not in _CASES:
        g = torch.Generator().manual_seed(77000 + hw * 1000 + K * 10 + n_oc + len(m2i))
        x = torch.randn(max(m2i) + 1, hw, hw, n_oc, generator=g).clamp(min=0)
        w = torch.randn(K, n_oc, 3, 3, generator=g) * 0.05
        s = distinct_normal((len(m2i), hw, hw, K), g)         # NHWC, as the kernel reads it
        _CASES[key] = (x, w, s, sha(x, w, s))
    return _CASES[key]


def pack(ops, w, K, n_oc):
    from lrp_amd import _lib
    return (ops.pack_weights_bf16x3(w.cuda(), K, n_oc, _lib.PACK_BWD_POS), ops.pack_weights_wino_b6(w.cuda(), K, n_oc, _lib.PACK_BWD_POS))


def launch(ops, x, s_dev, packed, hw, m2i, K, n_oc, wino=True):
    """one launch; s_dev is S on the GPU (a view into a larger allocation is taken as it is)"""
    from lrp_amd import _lib
    n_maps = len(m2i)
    out = torch.full((n_maps, hw * hw, n_oc), float("nan"), device="cuda")
    ops.conv_mfma(s_dev, packed[0], n_maps, hw, K, n_oc, 9, _lib.EPI_REL_MUL, oc_split=n_oc, x=x.contiguous().cuda(),
                  map2img=torch.tensor(m2i, dtype=torch.int32, device="cuda"), out1=out, bf16x6=1,
                  wpacked_wino=packed[1] if wino else None)
    torch.cuda.synchronize()
    return out.cpu()


def run(ops, shape, staging, s_dev=None, packed=None):
    hw, m2i, K, n_oc = shape
    x, w, s, _ = inputs(shape)
    prev = ops.set_b6_wino(-1)
    try:
        ops.set_b6_wino(staging)
        return launch(ops, x, s.contiguous().cuda() if s_dev is None else s_dev, packed or pack(ops, w, K, n_oc), hw, m2i, K, n_oc)
    finally:
        ops.set_b6_wino(prev)


def row_sums(out):
    return out.double().sum(dim=-1).numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under LRPX_LIB_PATH was built from")
    ap.add_argument("--out", default=NPZ)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lrp_amd  # noqa: F401
    from lrp_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_wino_parent_bits: needs a GPU")
    g = {"recorded_from_commit": np.array(a.commit)}
    for shape in SHAPES:
        hw, m2i, K, n_oc = shape
        n = name(shape)
        x, w, s, digest = inputs(shape)
        packed = pack(ops, w, K, n_oc)
        outs = [run(ops, shape, st, packed=packed) for st in STAGINGS]
        assert all(torch.isfinite(o).all() for o in outs), n
        assert torch.equal(outs[0], outs[1]), n + ": the two stagings of the recording build differ"
        direct = launch(ops, x, s.contiguous().cuda(), packed, hw, m2i, K, n_oc, wino=False)
        assert not torch.equal(outs[0], direct), n + ": the Winograd kernel did not run"
        g[n + "/inputs"] = np.array(digest)
        g[n + "/sha256"] = np.array(sha(outs[0]))
        g[n + "/row_sums"] = row_sums(outs[0])
        if hw <= STORE_ARRAYS_UP_TO_HW:
            g[n + "/out"] = outs[0].numpy()
    np.savez(a.out, **g)
    print(os.path.basename(a.out) + ":", os.path.getsize(a.out), "bytes;", len(SHAPES), "shapes, library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
