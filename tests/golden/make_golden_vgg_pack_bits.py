#!/usr/bin/env python3
"""sha256 of the whole packed weight blob that lrpx_vgg16_pack writes for seeded VGG16 weights, recorded once from a build whose blob
is to be kept - tests/test_gpu_vgg_pack_bits.py packs with the build at hand and requires the same digest.  Writes
tests/golden/vgg_pack_parent_bits.json.

    LRPX_LIB_PATH=<liblrpx.so of that commit> python tests/golden/make_golden_vgg_pack_bits.py --commit <its hash>

Needs a GPU.  The blob is ZERO-FILLED before the pack (ops.Vgg16 allocates it with torch.empty: the bytes between and behind what the
packers write would be whatever the allocator left), so the entry point is called directly.  The weights are the encoder part of
weights.make_gridtd_state(seed=SEED) with non-zero biases.  Stored: a sha256 of the weights and biases (a changed CPU draw is told
apart from a changed library), the blob's size and its sha256, taken in slices (the blob is about 1 GB)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
JSON = os.path.join(HERE, "vgg_pack_parent_bits.json")
SEED = 23
SLICE = 1 << 24            # floats per slice of the digest


_INPUTS = {}


def inputs():
    """the 13 weights and biases on the CPU, drawn once: dict(w, b, digest)"""
    if not _INPUTS:
        from lrp_amd import weights
        sd = weights.make_gridtd_state(seed=SEED, vocab_size=16, vgg_bias_std=0.05)
        names = [k for k in sd if k.startswith("img_encoder.encoder.") and k.endswith(".weight")]
        _INPUTS["w"] = [torch.from_numpy(sd[k]) for k in names]
        _INPUTS["b"] = [torch.from_numpy(sd[k.replace(".weight", ".bias")]) for k in names]
        h = hashlib.sha256()
        for t in _INPUTS["w"] + _INPUTS["b"]:
            h.update(t.contiguous().numpy().tobytes())
        _INPUTS["digest"] = h.hexdigest()
    return _INPUTS


def pack():
    """lrpx_vgg16_pack of the seeded weights into a fresh zero-filled blob -> the blob (device, float32)"""
    from lrp_amd import _lib
    lib = _lib.load()
    d = inputs()
    ws, bs = [w.cuda().contiguous() for w in d["w"]], [b.cuda().contiguous() for b in d["b"]]
    blob = torch.zeros(lib.lrpx_vgg16_packed_bytes() // 4, dtype=torch.float32, device="cuda")
    wp = (C.c_void_p * 13)(*[w.data_ptr() for w in ws])
    bp = (C.c_void_p * 13)(*[b.data_ptr() for b in bs])
    _lib.check(lib.lrpx_vgg16_pack(wp, bp, _lib.ptr(blob), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return blob


def sha_sliced(blob):
    h = hashlib.sha256()
    for lo in range(0, blob.numel(), SLICE):
        h.update(blob[lo: lo + SLICE].cpu().numpy().tobytes())
    return h.hexdigest()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under LRPX_LIB_PATH was built from")
    ap.add_argument("--out", default=JSON)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lrp_amd  # noqa: F401
    from lrp_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_vgg_pack_bits: needs a GPU")
    blob = pack()
    assert same_bits(blob, pack()), "the recording build does not repeat itself"
    g = {"recorded_from_commit": a.commit, "inputs": inputs()["digest"], "blob_bytes": blob.numel() * 4, "sha256": sha_sliced(blob)}
    with open(a.out, "w") as f:
        json.dump(g, f, indent=1, sort_keys=True)
        f.write("\n")
    print(os.path.basename(a.out) + ":", g["blob_bytes"], "bytes of blob, sha256", g["sha256"][:16], "...; library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
