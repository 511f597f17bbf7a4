#!/usr/bin/env python3
"""What the host side of csrc/lrpx_vgg.hip answers about the packed weight blob, the trace and the workspace of the VGG16 chains, recorded
once from a build whose layout is to be kept - tests/test_vgg_layout_host.py asks the build at hand the same and requires the same
numbers.  Writes tests/golden/vgg_layout_parent.json.  Pure host calls: no GPU.

    LRPX_LIB_PATH=<liblrpx.so of that commit> python tests/golden/make_golden_vgg_layout.py --commit <its hash>

Recorded: lrpx_vgg16_packed_bytes(); the byte offsets of lrpx_vgg16_row_spread and lrpx_vgg16_channel_scales (with its channel count;
null for a pool) for each of the 17 layers against BASE, an aligned address that is never dereferenced (the two only add to it); and, for
n = 1, 2, 16: lrpx_vgg16_trace_bytes(n), every offset of lrpx_vgg16_trace_layout(n), lrpx_vgg16_workspace_bytes(n)."""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
JSON = os.path.join(HERE, "vgg_layout_parent.json")
BASE = 1 << 40
NS = (1, 2, 16)


def measure(lib):
    """the recorded quantities of the library `lib` (lrp_amd._lib.load()), as JSON holds them"""
    g = {"packed_bytes": lib.lrpx_vgg16_packed_bytes(), "row_spread": lib.lrpx_vgg16_row_spread(C.c_void_p(BASE)) - BASE,
         "channel_scales": [], "per_n": {}}
    for l in range(17):
        n = C.c_int(-1)
        p = lib.lrpx_vgg16_channel_scales(C.c_void_p(BASE), l, C.byref(n))
        g["channel_scales"].append(None if not p else [p - BASE, n.value])
    for n in NS:
        act, zpos = (C.c_size_t * 18)(), (C.c_size_t * 17)()
        assert lib.lrpx_vgg16_trace_layout(n, act, zpos) == 0
        g["per_n"][str(n)] = {"trace_bytes": lib.lrpx_vgg16_trace_bytes(n), "act": list(act), "zpos": list(zpos),
                              "workspace_bytes": lib.lrpx_vgg16_workspace_bytes(n)}
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under LRPX_LIB_PATH was built from")
    ap.add_argument("--out", default=JSON)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lrp_amd  # noqa: F401
    from lrp_amd import _lib
    g = dict(recorded_from_commit=a.commit, base=BASE, **measure(_lib.load()))
    with open(a.out, "w") as f:
        json.dump(g, f, indent=1, sort_keys=True)
        f.write("\n")
    print(os.path.basename(a.out) + ":", os.path.getsize(a.out), "bytes; library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
