#!/usr/bin/env python3
"""Which kernel lrpx_conv_mfma picks for a descriptor (lrpx_conv_kernel_name: name, K split, tile group, or the refusal), over a grid of
descriptors, recorded once from the if-ladder that csrc/lrpx_vgg.hip:conv_dispatch was before the kernel list (csrc/conv_kernels.def) -
tests/test_conv_table_host.py asks the build at hand the same questions and requires the recorded answers.  Host code only: no GPU.

The ladder had no name entry: tools/experiments/conv_choice_recorder.patch adds one to that commit by a mechanical rewrite (every
`return launch_X(a, s)` answers X instead of launching, the output clear is skipped).  Apply it there, build, and

    LRPX_LIB_PATH=<that liblrpx.so> python tests/golden/make_golden_conv_choice.py --commit <the ladder's commit>

Writes tests/golden/conv_choice.json.  "conv" holds the 3x3 grid: key "f16x3,bf16x6,epi,pool_am,hw,n_oc,tile_group" -> the answers
for the six (wpacked_wino, lrpx_set_b6_wino bits) combinations WINOS, folded into one string where all six are equal.  "dense" is the
list of [field overrides, answer] of the taps = 1 descriptors DENSE."""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
JSON = os.path.join(HERE, "conv_choice.json")
FWD_DUAL, REL, FIRST, PLAIN, GUIDED, REL_MUL = range(6)
FAMILIES = ((0, 0), (1, 0), (2, 0), (0, 1))                        # (f16x3, bf16x6)
HWS, N_OCS, TILE_GROUPS = (224, 112, 56, 28, 14), (32, 64, 96, 128, 160, 256, 512), (0, 4)
WINOS = tuple(itertools.product((0, 1), (0, 7, 15)))               # (wpacked_wino given, lrpx_set_b6_wino bits)
PTR = 0x1000                                                       # never dereferenced: the name entry touches no memory behind the descriptor
# taps = 1: every dense route and its refusals; rows = n_maps * pix_per_map.  rows = 64 with cin = 16384 is what still reaches the atomic
# K split (dense_small_fits takes every smaller fp32 GEMM with out0 alone)
DENSE = [dict(bf16x6=1, epi=REL), dict(bf16x6=1, epi=REL, n_maps=64, pix_per_map=196, tile_group=4), dict(bf16x6=1, epi=PLAIN),
         dict(bf16x6=1, f16x3=1, epi=REL), dict(bf16x6=1, epi=REL, x=None),
         dict(f16x3=1, epi=PLAIN), dict(f16x3=1, epi=PLAIN, in_amax=None), dict(f16x3=2, epi=PLAIN), dict(f16x3=2, epi=REL),
         dict(f16x3=1, epi=GUIDED), dict(f16x3=1, epi=REL), dict(f16x3=1, epi=REL, n_maps=4096), dict(f16x3=1, epi=REL, n_maps=4097),
         dict(f16x3=1, epi=REL, n_maps=4097, in_amax=None), dict(f16x3=1, epi=REL, cin=2048), dict(f16x3=1, epi=REL, out1=PTR),
         dict(f16x3=1, epi=REL, out1=PTR, zdiv=None, stab=1), dict(f16x3=1, epi=REL, n_maps=8, pix_per_map=4, tile_group=4),
         dict(epi=REL), dict(epi=PLAIN), dict(epi=REL, x=None), dict(epi=GUIDED), dict(epi=REL, pix_per_map=0),
         dict(epi=REL, cin=8192), dict(epi=REL, cin=16384), dict(epi=PLAIN, cin=16384), dict(epi=PLAIN, cin=16384, relu=1),
         dict(epi=PLAIN, cin=16384, n_maps=2048), dict(epi=PLAIN, cin=16384, n_maps=2049), dict(epi=REL, cin=16384, out1=PTR),
         dict(epi=REL, n_maps=8, pix_per_map=1024), dict(epi=REL, out1=PTR), dict(epi=REL, cin=48), dict(epi=REL, cin=16384, hw=0),
         dict(epi=PLAIN, cin=16384, pool_am=PTR), dict(epi=REL, n_oc=48)]


def conv_fields(f16x3, bf16x6, epi, pool, hw, n_oc, tg, wino):
    """a 3x3 descriptor that is valid wherever the selection allows one with these choices"""
    return dict(taps=9, f16x3=f16x3, bf16x6=bf16x6, epi=epi, hw=hw, n_oc=n_oc, n_maps=8, cin=64, tile_group=tg,
                oc_split=n_oc // 64 * 32 if epi == FWD_DUAL else n_oc,
                out0=None if epi == REL_MUL else PTR, out1=PTR if epi in (FWD_DUAL, REL_MUL) else None,
                blocked=(1 if hw == 224 else 7) if (f16x3 == 2 and epi == REL_MUL) else 0,
                pool_am=PTR if pool else None, wpacked_wino=PTR if wino else None)


def dense_fields(over):
    f = dict(taps=1, hw=14, n_maps=64, pix_per_map=1, cin=512, n_oc=32, oc_split=32, out0=PTR)
    f.update(over)
    return f


def ask(lib, _lib, fields, bits=None):
    """(answer, error text): lrpx_conv_kernel_name's string, or "EINVAL" with lrpx_last_error_string()"""
    kw = dict(in_=PTR, wpacked=PTR, x=PTR, u=PTR, zdiv=PTR, in_amax=PTR)
    kw.update(fields)
    d = _lib.ConvDesc(**kw)
    if bits is not None:
        lib.lrpx_set_b6_wino(bits)
    buf = C.create_string_buffer(96)
    rc = lib.lrpx_conv_kernel_name(C.byref(d), buf, len(buf))
    if rc == _lib.OK:
        return buf.value.decode(), ""
    assert rc == _lib.EINVAL, rc
    return "EINVAL", lib.lrpx_last_error_string().decode()


def conv_keys():
    for (f16x3, bf16x6), epi, pool, hw, n_oc, tg in itertools.product(FAMILIES, range(6), (0, 1), HWS, N_OCS, TILE_GROUPS):
        yield "%d,%d,%d,%d,%d,%d,%d" % (f16x3, bf16x6, epi, pool, hw, n_oc, tg)


def conv_answers(lib, _lib, key):
    """[(answer, error text)] of one grid key, in the order of WINOS"""
    k = [int(v) for v in key.split(",")]
    prev = lib.lrpx_set_b6_wino(-1)
    try:
        return [ask(lib, _lib, conv_fields(*k, wino), bits) for wino, bits in WINOS]
    finally:
        lib.lrpx_set_b6_wino(prev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under LRPX_LIB_PATH was built from (plus the recorder patch)")
    ap.add_argument("--out", default=JSON)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lrp_amd  # noqa: F401
    from lrp_amd import _lib
    lib = _lib.load()
    g = {"recorded_from_commit": a.commit, "winos": [list(w) for w in WINOS], "conv": {}, "dense": []}
    for key in conv_keys():
        ans = [r[0] for r in conv_answers(lib, _lib, key)]
        g["conv"][key] = ans[0] if len(set(ans)) == 1 else ans
    for over in DENSE:
        g["dense"].append([over, ask(lib, _lib, dense_fields(over))[0]])
    with open(a.out, "w") as f:
        json.dump(g, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    names = {s.split()[0] for v in g["conv"].values() for s in (v if isinstance(v, list) else [v])} | {v.split()[0] for _, v in g["dense"]}
    print(os.path.basename(a.out) + ":", os.path.getsize(a.out), "bytes;", len(g["conv"]) * len(WINOS), "3x3 and", len(DENSE),
          "dense descriptors,", len(names) - 1, "kernel names, library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
