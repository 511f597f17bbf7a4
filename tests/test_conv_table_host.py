"""The conv kernel list (csrc/conv_kernels.def, conv_dispatch.hip: conv_select) picks what the if-ladder before it picked: for every
descriptor of tests/golden/conv_choice.json (recorded from that ladder, make_golden_conv_choice.py) lrpx_conv_kernel_name answers the
recorded kernel, K split and tile group, or refuses where the ladder refused.  Host code only: no GPU."""
import json
import os
import re
import sys

import pytest

import lrp_amd  # noqa: F401
from lrp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_conv_choice as G  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="liblrpx.so not built (run __graft_entry__.build())")


def ladder_name(answer):
    """the ladder had ONE launcher per Winograd map size and chose the staging inside it; the list has a row per staging variant,
    b6_<hw>_wino (lrpx_set_b6_wino bit 8 set: own fetch) and b6_<hw>_wino_share: the recorded name is the row's without `_share`"""
    return re.sub(r"^(b6_\d+_wino)_share ", r"\1 ", answer)


@pytest.fixture(scope="module")
def answers():
    """{(grid key, index into G.WINOS) or ("dense", i): (recorded, answer, error text)}: every descriptor of the golden, asked once"""
    lib, gold = _lib.load(), json.load(open(G.JSON))
    assert [tuple(w) for w in gold["winos"]] == list(G.WINOS)
    assert sorted(gold["conv"]) == sorted(G.conv_keys()) and [o for o, _ in gold["dense"]] == G.DENSE       # no entry is left out
    res = {}
    for key, want in gold["conv"].items():
        for i, (got, err) in enumerate(G.conv_answers(lib, _lib, key)):
            res[key, i] = (want[i] if isinstance(want, list) else want, got, err)
    for i, (over, want) in enumerate(gold["dense"]):
        res["dense", i] = (want,) + G.ask(lib, _lib, G.dense_fields(over))
    return res


def test_every_descriptor_gets_the_recorded_kernel(answers):
    assert len(answers) == 4 * 6 * 2 * 5 * 7 * 2 * 6 + len(G.DENSE)
    bad = {k: v[:2] for k, v in answers.items() if v[0] != ladder_name(v[1])}
    assert not bad, (len(bad), sorted(bad.items(), key=str)[:8])


def test_winograd_staging_variant_follows_bit_8(answers):
    """bit 8 of lrpx_set_b6_wino set (15): launch_conv_wino_b6<HW, false>, the b6_<hw>_wino row; clear (7): <HW, true>, the _share row"""
    wino = {k: v[1].split()[0] for k, v in answers.items() if "_wino" in v[1]}
    assert wino and {G.WINOS[k[1]] for k in wino} == {(1, 7), (1, 15)}
    for k, name in wino.items():
        assert name.endswith("_share") == (G.WINOS[k[1]][1] == 7), (k, name)
    src = open(os.path.join(ROOT, "lrp-imagecaptioning-pytorch_amd", "csrc", "conv_kernels.def")).read()
    for name in set(wino.values()):
        hw = name.split("_")[1]
        assert re.search(r"^K\(%s, .*launch_conv_wino_b6, %s, %s\)$" % (name, hw, "true" if name.endswith("_share") else "false"), src, re.M), name


def test_every_row_of_the_list_is_some_descriptors_answer(answers):
    rows = re.findall(r"^K\((\w+),", open(os.path.join(ROOT, "lrp-imagecaptioning-pytorch_amd", "csrc", "conv_kernels.def")).read(), re.M)
    assert rows and len(set(rows)) == len(rows)                        # a row's name is its launcher's: no two alike
    got = {v[1].split()[0] for v in answers.values()}
    assert not set(rows) - got, sorted(set(rows) - got)
    assert got - set(rows) == {"EINVAL", "dense_bf16x6", "dense_f16x3", "dense_small_f16x3", "dense_small"}


def test_no_descriptor_matches_two_rows(answers):
    """conv_select counts the rows that take a descriptor and refuses with "<n> rows of conv_kernels.def take ..." unless it is one"""
    assert not [k for k, v in answers.items() if "rows of conv_kernels.def" in v[2]]


def test_other_map_sizes_are_refused():
    """taps = 9 is built for 224 / 112 / 56 / 28 / 14-pixel maps: the ladder ran bf16x6 PLAIN and Winograd descriptors of any other
    hw <= 56 on the 14 x 14 kernels"""
    lib = _lib.load()
    for hw in (7, 42, 448):
        for f16x3, bf16x6 in G.FAMILIES:
            for epi in range(6):
                for wino, bits in ((0, None), (1, 15)):
                    prev = lib.lrpx_set_b6_wino(-1)
                    try:
                        got, err = G.ask(lib, _lib, G.conv_fields(f16x3, bf16x6, epi, 0, hw, 64, 0, wino), bits)
                    finally:
                        lib.lrpx_set_b6_wino(prev)
                    assert got == "EINVAL" and "hw=%d" % hw in err, (hw, f16x3, bf16x6, epi, wino, got, err)
