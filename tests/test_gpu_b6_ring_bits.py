"""Every conv-mode-1 kernel on the conv_f16x3.h tiling (the B6 rows of csrc/conv_kernels.def) keeps the bits it had when
tests/golden/b6_ring_parent_bits.json was recorded - from the commit named in that file, before the weight queue of these kernels became
a ring of buffer loads.  The change is one of scheduling alone: every MFMA keeps its operands and its place in its accumulator's order.

The cases are those of tests/golden/make_golden_b6_ring_parent_bits.py (that file lists them and says why: every row once - relevance,
pooled input, forward DUAL and PLAIN, guided; K = 16 / 32 / 48, that is 9 / 18 / 27 queue steps against a ring of 3 - 5 entries, so the
prologue, the wrap across a chunk boundary and the clamped tail all run; waves without a channel block; winners in every window position;
an Inf and a NaN in S).  Each case goes through lrpx_conv_mfma (conv_dispatch) and must
  - run on the row of the kernel list it is named after,
  - give the recorded sha256 (the sampled rows say whether a difference is everywhere or not),
  - give the same bits when launched again,
  - give, for every map, the bits of that map launched alone.
A changed digest of the INPUTS fails the test as such: the CPU draw changed, nothing is known about the kernel."""
import json
import sys

import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_b6_ring_parent_bits as G  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden():
    with open(G.JSON) as f:
        return json.load(f)


def test_the_golden_holds_every_case_and_every_row(golden):
    assert sorted(golden["cases"]) == sorted(G.name(c) for c in G.CASES)
    assert len(golden["recorded_from_commit"]) == 40
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "lrp-imagecaptioning-pytorch_amd", "csrc", "conv_kernels.def")) as f:
        rows = re.findall(r"^K\((b6_\w+), FAM_B6, \d+, \w+, VAR_(?:DIRECT|POOL), .*launch_conv_f16x3,", f.read(), re.M)
    assert len(rows) == 26 and sorted(rows) == sorted({c[0] for c in G.CASES})


@pytest.mark.parametrize("case", G.CASES, ids=G.name)
def test_same_bits_as_the_recorded_build(ops, golden, case):
    n = G.name(case)
    want = golden["cases"][n]
    assert G.inputs(case)["digest"] == want["inputs"], f"{n}: the INPUTS changed (the CPU draw of this torch is not the recorded one), nothing is known about the kernel"
    got, row = G.run(ops, case)
    assert row == case[0] == want["row"]
    if case[1].endswith("+nan"):
        assert torch.isnan(got).any() and torch.isfinite(got).any()
    else:
        assert torch.isfinite(got).all()
    rows = G.sampled(got)
    diff = [k for k in rows if rows[k] != want["rows"][k]]
    assert G.sha(got) == want["sha256"], f"{n}: not the bits of the build recorded at {golden['recorded_from_commit']}; sampled rows (map,pixel) that differ: {diff or 'none'}"
    assert not diff
    # again, and every map alone
    assert G.same_bits(got, G.run(ops, case)[0]), n + ": a second launch gives other bits"
    if len(case[3]) > 1:
        for i in range(len(case[3])):
            alone, row_i = G.run(ops, case, maps=[i])
            assert row_i == case[0]
            assert G.same_bits(alone[0], got[i]), f"{n}: map {i} alone is not the map in the batch"
