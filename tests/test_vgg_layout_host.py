"""The packed weight blob, the trace and the workspace of the VGG16 chains keep the layout they had when
tests/golden/vgg_layout_parent.json was recorded - from the commit named in that file, before the blob's regions became one list that
both the layout and the packer walk.  Pure host calls (tests/golden/make_golden_vgg_layout.py lists them): no GPU."""
import json
import sys

import pytest

import lrp_amd  # noqa: F401
from conftest import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_vgg_layout as G  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(G.JSON) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    from lrp_amd import _lib
    return G.measure(_lib.load())


def test_the_golden_is_complete(golden):
    assert len(golden["recorded_from_commit"]) == 40 and golden["base"] == G.BASE
    assert sorted(golden["per_n"]) == sorted(str(n) for n in G.NS)
    assert len(golden["channel_scales"]) == 17 and sum(c is not None for c in golden["channel_scales"]) == 13


def test_packed_blob(golden, got):
    assert got["packed_bytes"] == golden["packed_bytes"]
    assert got["row_spread"] == golden["row_spread"]
    for l in range(17):
        assert got["channel_scales"][l] == golden["channel_scales"][l], "layer %d" % l
    # both regions lie inside the blob, and in float units
    assert 0 < got["row_spread"] < got["packed_bytes"] and got["row_spread"] % 4 == 0


@pytest.mark.parametrize("n", G.NS)
def test_trace_and_workspace(golden, got, n):
    want, have = golden["per_n"][str(n)], got["per_n"][str(n)]
    assert have["trace_bytes"] == want["trace_bytes"]
    assert have["workspace_bytes"] == want["workspace_bytes"]
    assert have["act"] == want["act"]
    assert have["zpos"] == want["zpos"]
