"""The VGG16 chains of csrc/lrpx_vgg.hip keep the bits they had when tests/golden/vgg_chain_parent_bits.json was recorded - from the
commit named in that file, before the host code that drives them was rewritten around one list of the blob's regions, one row per conv
mode and one function per flow.  No kernel changed: every launch keeps its descriptor, its operands and its place in the order.

The cases are those of tests/golden/make_golden_vgg_chain_parent_bits.py (that file lists them and says why): conv modes 0 - 3, modes 2
and 3 with forward_f16 as well, mode 1 also without the Winograd kernels; per config the features and every tensor of trace_views(),
then relevance, gradient and guided backprop for three map sets (map2img None; tile group 2; tile group off), and one relevance through
layer_ms.  Each must
  - give the recorded sha256,
  - give the same bits on a second call,
  - (the timed relevance) give the untimed call's bits and a time for exactly the layers the recorded build timed.
The recorded build repeated every case, so none is left out (the golden's "not_recorded" is empty, and the first test says so).
A changed digest of the INPUTS fails the test as such: the CPU draw changed, nothing is known about the library."""
import json
import sys

import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_vgg_chain_parent_bits as G  # noqa: E402


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


@pytest.fixture(scope="module")
def vgg(ops):
    return G.context(ops)


def test_the_golden_holds_every_case(golden):
    assert len(golden["recorded_from_commit"]) == 40
    assert golden["not_recorded"] == []
    assert sorted(golden["configs"]) == sorted(G.config_name(c) for c in G.CONFIGS)
    names = ["features"] + ["act%d" % l for l in range(18)] + ["zpos%d" % l for l in (0, 1, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15, 16)]
    names += ["%s_%s" % (c, m) for c in G.CHAINS for m, _ in G.MAPSETS]
    for c in golden["configs"].values():
        assert sorted(c["sha256"]) == sorted(names)
        assert c["timed_layers"] == [0, 1, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15, 16]       # the conv layers, the first one included


@pytest.mark.parametrize("cfg", G.CONFIGS, ids=G.config_name)
def test_same_bits_as_the_recorded_build(ops, golden, vgg, cfg):
    assert G.inputs()["digest"] == golden["inputs"], "the INPUTS changed (the CPU draw of this numpy / torch is not the recorded one), nothing is known about the library"
    want = golden["configs"][G.config_name(cfg)]
    before = ops.set_b6_wino(-1)
    got, unstable, timed = G.run(ops, vgg, cfg)
    assert ops.set_b6_wino(-1) == before                  # (the Winograd mask is back where it was)
    assert not unstable, "a second call gives other bits: %s" % unstable
    diff = sorted(k for k in want["sha256"] if got.get(k) != want["sha256"][k])
    assert not diff, "%s: not the bits of the build recorded at %s: %s" % (G.config_name(cfg), golden["recorded_from_commit"], diff)
    assert sorted(got) == sorted(want["sha256"])
    assert timed == want["timed_layers"]
