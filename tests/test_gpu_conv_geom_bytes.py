"""The runtime-geometry conv engine (csrc/conv_geom_kernel.h: lrpx_conv_geom, _ex, _ex_b6, _ab, _ab_b6 and the two packers) gives the bytes
it gave when tests/golden/conv_geom_bytes.json was recorded: sha256 of every output of tests/golden/make_golden_conv_geom_bytes.py's
cases, which reach every path of the tiling (that file lists them).  A changed digest of a shape's INPUTS is reported as such - the CPU
draw changed, not the kernel.  And lrpx_conv_geom's transposed direction is lrpx_conv_geom_ex's with q, addend and map2img null, byte for
byte, whatever the golden says."""
import json
import sys

import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_conv_geom_bytes as G  # noqa: E402


@pytest.mark.parametrize("gname", list(G.GEOMS))
def test_bytes_are_the_recorded_ones(gname):
    from lrp_amd import _lib, ops
    with open(G.JSON) as f:
        golden = json.load(f)
    assert golden["fill"] == "0x%08X" % G.FILL
    shapes = [s for s in G.SHAPES if s[1] == G.GEOMS[gname]]
    assert len(shapes) == len(G.KS) * len(G.N_OCS)
    changed = []
    for name, geom, k, n_oc in shapes:
        want = golden["shapes"][name]
        c = G.inputs(name, geom, k, n_oc)
        assert c["digest"] == want["inputs"], f"{name}: the INPUTS changed (the CPU draw of this torch is not the recorded one), nothing is known about the kernels"
        got = G.run_shape(c, ops, _lib)
        torch.cuda.synchronize()
        assert sorted(got) == sorted(want["outputs"]), f"{name}: the cases are not the recorded ones"
        changed += [f"{name}/{case}" for case in got if got[case] != want["outputs"][case]]
        assert got["geom_bwd"] == got["ex_bwd_q0_add0_m2i0"], f"{name}: lrpx_conv_geom BWD differs from lrpx_conv_geom_ex BWD without its operands"
    assert not changed, f"{len(changed)} outputs differ from the bytes recorded at {golden['recorded_from_commit']}: " + ", ".join(changed)


def test_the_golden_holds_every_shape():
    with open(G.JSON) as f:
        golden = json.load(f)
    assert sorted(golden["shapes"]) == sorted(s[0] for s in G.SHAPES)
    per_shape = 3 + 2 * (1 + 8) + 2 * 6
    for name, _, k, n_oc in G.SHAPES:
        assert len(golden["shapes"][name]["outputs"]) == per_shape + (4 if (k, n_oc) == G.PACK_SHAPE else 0), name
