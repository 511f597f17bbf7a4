"""The caption explainers - both engines' batch entry points, static-buffer drivers and decode loops, and the ten drop-in classes - give
the bytes they gave when tests/golden/explainer_bytes.json was recorded: sha256 of every output of
tests/golden/make_golden_explainer_bytes.py's groups (that file lists them), run here through the generator's own group functions, and
the library call names of every recorded step (`explain_batch_replay`): the same kernels in the same order.  A changed digest of a
group's INPUTS is reported as such - the CPU draw changed, not the explainer.

The JSON was recorded from the explainers of 3939969, the commit before the two engines and the two drop-in families were put on
shared bases (explainers/engine_base.py, explainers/dropin.py); `recorded_from_commit` in the file says so, and every case was
bit-stable over two runs in fresh processes there.  The graph groups' later replays (`*_call1`) were added afterwards: their digests are
the eager step's on the same inputs (GRAPH_NOTE of the generator).  To regenerate - only from a checkout whose bytes are meant to be kept, never to
make a failing tree pass:

    python tests/golden/make_golden_explainer_bytes.py --commit <hash of that checkout>"""
import json
import sys

import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_explainer_bytes as G  # noqa: E402


def _golden():
    with open(G.JSON) as f:
        return json.load(f)


@pytest.mark.parametrize("group", list(G.GROUPS))
def test_bytes_are_the_recorded_ones(group):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    golden = _golden()
    want = golden["cases"][group]
    digest, got, calls = G.GROUPS[group]()
    torch.cuda.synchronize()
    assert digest == want["inputs"], f"{group}: the INPUTS changed (the draw or the fixture is not the recorded one), nothing is known about the explainer"
    assert sorted(got) == sorted(want["outputs"]), f"{group}: the outputs are not the recorded set"
    changed = [name for name in got if got[name] != want["outputs"][name]]
    assert not changed, f"{group}: {len(changed)} of {len(got)} outputs differ from the bytes recorded at {golden['recorded_from_commit']}: " + ", ".join(changed)
    assert calls == want["recorded_calls"], f"{group}: a recorded step issues other library calls than at {golden['recorded_from_commit']}"


def test_the_golden_holds_every_case():
    golden = _golden()
    assert sorted(golden["cases"]) == sorted(G.GROUPS) and golden["graph_note"] == G.GRAPH_NOTE
    n = {"aoa_bu": 2 * (2 + 2) + 3, "aoa_bu_graph": 2 * 2, "gridtd_resnet_mode0": 4 + 6 + 4, "gridtd_resnet_mode1": 4 + 6 + 4,
         "gridtd_vgg": 2 * (2 + 4) + 2, "gridtd_vgg_graph": 2, "aoa_vgg": 2 * (2 + 4), "dropin_gridtd": 5 * 8, "dropin_aoa": 5 * 9}
    for name, c in golden["cases"].items():
        assert len(c["outputs"]) == n[name], name
    # a recorded step per head (bottom-up AoA) / one (gridTD): the call names are kept, and they are launches
    assert [len(c) for c in golden["cases"]["aoa_bu"]["recorded_calls"]] == [23, 23] and len(golden["cases"]["gridtd_vgg"]["recorded_calls"]) == 1
    assert all(name.startswith("lrpx_") for g in golden["cases"].values() for c in g["recorded_calls"] for name in c)
    # a later replay of a captured graph gives the bytes of the eager step of the same inputs - here: of the recorded step, its equal
    for graph, eager, pairs in (("aoa_bu_graph", "aoa_bu", [("graph_h%d_call%d" % (h, k), "replay_h%d_call%d" % (h, k)) for h in (2, 5) for k in (0, 1)]),
                                ("gridtd_vgg_graph", "gridtd_vgg", [("graph_call%d" % k, "replay_call%d" % k) for k in (0, 1)])):
        for a, b in pairs:
            assert golden["cases"][graph]["outputs"][a] == golden["cases"][eager]["outputs"][b], (graph, a)
