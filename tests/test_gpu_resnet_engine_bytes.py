"""The batched bottleneck-ResNet encoder engine (ops.ResNetEncoder in both conv modes) and the elementwise entries of
csrc/resnet_engine.hip give the bytes they gave when tests/golden/resnet_engine_bytes.json was recorded: sha256 of every output of
tests/golden/make_golden_resnet_engine_bytes.py's cases (that file lists them), run here through the generator's own case functions.
A changed digest of a case's INPUTS is reported as such - the CPU draw changed, not the engine.

The JSON was recorded from an untouched checkout of 8fcfe30 (library and ops.py), the commit before the engine's three per-map walks,
the three transposed-direction wrappers and the two pool gather kernels were folded into one each; `recorded_from_commit` in the file
says so.  To regenerate - only from a checkout whose bytes are meant to be kept, never to make a failing tree pass:

    python tests/golden/make_golden_resnet_engine_bytes.py --commit <hash of that checkout>"""
import json
import sys

import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_resnet_engine_bytes as G  # noqa: E402


def _golden():
    with open(G.JSON) as f:
        return json.load(f)


def test_bytes_are_the_recorded_ones():
    from lrp_amd import _lib, ops
    golden = _golden()
    assert golden["fill"] == "0x%08X" % G.FILL
    changed, total = [], 0
    for case, fn in G.CASES.items():
        want = golden["cases"][case]
        digest, got = fn(ops, _lib)
        torch.cuda.synchronize()
        assert digest == want["inputs"], f"{case}: the INPUTS changed (the draw or the fixture is not the recorded one), nothing is known about the engine"
        assert sorted(got) == sorted(want["outputs"]), f"{case}: the outputs are not the recorded set"
        changed += [f"{case}/{name}" for name in got if got[name] != want["outputs"][name]]
        total += len(got)
        if case.startswith("engine_"):
            assert got["trace"] == got["trace_after"], f"{case}: a per-map pass wrote into the trace"
    assert not changed, f"{len(changed)} of {total} outputs differ from the bytes recorded at {golden['recorded_from_commit']}: " + ", ".join(changed)


def test_the_golden_holds_every_case():
    golden = _golden()
    assert sorted(golden["cases"]) == sorted(G.CASES)
    per = {"engine": 5 + len(G.ALPHA_BETA) + 5, "pool": 5, "coef": 3, "per_map": 6}
    for name, c in golden["cases"].items():
        assert len(c["outputs"]) == per[[k for k in per if name.startswith(k)][0]], name
