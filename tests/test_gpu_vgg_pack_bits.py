"""lrpx_vgg16_pack writes the blob it wrote when tests/golden/vgg_pack_parent_bits.json was recorded - from the commit named in that
file, before the layout and the packer became two walks over one list of the blob's regions: same size, and over a ZERO-FILLED blob the
same sha256 of every byte (offsets, contents and the gaps nobody writes).  A second pack into a fresh zeroed blob gives the same bits.
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
import make_golden_vgg_pack_bits as G  # noqa: E402


def test_the_packed_blob_has_the_recorded_bits():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    with open(G.JSON) as f:
        golden = json.load(f)
    assert len(golden["recorded_from_commit"]) == 40
    assert G.inputs()["digest"] == golden["inputs"], "the INPUTS changed (the CPU draw of this numpy is not the recorded one), nothing is known about the library"
    blob = G.pack()
    assert blob.numel() * 4 == golden["blob_bytes"]
    assert G.sha_sliced(blob) == golden["sha256"], "not the blob of the build recorded at " + golden["recorded_from_commit"]
    assert G.same_bits(blob, G.pack()), "a second pack gives other bits"
