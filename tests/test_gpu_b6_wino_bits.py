"""The Winograd relevance conv (csrc/conv_wino_b6.h) keeps the bits it had when tests/golden/wino_parent_bits.npz was recorded, and what
its staging threads do not fetch never reaches a result.

Same bits: the cases of tests/golden/make_golden_wino_parent_bits.py (that file lists them: one to four K-chunks, so that the prologue,
the steady-state loop and the drain of the staging pipeline all run, on both LDS buffers; a ragged last workgroup; two channel blocks; a
map that starts inside a wave), in both stagings (lrpx_set_b6_wino 15 and 7), torch.equal against the recorded output - or, for the two
larger maps, whose outputs are not stored, its sha256, with the recorded fp64 sum per pixel row saying where a difference lies.  A
changed digest of the INPUTS fails the test as such: the CPU draw changed, nothing is known about the kernel.

No leak: the patch loads are issued by every thread for every patch element, and what must not be fetched (zero padding, the ragged
tail, shared columns) is answered with zero by the range check of the buffer resource.  With the middle one of three 14 x 14 maps all
NaN, maps 0 and 2 are the bits of each map run alone (a neighbour's NaN times zero would be NaN); and with S a view into a larger
allocation whose bytes before and behind it are NaN, the result is finite and the same bits."""
import sys

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_wino_parent_bits as G  # noqa: E402

LEAK = (14, [0, 1, 0], 32, 64)           # (hw, map2img, K, n_oc): 147 tiles, fragments straddle the maps, ragged last workgroup


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden():
    return np.load(G.NPZ)


@pytest.mark.parametrize("staging", G.STAGINGS)
@pytest.mark.parametrize("shape", G.SHAPES, ids=G.name)
def test_same_bits_as_the_recorded_build(ops, golden, shape, staging):
    n = G.name(shape)
    assert G.inputs(shape)[3] == str(golden[n + "/inputs"]), f"{n}: the INPUTS changed (the CPU draw of this torch is not the recorded one), nothing is known about the kernel"
    got = G.run(ops, shape, staging)
    assert torch.isfinite(got).all()
    rows = np.argwhere(G.row_sums(got) != golden[n + "/row_sums"])
    where = f"{n}, staging {staging}: {len(rows)} pixel rows (map, pixel) differ from the build recorded at {golden['recorded_from_commit']}, first {rows[:4].tolist()}"
    if n + "/out" in golden.files:
        assert torch.equal(got, torch.from_numpy(golden[n + "/out"])), where
    assert G.sha(got) == str(golden[n + "/sha256"]), where


def test_the_golden_holds_every_shape(golden):
    assert sorted(k.split("/")[0] for k in golden.files if k.endswith("/sha256")) == sorted(G.name(s) for s in G.SHAPES)


@pytest.fixture(scope="module")
def leak_case(ops):
    """(x, s, packed, {staging: [map 0 alone, map 2 alone]}) of the LEAK shape; S of the middle map is replaced by the caller's copy"""
    hw, m2i, K, n_oc = LEAK
    x, w, s, _ = G.inputs(LEAK)
    packed = G.pack(ops, w, K, n_oc)
    alone = {}
    prev = ops.set_b6_wino(-1)
    try:
        for st in G.STAGINGS:
            ops.set_b6_wino(st)
            alone[st] = [G.launch(ops, x, s[i:i + 1].contiguous().cuda(), packed, hw, [m2i[i]], K, n_oc)[0] for i in (0, 2)]
            assert all(torch.isfinite(a).all() and a.abs().sum() > 0 for a in alone[st])
    finally:
        ops.set_b6_wino(prev)
    assert torch.equal(alone[15][0], alone[7][0]) and torch.equal(alone[15][1], alone[7][1])
    return x, s, packed, alone


def _staged(ops, staging, fn):
    prev = ops.set_b6_wino(-1)
    try:
        ops.set_b6_wino(staging)
        return fn()
    finally:
        ops.set_b6_wino(prev)


@pytest.mark.parametrize("staging", G.STAGINGS)
def test_a_nan_map_between_two_maps_does_not_leak(ops, leak_case, staging):
    hw, m2i, K, n_oc = LEAK
    x, s, packed, alone = leak_case
    s_nan = s.clone()
    s_nan[1] = float("nan")
    got = _staged(ops, staging, lambda: G.launch(ops, x, s_nan.contiguous().cuda(), packed, hw, m2i, K, n_oc))
    assert torch.isnan(got[1]).all()
    assert torch.equal(got[0], alone[staging][0]), "map 0 is not the map run alone"
    assert torch.equal(got[2], alone[staging][1]), "map 2 is not the map run alone"


@pytest.mark.parametrize("staging", G.STAGINGS)
def test_nan_before_and_behind_the_tensor_does_not_leak(ops, leak_case, golden, staging):
    hw, m2i, K, n_oc = LEAK
    x, s, packed, alone = leak_case
    band = 2 * (hw + 2) * K                               # more than a patch row and column beyond either end
    buf = torch.full((s.numel() + 2 * band,), float("nan"), device="cuda")
    buf[band:band + s.numel()] = s.contiguous().view(-1).cuda()
    s_dev = buf[band:band + s.numel()].view(s.shape)
    got = _staged(ops, staging, lambda: G.launch(ops, x, s_dev, packed, hw, m2i, K, n_oc))
    assert torch.isnan(buf[:band]).all() and torch.isnan(buf[-band:]).all()
    assert torch.isfinite(got).all()
    assert torch.equal(got, torch.from_numpy(golden[G.name(LEAK) + "/out"]))
    assert torch.equal(got[0], alone[staging][0]) and torch.equal(got[2], alone[staging][1])
