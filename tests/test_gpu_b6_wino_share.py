"""Column sharing in the staging of the Winograd relevance conv (csrc/conv_wino_b6.h): a staging thread fetches its
tile's own two patch columns and takes the outer two from lanes -/+ 4 of its wave.  The values that reach the transform are the
ones the legacy staging (lrpx_set_b6_wino bit 8: every thread fetches its whole patch) fetched itself, so every launch is run with
the switch at 7 and at 15 and the two outputs must be the same bits - no tolerance.  S is seeded normal with a distinct value at
every (map, y, x, channel), so a column taken from the wrong lane, row or channel cannot cancel.  Shapes: the smallest at which the
exchange can go wrong - 14 x 14 x 3 maps (TW = 7: the 16 tiles of a wave span three tile rows, fragments straddle maps, the last
workgroup is ragged), 28 x 28 (TW = 14: tile rows do not align with waves; two channel blocks), 56 x 56 (TW = 28: waves inside one
tile row and waves that wrap); S on the border ring / in the corners only (zero padding at tx = 0 and tx = TW - 1); two maps of
one image against each map alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (hw, map2img, K, n_oc)
S14, S28, S56 = (14, [0, 1, 0], 32, 64), (28, [0], 16, 128), (56, [0], 16, 64)
SHAPES = [S14, S28, S56]
_id = lambda s: f"hw{s[0]}_m{len(s[1])}_k{s[2]}_oc{s[3]}"  # noqa: E731


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import ops as o
    return o


def distinct_normal(shape, g):
    """standard normal draws, re-drawn where two elements came out equal: every element is another value"""
    s = torch.randn(shape, generator=g)
    flat = s.view(-1)
    while True:
        srt, idx = flat.sort()
        dup = idx[1:][srt[1:] == srt[:-1]]
        if dup.numel() == 0:
            return s
        flat[dup] = torch.randn(dup.numel(), generator=g)


_CASES = {}


def make_case(hw, m2i, K, n_oc, kind="full"):
    key = (hw, tuple(m2i), K, n_oc, kind)
    if key not in _CASES:
        g = torch.Generator().manual_seed(hw * 1000 + K * 10 + n_oc + len(m2i) + len(kind))
        x = torch.randn(max(m2i) + 1, hw, hw, n_oc, generator=g).clamp(min=0)
        w = torch.randn(K, n_oc, 3, 3, generator=g) * 0.05
        s = distinct_normal((len(m2i), hw, hw, K), g)         # NHWC, as the kernel reads it
        assert s.unique().numel() == s.numel()
        mask = torch.ones(hw, hw)
        if kind == "ring":
            mask[1:-1, 1:-1] = 0
        elif kind == "corners":
            mask[:] = 0
            mask[0, 0] = mask[0, -1] = mask[-1, 0] = mask[-1, -1] = 1
        _CASES[key] = (x, w, s * mask[None, :, :, None])
    return _CASES[key]


def launch(ops, x, s, packed, hw, m2i, K, n_oc, wino=True):
    from lrp_amd import _lib
    n_maps = len(m2i)
    out = torch.full((n_maps, hw * hw, n_oc), float("nan"), device="cuda")
    ops.conv_mfma(s.contiguous().cuda(), packed[0], n_maps, hw, K, n_oc, 9, _lib.EPI_REL_MUL, oc_split=n_oc, x=x.contiguous().cuda(),
                  map2img=torch.tensor(m2i, dtype=torch.int32, device="cuda"), out1=out, bf16x6=1,
                  wpacked_wino=packed[1] if wino else None)
    torch.cuda.synchronize()
    return out.cpu()


def pack(ops, w, K, n_oc):
    from lrp_amd import _lib
    return (ops.pack_weights_bf16x3(w.cuda(), K, n_oc, _lib.PACK_BWD_POS), ops.pack_weights_wino_b6(w.cuda(), K, n_oc, _lib.PACK_BWD_POS))


def both_stagings(ops, x, s, packed, hw, m2i, K, n_oc):
    """the same launch with shared (7) and with legacy (15) staging"""
    prev = ops.set_b6_wino(-1)
    try:
        ops.set_b6_wino(7)
        shared = launch(ops, x, s, packed, hw, m2i, K, n_oc)
        ops.set_b6_wino(15)
        legacy = launch(ops, x, s, packed, hw, m2i, K, n_oc)
    finally:
        ops.set_b6_wino(prev)
    assert torch.isfinite(shared).all() and torch.isfinite(legacy).all()
    return shared, legacy


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_shared_staging_is_the_legacy_staging_bit_for_bit(ops, shape):
    hw, m2i, K, n_oc = shape
    x, w, s = make_case(hw, m2i, K, n_oc)
    packed = pack(ops, w, K, n_oc)
    shared, legacy = both_stagings(ops, x, s, packed, hw, m2i, K, n_oc)
    assert torch.equal(shared, legacy)
    assert shared.abs().sum() > 0
    assert not torch.equal(shared, launch(ops, x, s, packed, hw, m2i, K, n_oc, wino=False)), "the Winograd kernel did not run"


@pytest.mark.parametrize("kind", ("ring", "corners"))
@pytest.mark.parametrize("shape", (S14, S28), ids=_id)
def test_border_ring_and_corners(ops, shape, kind):
    """S non-zero only on the outermost pixel ring / at the four corners: the padding columns at tx = 0 and tx = TW - 1 stay zero"""
    hw, m2i, K, n_oc = shape
    x, w, s = make_case(hw, m2i, K, n_oc, kind)
    shared, legacy = both_stagings(ops, x, s, pack(ops, w, K, n_oc), hw, m2i, K, n_oc)
    assert torch.equal(shared, legacy)
    assert shared.abs().sum() > 0


def test_two_maps_of_one_image_are_each_map_alone(ops):
    """map2img = [0, 0] on 14 x 14: 98 tiles, the second map starts inside a wave; same bits as each map run alone, in both stagings"""
    hw, m2i, K, n_oc = 14, [0, 0], 32, 64
    x, w, s = make_case(hw, m2i, K, n_oc)
    packed = pack(ops, w, K, n_oc)
    shared, legacy = both_stagings(ops, x, s, packed, hw, m2i, K, n_oc)
    assert torch.equal(shared, legacy)
    for i in range(2):
        alone_s, alone_l = both_stagings(ops, x, s[i:i + 1], packed, hw, [0], K, n_oc)
        assert torch.equal(alone_s, alone_l)
        assert torch.equal(alone_s[0], shared[i]), i
