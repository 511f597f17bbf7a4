"""The Winograd F(2x2,3x3) relevance conv of conv mode 1 (csrc/conv_wino_b6.h) through ops.conv_mfma with EPI_REL_MUL and the
switch on (lrpx_set_b6_wino), at the smallest shapes that can still go wrong: 49 / 147 tiles of 14 x 14 maps (fragments straddle
maps, ragged last workgroup), 28 x 28 with a map2img table, one and three k-steps (double-buffer parity), one and two
64-channel tiles, 56 x 56 once.  Reference: fp64_anchor.rel_mul in fp64 / fp32 / the three-product witness under fp32_grade with
the default C; invariants bit for bit; each bit of the switch moves exactly its map size."""
import pytest
import torch
import torch.nn.functional as F

import fp64_anchor as A

pytestmark = pytest.mark.gpu

# (hw, map2img, K, n_oc)
SHAPES = [(14, [0], 16, 64), (14, [0, 0, 0], 48, 128), (28, [1, 0, 1], 48, 64), (28, [1, 0, 1], 16, 128), (56, [0], 32, 64)]
KINDS = ("heavy", "ring", "corners")
BIT = {56: 1, 28: 2, 14: 4}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import ops as o
    prev = o.set_b6_wino(7)
    yield o
    o.set_b6_wino(prev)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


_CASES = {}


def make_case(hw, m2i, K, n_oc, kind):
    """x >= 0, W with two dead output channels (all weights negative: Z+ == 0, S = R / 1e-7 meets W+ == 0), heavy-tailed targets;
    ring / corners: S non-zero only on the border ring / in the four corners (padding and halo of the 4 x 4 patches)"""
    key = (hw, tuple(m2i), K, n_oc, kind)
    if key in _CASES:
        return _CASES[key]
    n_maps, n_img = len(m2i), max(m2i) + 1
    g = torch.Generator().manual_seed(hw * 1000 + K * 10 + n_oc + len(kind))
    x = torch.randn(n_img, n_oc, hw, hw, generator=g).clamp(min=0)
    w = torch.randn(K, n_oc, 3, 3, generator=g) * 0.05
    w[1], w[5] = -w[1].abs(), -w[5].abs()
    wp = w.clamp(min=0)
    z = F.conv2d(x, wp, padding=1)
    assert (z[:, 1] == 0).all() and (z[:, 5] == 0).all()
    r = torch.randn(n_maps, K, hw, hw, generator=g) * torch.exp(4 * torch.randn(n_maps, K, hw, hw, generator=g))
    mask = torch.ones(hw, hw)
    if kind == "ring":
        mask[1:-1, 1:-1] = 0
    elif kind == "corners":
        mask[:] = 0
        mask[0, 0] = mask[0, -1] = mask[-1, 0] = mask[-1, -1] = 1
    s = (A.safe_div(r, z[m2i]) * mask).float()
    assert torch.isfinite(s).all()
    _CASES[key] = (x, w, wp, s)
    return _CASES[key]


def launch(ops, x, w, s, hw, m2i, K, n_oc, wino=True, tile_group=0, packed=None):
    from lrp_amd import _lib
    dev = "cuda"
    n_maps = len(m2i)
    wb, ww = packed if packed else (ops.pack_weights_bf16x3(w.to(dev), K, n_oc, _lib.PACK_BWD_POS),
                                    ops.pack_weights_wino_b6(w.to(dev), K, n_oc, _lib.PACK_BWD_POS))
    out = torch.full((n_maps, hw * hw, n_oc), float("nan"), device=dev)
    ops.conv_mfma(_nhwc(s).to(dev), wb, n_maps, hw, K, n_oc, 9, _lib.EPI_REL_MUL, oc_split=n_oc, x=_nhwc(x).to(dev),
                  map2img=torch.tensor(m2i, dtype=torch.int32, device=dev), out1=out, bf16x6=1, tile_group=tile_group,
                  wpacked_wino=ww if wino else None)
    torch.cuda.synchronize()
    return out.cpu().view(n_maps, hw, hw, n_oc).permute(0, 3, 1, 2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"hw{h}_m{len(m)}_k{k}_oc{o}" for h, m, k, o in SHAPES])
def test_wino_launch_is_fp32_grade(ops, shape, kind):
    hw, m2i, K, n_oc = shape
    x, w, wp, s = make_case(hw, m2i, K, n_oc, kind)
    got = launch(ops, x, w, s, hw, m2i, K, n_oc)
    assert torch.isfinite(got).all()
    direct = launch(ops, x, w, s, hw, m2i, K, n_oc, wino=False)
    assert not torch.equal(got, direct), "the Winograd kernel did not run"
    for i in range(len(m2i)):
        xi, si = x[m2i[i]:m2i[i] + 1], s[i:i + 1]
        ref64 = A.rel_mul(xi.double(), si.double(), wp.double())
        ref32 = A.rel_mul(xi, si, wp)
        three = A.rel_mul(xi, si, wp, A.THREE)
        A.fp32_grade(got[i:i + 1], ref64, ref32, three, f"b6 wino hw {hw} K {K} n_oc {n_oc} {kind} map {i}")


@pytest.mark.parametrize("shape", SHAPES[1:3], ids=["hw14", "hw28"])
def test_wino_invariants_bit_for_bit(ops, shape):
    """the same launch twice; targets times 2^k; a map alone against the map inside the batch; the tile-group hint"""
    from lrp_amd import _lib
    hw, m2i, K, n_oc = shape
    x, w, wp, s = make_case(hw, m2i, K, n_oc, "heavy")
    packed = (ops.pack_weights_bf16x3(w.cuda(), K, n_oc, _lib.PACK_BWD_POS), ops.pack_weights_wino_b6(w.cuda(), K, n_oc, _lib.PACK_BWD_POS))
    base = launch(ops, x, w, s, hw, m2i, K, n_oc, packed=packed)
    assert torch.equal(base, launch(ops, x, w, s, hw, m2i, K, n_oc, packed=packed))
    for k in (-40, 17, 40):
        scaled = launch(ops, x, w, s * 2.0 ** k, hw, m2i, K, n_oc, packed=packed)
        assert torch.isfinite(scaled).all() and torch.equal(scaled, base * 2.0 ** k), k
    for i in range(len(m2i)):
        alone = launch(ops, x[m2i[i]:m2i[i] + 1], w, s[i:i + 1], hw, [0], K, n_oc, packed=packed)
        assert torch.equal(alone[0], base[i]), i
    if len(set(m2i)) == 1:
        assert torch.equal(base, launch(ops, x, w, s, hw, m2i, K, n_oc, tile_group=len(m2i), packed=packed))
    else:       # (one map per group: the hint is legal for any table)
        assert torch.equal(base, launch(ops, x, w, s, hw, m2i, K, n_oc, tile_group=1, packed=packed))


def test_packed_u_is_the_rounded_fp64_value(ops):
    """lrpx_pack_weights_wino_b6 against the host evaluation (tests/wino_emulation.py): the three planes, read back from the
    fragment layout [ocb][xi][k-step][plane][lane][8], are the exact split of fp32(G g G^T in fp64)"""
    import wino_emulation as W
    from lrp_amd import _lib
    K, n_oc = 48, 64
    g = torch.Generator().manual_seed(3)
    w = torch.randn(K, n_oc, 3, 3, generator=g)
    blob = ops.pack_weights_wino_b6(w.cuda(), K, n_oc, _lib.PACK_BWD_POS).cpu()
    planes = blob.view(n_oc // 32, 16, K // 16, 3, 2, 32, 8)          # ocb, xi, ks, plane, k half, channel, j
    planes = planes.permute(3, 1, 2, 4, 6, 0, 5).reshape(3, 16, K, n_oc)     # plane, xi, co = 16 ks + 8 half + j, ci = 32 ocb + channel
    got = (planes.view(torch.bfloat16)).float()
    want = torch.stack(A.bf16_split3(W.wino_u(w.clamp(min=0))))
    assert torch.equal(got, want)


def test_each_switch_bit_moves_exactly_its_map_size(ops):
    """with a bit off the launch is the direct kernel's, bit for bit (what the library computed before the Winograd kernel)"""
    cases = {hw: (hw, m2i, K, n_oc) for hw, m2i, K, n_oc in (SHAPES[4], SHAPES[2], SHAPES[0])}
    direct, data = {}, {}
    for hw, (_, m2i, K, n_oc) in cases.items():
        data[hw] = make_case(hw, m2i, K, n_oc, "heavy")
        x, w, wp, s = data[hw]
        direct[hw] = launch(ops, x, w, s, hw, m2i, K, n_oc, wino=False)
    try:
        for bits in (0, 1, 2, 4):
            ops.set_b6_wino(bits)
            for hw, (_, m2i, K, n_oc) in cases.items():
                x, w, wp, s = data[hw]
                got = launch(ops, x, w, s, hw, m2i, K, n_oc)
                assert torch.equal(got, direct[hw]) == (not (bits & BIT[hw])), (bits, hw)
    finally:
        ops.set_b6_wino(7)
