"""`lrpx_expand_maps` alone (csrc/lrpx_expand.hip; `ops.expand_maps`): a feature-resolution heat map at image size.

Two bit-level contracts - the raw output is the factor `lrpx_guided_gradcam` multiplies by, the normalised output is
`lrpx_project_maxabs` of the raw one - and one numeric bound against the oracle's restatement of `skimage.transform.pyramid_expand`,
evaluated in float64 (oracle/lrp_oracle.py: `pyramid_expand`).

The bound.  E = M a M^T with M (hw, p) >= 0 and unit row sums, so |E| <= max|a|.  u = 2^-24.  The kernel forms tmp = M a and E = tmp M^T
with one fmaf chain of p terms each: (p + 1) u max|a| per chain covers the p roundings and the fp32 rounding of M's entries (built in
float64, stored fp32); the oracle returns its float64 result as fp32 (1 u) and forms the same operator in another order (1 u):
(2 p + 4) u max|a|.  An fp32 emulation of the kernel's order on the CPU stays at or below 0.30 of that at all five geometries; on an MI355X the kernel
itself stays at or below 0.36 (raw) and 0.27 (normalised).
The normalised map E / m against E_ref / m_ref: |E - E_ref| <= b and |m - m_ref| <= b give 2 b / m_ref, plus the division's u."""
import ctypes as C

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401

pytestmark = pytest.mark.gpu

GEOMS = [(14, 16), (7, 32), (3, 8), (14, 32), (2, 4)]          # (p, upscale)
ROWS = (1, 3, 65)
U = 2.0 ** -24


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _maps(p, rows, heads, seed):
    """(rows, heads, p*p) fp32; row r is of kind r % 4: a peaky softmax-like map, a signed map, an all-zero map, a single spike"""
    rs = np.random.RandomState(seed)
    P = p * p
    x = np.zeros((rows, heads, P), np.float32)
    for r in range(rows):
        for h in range(heads):
            kind = r % 4
            if kind == 0:
                z = rs.standard_normal(P) * 4.0
                e = np.exp(z - z.max())
                x[r, h] = (e / e.sum()).astype(np.float32)
            elif kind == 1:
                x[r, h] = rs.standard_normal(P).astype(np.float32)
            elif kind == 3:
                x[r, h, rs.randint(P)] = np.float32(rs.uniform(0.5, 2.0)) * (1 if h % 2 == 0 else -1)
    return x


def _reduce_heads(x, head):
    """what the reference hands to pyramid_expand: `alphas[t][head]` (evaluation.py:744) or `np.mean(attention, axis=0)` of the (NH, P)
    array (:202), row by row as the reference does it"""
    if head is not None:
        return np.ascontiguousarray(x[:, head])
    if x.shape[1] == 1:
        return np.ascontiguousarray(x[:, 0])
    return np.stack([np.mean(x[r], axis=0) for r in range(x.shape[0])]).astype(np.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("heads", [1, 2, 8])
@pytest.mark.parametrize("p,upscale", GEOMS)
def test_expand_maps_bits_and_bound(p, upscale, heads):
    _need_gpu()
    from lrp_amd import evaluation, ops
    from oracle import lrp_oracle as O
    hw = p * upscale
    x = _maps(p, max(ROWS), heads, seed=100 * p + upscale + heads)
    xd = torch.from_numpy(x).cuda()
    for head in ([None] if heads == 1 else [None, heads - 1]):
        a = _reduce_heads(x, head)
        ad = torch.from_numpy(a).cuda()
        full_raw = full_norm = None
        for rows in sorted(ROWS, reverse=True):
            src = xd[:rows, 0].contiguous() if heads == 1 and rows != 3 else xd[:rows].contiguous()          # (R, P) and (R, 1, P) both
            raw = ops.expand_maps(src, hw, head=head)
            norm = ops.expand_maps(src, hw, head=head, normalize=True)
            assert raw.shape == (rows, hw, hw) and norm.shape == (rows, hw, hw)
            # contract 1: the factor Guided Grad-CAM multiplies by
            want = ops.guided_gradcam(torch.ones(rows, 1, hw, hw, device="cuda"), ad[:rows].contiguous(), p)[:, 0]
            assert torch.equal(_bits(raw), _bits(want)), (p, upscale, heads, head, rows)
            # contract 2: `_project_maxabs` of the raw map
            assert torch.equal(_bits(norm), _bits(evaluation.project_maxabs(raw))), (p, upscale, heads, head, rows)
            # a row's bits do not depend on the batch
            if full_raw is None:
                full_raw, full_norm = raw, norm
            else:
                assert torch.equal(_bits(raw), _bits(full_raw[:rows])) and torch.equal(_bits(norm), _bits(full_norm[:rows]))
        # all-zero maps stay zero, normalised or not
        zero = [r for r in range(max(ROWS)) if r % 4 == 2]
        assert not full_raw[zero].any().item() and not full_norm[zero].any().item()
        # against the oracle in float64, on rows of every kind and the last row
        worst = worst_n = 0.0
        for r in (0, 1, 2, 3, 4, 5, 7, max(ROWS) - 1):
            ref = O.pyramid_expand(torch.from_numpy(a[r].astype(np.float64).reshape(p, p)), upscale).double().numpy()
            amax = float(np.abs(a[r]).max())
            bound = (2 * p + 4) * U * amax
            d = float(np.abs(full_raw[r].cpu().double().numpy() - ref).max())
            assert d <= bound, (p, upscale, heads, head, r, d, bound)
            m = float(np.abs(ref).max())
            if amax > 0:
                worst = max(worst, d / bound)
                dn = float(np.abs(full_norm[r].cpu().double().numpy() - ref / m).max())
                bn = 2 * bound / m + U
                assert dn <= bn, (p, upscale, heads, head, r, dn, bn)
                worst_n = max(worst_n, dn / bn)
                assert float(full_norm[r].abs().max()) == 1.0
        print("expand_maps p %d x %d heads %d head %s: raw %.2f of the bound, normalised %.2f of its bound" % (
            p, upscale, heads, head, worst, worst_n))


def test_expand_maps_out_argument_and_selected_heads():
    """`out=` is written in place; head k of (R, NH, P) equals the (R, P) call on that head, for every k"""
    _need_gpu()
    from lrp_amd import ops
    x = torch.from_numpy(_maps(7, 5, 4, seed=9)).cuda()
    out = torch.full((5, 56, 56), 7.0, device="cuda")
    got = ops.expand_maps(x, 56, head=None, normalize=True, out=out)
    assert got is out and torch.equal(_bits(out), _bits(ops.expand_maps(x, 56, normalize=True)))
    for k in range(4):
        assert torch.equal(_bits(ops.expand_maps(x, 56, head=k)), _bits(ops.expand_maps(x[:, k].contiguous(), 56)))
    with pytest.raises(ValueError):
        ops.expand_maps(x, 56, out=torch.empty(5, 56, 57, device="cuda"))


def test_expand_maps_refusals_return_einval_before_any_launch():
    _need_gpu()
    from lrp_amd import _lib, ops
    lib = _lib.load()
    maps = torch.zeros(2, 8, 32 * 32, device="cuda")
    m = torch.zeros(512 * 32, device="cuda")
    out = torch.full((2 * 512 * 512,), 3.0, device="cuda")
    st = _lib.stream_ptr()
    P, M, O_ = _lib.ptr(maps), _lib.ptr(m), _lib.ptr(out)
    call = lib.lrpx_expand_maps
    bad = [
        (None, M, O_, 2, 8, -1, 14, 224, 0), (P, None, O_, 2, 8, -1, 14, 224, 0), (P, M, None, 2, 8, -1, 14, 224, 0),       # null pointers
        (P, M, O_, 0, 8, -1, 14, 224, 0), (P, M, O_, 2, 0, -1, 14, 224, 0),                                                   # rows, heads
        (P, M, O_, 2, 8, 8, 14, 224, 0), (P, M, O_, 2, 8, -2, 14, 224, 0),                                                    # head
        (P, M, O_, 2, 8, -1, 1, 16, 0), (P, M, O_, 2, 8, -1, 33, 33 * 4, 0),                                                  # p outside 2..32
        (P, M, O_, 2, 8, -1, 14, 225, 0), (P, M, O_, 2, 8, -1, 14, 0, 0),                                                     # hw
        (P, M, O_, 2, 8, -1, 14, 224, 2),                                                                                     # normalize
        (P, M, O_, 2, 8, -1, 32, 512, 1),                                                                                     # 69 696 bytes of LDS
    ]
    for args in bad:
        assert call(*args, st) == _lib.EINVAL, args
        assert b"expand_maps" in lib.lrpx_last_error_string()
    torch.cuda.synchronize()
    assert (out == 3.0).all().item()
    # p = 32 at 448 x 448 fits the LDS and runs, and so does p = 14 at 448 x 448
    assert call(P, M, O_, 1, 8, -1, 32, 448, 1, st) == _lib.OK          # 61 504 bytes
    assert ops.expand_maps(torch.zeros(1, 196, device="cuda"), 448).shape == (1, 448, 448)
    # a host pointer is refused by name, not dereferenced
    host = torch.zeros(4, 196)
    assert call(C.c_void_p(host.data_ptr()), M, O_, 1, 1, -1, 14, 224, 0, st) == _lib.EINVAL
    assert b"maps" in lib.lrpx_last_error_string()
    torch.cuda.synchronize()
