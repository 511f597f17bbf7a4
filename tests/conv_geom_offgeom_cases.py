"""The runtime-geometry contraction engine (csrc/conv_geom_kernel.h) at geometries outside ResNet-50's, on the CPU: the geometry table,
seeded tensor builders and the operation of every entry (lrpx_conv_geom, _ex, _ab, _grad and their _b6 forms) in any dtype and from bf16
plane products, with (sh, sw) / (ph, pw) tuples throughout.  Shared by tests/test_conv_geom_offgeom_host.py, which decides on the CPU
that exactly these tensors are fit for the criterion of tests/fp64_anchor.py (the six-product emulation passes the bound), and
tests/test_gpu_conv_geom_offgeom.py, which builds them with the same functions.

These are placement tests - a misplaced element is an O(1) error - so the data is plain randn and no witness margin is asked."""
import torch
import torch.nn.functional as F

from fp64_anchor import emulate

# id: ((kh, kw, sh, sw, ph, pw), (H, W)) - each the smallest that shows its edge
GEOMS = {
    "k2s2": ((2, 2, 2, 2, 0, 0), (11, 13)),       # even kernel; the last row and column are reached by no window
    "k4s4": ((4, 4, 4, 4, 0, 0), (11, 13)),       # 16 classes of one tap each; three trailing rows unreached
    "k5s3p2": ((5, 5, 3, 3, 2, 2), (11, 13)),     # classes with 2 and with 1 taps per axis
    "k3p0": ((3, 3, 1, 1, 0, 0), (11, 13)),       # valid conv
    "k1p1": ((1, 1, 1, 1, 1, 1), (11, 13)),       # padding beyond the kernel: the output is larger than the input
    "k3s2p2": ((3, 3, 2, 2, 2, 2), (11, 13)),     # padding above k // 2 with a stride
    "rect": ((3, 5, 2, 3, 1, 2), (11, 13)),       # everything rectangular, sh != sw, both above 1
    "k7x1": ((7, 1, 2, 1, 3, 0), (11, 13)),       # a 1-D kernel
    "gap": ((2, 3, 3, 2, 1, 0), (2, 13)),         # a stride above the kernel with padding; H < sh: class row 2 has no pixels
    "k11s4": ((11, 11, 4, 4, 2, 2), (23, 19)),    # 121 taps
    "rect_5x3": ((3, 5, 2, 3, 1, 2), (5, 3)),     # five maps on three images: a 64-pixel tile spans every map
}
MAPS = {"rect_5x3": (3, [2, 0, 1, 0, 2])}         # (n_img, map2img); every other row: three maps on two images
DEFAULT_MAPS = (2, [1, 0, 1])
UNREACHED = ("k2s2", "k4s4", "gap")               # geometries with output pixels of the transposed direction that no window reaches
CHANNELS = [(k, n_oc) for k in (4, 36) for n_oc in (3, 40, 72)]       # at 72 the fourth 32-column block is an idle wave
AB_CHANNELS = [(kr, n_oc) for kr in (4, 36) for n_oc in (4, 40)]
ALPHA, BETA = 2., 1.
# entry: does it have a _b6 form
ENTRIES = {"fwd": True, "plain": False, "ex": True, "ex_noadd": True, "grad_full": True, "grad_none": True}
AB_ENTRIES = {"ab_single": True, "ab_dual": True}
# The draw of a dual alpha-beta case whose first draw is not fit for the criterion (W+ against W- cancels): the first later draw whose
# six-product emulation passes the bound.  Found with `python tests/conv_geom_offgeom_cases.py`.
REDRAW = {}
_CACHE = {}


def maps_of(gid):
    return MAPS.get(gid, DEFAULT_MAPS)


def out_hw(gid):
    (kh, kw, sh, sw, ph, pw), (h, w) = GEOMS[gid]
    return (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1


def unreached(gid):
    """bool (H, W): the pixels of the conv's input that no window reaches, by the index arithmetic alone"""
    (kh, kw, sh, sw, ph, pw), (h, w) = GEOMS[gid]
    oh, ow = out_hw(gid)
    rows = torch.tensor([not any(0 <= y + ph - r < oh * sh and (y + ph - r) % sh == 0 for r in range(kh)) for y in range(h)])
    cols = torch.tensor([not any(0 <= x + pw - s < ow * sw and (x + pw - s) % sw == 0 for s in range(kw)) for x in range(w)])
    return rows[:, None] | cols[None, :]


def case(gid, k, n_oc):
    """dict of the CPU tensors (NCHW) of one geometry at contraction length k and n_oc columns, built once per process and shared,
    read-only.  Transposed direction: w (k, n_oc, kh, kw) is a conv weight (cout = k, cin = n_oc), r the per-map operand, q / mask per
    image on the conv's output map, x per image and addend per map on its input map, scale per channel.  Forward direction: wf (n_oc, k,
    kh, kw), xin (n maps, k, H, W), bias (n_oc,)."""
    key = (gid, k, n_oc)
    if key in _CACHE:
        return _CACHE[key]
    geom, (h, w_) = GEOMS[gid]
    kh, kw = geom[:2]
    oh, ow = out_hw(gid)
    n_img, m2i = maps_of(gid)
    n = len(m2i)
    g = torch.Generator().manual_seed(9000 + 101 * list(GEOMS).index(gid) + 7 * k + n_oc)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = dict(gid=gid, geom=geom, hw=(h, w_), ohw=(oh, ow), k=k, n_oc=n_oc, n=n, n_img=n_img, m2i=m2i,
             w=rn(k, n_oc, kh, kw) * (2.0 / (k * kh * kw)) ** 0.5, r=rn(n, k, oh, ow), q=torch.rand(n_img, k, oh, ow, generator=g) + 0.5,
             x=rn(n_img, n_oc, h, w_), addend=rn(n, n_oc, h, w_) * 0.1, mask=rn(n_img, k, oh, ow), scale=rn(k),
             wf=rn(n_oc, k, kh, kw) * (2.0 / (k * kh * kw)) ** 0.5, xin=rn(n, k, h, w_), bias=rn(n_oc))
    _CACHE[key] = c
    return c


def ab_case(gid, kr, n_oc):
    """the tensors of the alpha-beta entries, as tests/resnet_ab_cases.case builds them: w (kr, n_oc, kh, kw) the conv's weight, rows
    [W+ ; W-], xs >= 0 per image, qp > 0 and qn < 0 like 1 / Z+ and 1 / Z-"""
    key = ("ab", gid, kr, n_oc)
    if key in _CACHE:
        return _CACHE[key]
    geom, (h, w_) = GEOMS[gid]
    kh, kw = geom[:2]
    oh, ow = out_hw(gid)
    n_img, m2i = maps_of(gid)
    n = len(m2i)
    name = "%s_%d_%d" % (gid, kr, n_oc)
    g = torch.Generator().manual_seed(11000 + 101 * list(GEOMS).index(gid) + 7 * kr + n_oc + 100003 * REDRAW.get(name, 0))
    wt = torch.randn(kr, n_oc, kh, kw, generator=g) * (2.0 / (n_oc * kh * kw)) ** 0.5
    c = dict(gid=gid, name=name, geom=geom, hw=(h, w_), ohw=(oh, ow), kr=kr, n_oc=n_oc, n=n, n_img=n_img, m2i=m2i,
             rows=torch.cat([wt.clamp(min=0), wt.clamp(max=0)], 0), xs=torch.randn(n_img, n_oc, h, w_, generator=g).clamp(min=0),
             qp=torch.rand(n_img, kr, oh, ow, generator=g) + 0.5, qn=-(torch.rand(n_img, kr, oh, ow, generator=g) + 0.5),
             r=torch.randn(n, kr, oh, ow, generator=g), addend=torch.randn(n, n_oc, h, w_, generator=g) * 0.1)
    _CACHE[key] = c
    return c


def _strides(c):
    kh, kw, sh, sw, ph, pw = c["geom"]
    return dict(stride=(sh, sw), padding=(ph, pw))


def _back(c, a32, wt32, dtype, pairs):
    """convT(a, wt) onto the conv's input map: plainly in `dtype`, or in fp64 from those plane products of the fp32 operands"""
    shape = (c["n"], c["n_oc"]) + c["hw"]
    convT = lambda a, wt: torch.nn.grad.conv2d_input(shape, wt, a, **_strides(c))
    if pairs is None:
        return convT(a32.to(dtype), wt32.to(dtype))
    assert dtype == torch.float64
    return emulate(convT, a32, wt32, pairs)


def reference(entry, c, dtype, pairs=None):
    """the operation of `entry` on the tensors of `c` (NCHW).  pairs=None: plainly in `dtype` from the fp32 tensors.  Otherwise in fp64
    from those plane products of (the contraction's operand formed in fp32 in the kernel's order, the fp32 weights)."""
    key = (id(c), entry, dtype, pairs)
    if key not in _CACHE:
        _CACHE[key] = _reference(entry, c, dtype, pairs)
    return _CACHE[key]


def _reference(entry, c, dtype, pairs):
    m2i = c["m2i"]
    f = (lambda t: t) if pairs is not None else (lambda t: t.to(dtype))        # operands: fp32 in the kernel's order under emulation
    if entry == "fwd":          # out = conv(xin, wf) + bias
        conv = lambda a, wt: F.conv2d(a, wt, **_strides(c))
        y = conv(c["xin"].to(dtype), c["wf"].to(dtype)) if pairs is None else emulate(conv, c["xin"], c["wf"], pairs)
        return y + c["bias"].to(dtype)[None, :, None, None]
    if entry == "plain":        # lrpx_conv_geom: out[m] = x[m] * convT(r[m], w), x materialised per map
        return c["x"].to(dtype)[m2i] * _back(c, c["r"], c["w"], dtype, pairs)
    if entry in ("ex", "ex_noadd"):     # out[m] = x[img] * convT(r[m] q[img], w) (+ addend[m])
        out = c["x"].to(dtype)[m2i] * _back(c, f(c["r"]) * f(c["q"])[m2i], c["w"], dtype, pairs)
        return out + c["addend"].to(dtype) if entry == "ex" else out
    if entry == "grad_none":    # out[m] = convT(g[m], w)
        return _back(c, c["r"], c["w"], dtype, pairs)
    if entry == "grad_full":    # out[m] = convT(scale * (mask[img] > 0 ? max(g[m], 0) : 0), w) + addend[m]: clamp, mask, scale in this order
        a = f(c["r"]).clamp(min=0) * (c["mask"][m2i] > 0).to(f(c["r"]).dtype) * f(c["scale"])[None, :, None, None]
        return _back(c, a, c["w"], dtype, pairs) + c["addend"].to(dtype)
    if entry == "ab_single":    # out[m] = xs[img] * convT((r[m] qp[img]) alpha, W+)
        a = (f(c["r"]) * f(c["qp"])[m2i]) * ALPHA
        return c["xs"].to(dtype)[m2i] * _back(c, a, c["rows"][:c["kr"]], dtype, pairs)
    if entry == "ab_dual":      # out[m] = xs[img] * convT([(r[m] qp[img]) alpha | (r[m] qn[img]) (-beta)], [W+ ; W-]) + addend[m]
        r = f(c["r"])
        a = torch.cat([(r * f(c["qp"])[m2i]) * ALPHA, (r * f(c["qn"])[m2i]) * (-BETA)], 1)
        return c["xs"].to(dtype)[m2i] * _back(c, a, c["rows"], dtype, pairs) + c["addend"].to(dtype)
    raise KeyError(entry)


def fit(entry, c):
    """six-product error / bound of one entry on one case: <= 1 means a conv mode 1 failure on the GPU is the kernel's"""
    from conftest import rel_err
    from fp64_anchor import C, FLOOR, SIX
    ref64 = reference(entry, c, torch.float64)
    bound = C * max(rel_err(reference(entry, c, torch.float32), ref64), FLOOR)
    return rel_err(reference(entry, c, torch.float64, SIX), ref64) / bound


if __name__ == "__main__":      # prints the REDRAW table: per dual alpha-beta case the first draw that is fit
    table = {}
    for gid in GEOMS:
        for kr, n_oc in AB_CHANNELS:
            name = "%s_%d_%d" % (gid, kr, n_oc)
            for draw in range(64):
                REDRAW[name] = draw
                _CACHE.clear()
                if all(fit(e, ab_case(gid, kr, n_oc)) <= 1 for e in AB_ENTRIES):
                    break
            else:
                raise SystemExit("no fit draw for " + name)
            if draw:
                table[name] = draw
    print("REDRAW =", table)
