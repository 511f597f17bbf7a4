"""The general alpha-beta rule of a conv directly under a 2x2 max-pool on the CPU, shared by tests/test_vgg_ab_host.py
and tests/test_gpu_vgg_ab.py:

  * the tensors of the kernel tests of `lrpx_conv_geom_ab_pool` / `lrpx_conv_geom_ab_pool_b6` and the operation they implement - the
    FOLDED formulation: the relevance behind the pool read at (oh >> 1, ow >> 1), the pool's winner factor inside qp / qn - in any
    precision and from bf16 plane products;
  * the LAYERED rule it must equal: Pool2d rule (LRPtools/lrp_modules.py:182-195), then the Conv2d rule (:124-150).

3x3 stride 1 padding 1 convs, 2 images, 3 maps on [1, 0, 1].  The pool's input is quantised to halves, so that ties and all-zero
windows occur; at 11 x 9 the last row and column lie under no window (the pooled map is 5 x 4).  r carries a heavy tail,
randn exp(2 randn), as in tests/resnet_ab_cases.py."""
import torch
import torch.nn.functional as F

from fp64_anchor import emulate

ALPHA, BETA = 2., 1.
N_MAPS, MAP2IMG = 3, [1, 0, 1]
RUNS = ((True, BETA), (False, BETA), (True, 0.))        # (addend, beta) of every kernel run of a case
SIZES = {"10x6": (10, 6), "11x9": (11, 9)}

# (id, kr, n_oc, (oh, ow), first): kr below a K chunk of 32, with the W+ / W- boundary inside a chunk, above one chunk; n_oc across the
# 64-column tile; the first-layer form n_oc = 8 on the split image [x+ | x- | 0 0]
EDGE_CASES = [("c%s_%d_%d" % (sname, kr, n_oc), kr, n_oc, hw, False) for sname, hw in SIZES.items() for kr in (4, 20, 36, 52)
              for n_oc in (4, 36, 68)]
EDGE_CASES += [("first%s_%d" % (sname, kr), kr, 8, hw, True) for sname, hw in SIZES.items() for kr in (4, 20, 36, 52)]
# conv4_3's shape and conv1_2's, one map on one image each (the GPU test alone: the host test leaves them to it)
PROD_CASES = [("conv4_3", 512, 512, (28, 28), False), ("conv1_2", 64, 64, (224, 224), False)]
# The draw of a case whose first draw is not fit for the criterion of tests/fp64_anchor.py (tests/test_vgg_ab_host.py decides that on the
# CPU, over all three runs of a case: `fit`): the first later draw that is.  Found with `python tests/vgg_ab_cases.py`.
REDRAW = {'c11x9_20_68': 1, 'c11x9_52_4': 1, 'first11x9_36': 1}
_CACHE = {}


def _safe(z):
    return z + 1e-7 * (z == 0).to(z.dtype)


def winners(a):
    """(n, c, oh, ow) 0 / 1: the first maximum of every 2x2 window (F.max_pool2d's own choice) where that maximum is non-zero; pixels
    of a last odd row / column lie under no window: 0"""
    pooled, idx = F.max_pool2d(a, 2, 2, return_indices=True)
    hit = (pooled != 0).to(a.dtype).flatten(2)
    return torch.zeros_like(a).flatten(2).scatter_(2, idx.flatten(2), hit).view(a.shape)


def coef(c, dtype):
    """(qp, qn) = win / safe(Z+), win / safe(Z-) of the case in `dtype`, Z+- = conv(xs, rows+-)"""
    xs, rows, kr = c["xs"].to(dtype), c["rows"].to(dtype), c["kr"]
    win = winners(c["a"].to(dtype))
    return win / _safe(F.conv2d(xs, rows[:kr], padding=1)), win / _safe(F.conv2d(xs, rows[kr:], padding=1))


def case(name, n_img=2, n_maps=N_MAPS):
    """dict of the CPU tensors (NCHW) of one case, built once per process and shared, read-only.  xs the conv's input (the first-layer
    form: the split image), rows (2 kr, n_oc, 3, 3) = [W+ ; W-], a (n_img, kr, oh, ow) the pool's input, r (n_maps, kr, oh // 2, ow // 2)
    the relevance behind the pool, qp / qn the fp32 coefficients."""
    if name in _CACHE:
        return _CACHE[name]
    _, kr, n_oc, (h, w_), first = next(c for c in EDGE_CASES + PROD_CASES if c[0] == name)
    cin = 3 if first else n_oc
    g = torch.Generator().manual_seed(9000 + 7 * h + 3 * kr + n_oc + 100003 * REDRAW.get(name, 0))
    wt = torch.randn(kr, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    x = torch.randn(n_img, cin, h, w_, generator=g)
    if not first:
        x = x.clamp(min=0)
    a = (torch.randn(n_img, kr, h, w_, generator=g).clamp(min=0) * 2).round() / 2
    r = torch.randn(n_maps, kr, h // 2, w_ // 2, generator=g)
    r = r * torch.exp(2 * torch.randn(n_maps, kr, h // 2, w_ // 2, generator=g))
    addend = torch.randn(n_maps, n_oc, h, w_, generator=g) * 0.1
    wp, wn = wt.clamp(min=0), wt.clamp(max=0)
    if first:       # the split image [x+ | x- | 0 0] against the rows [W+ | W- | 0 0 ; W- | W+ | 0 0]
        zx, zw = torch.zeros(n_img, 8 - 2 * cin, h, w_), torch.zeros(kr, 8 - 2 * cin, 3, 3)
        xs = torch.cat([x.clamp(min=0), x.clamp(max=0), zx], 1)
        rows = torch.cat([torch.cat([wp, wn, zw], 1), torch.cat([wn, wp, zw], 1)], 0)
    else:
        xs, rows = x, torch.cat([wp, wn], 0)
    c = dict(name=name, kr=kr, n_oc=n_oc, hw=(h, w_), xs=xs, rows=rows, a=a, r=r, addend=addend,
             map2img=MAP2IMG if n_maps == N_MAPS else list(range(n_maps)))
    c["qp"], c["qn"] = coef(c, torch.float32)
    _CACHE[name] = c
    return c


def upsample(c, r):
    """r (m, kr, oh // 2, ow // 2) -> (m, kr, oh, ow): every pooled pixel over its window, zeros under no window"""
    h, w_ = c["hw"]
    up = r.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return F.pad(up, (0, w_ - up.shape[3], 0, h - up.shape[2]))


def reference(c, dtype, pairs=None, addend=True, alpha=ALPHA, beta=BETA, q=None):
    """The folded formulation, NCHW: out[m] = xs[img] * convT([(R qp[img]) alpha | (R qn[img]) (-beta)], [W+ ; W-]) (+ addend[m]) with
    R[m, k, oh, ow] = r[m, k, oh >> 1, ow >> 1].  pairs=None: plainly in `dtype` (q: the coefficients, default the case's fp32 ones
    cast); otherwise in fp64 from those plane products of the operand formed in fp32 in the kernel's order and the fp32 rows.
    beta == 0: the W+ half alone."""
    m2i, kr = c["map2img"], c["kr"]
    shape = (c["r"].shape[0], c["n_oc"]) + c["hw"]
    convT = lambda a, wt: torch.nn.grad.conv2d_input(shape, wt, a, padding=1)
    dual = beta != 0.

    def operand(dt, qp, qn):
        r = upsample(c, c["r"].to(dt))
        pos = (r * qp[m2i]) * alpha
        return torch.cat([pos, (r * qn[m2i]) * (-beta)], 1) if dual else pos
    if pairs is None:
        qp, qn = (c["qp"].to(dtype), c["qn"].to(dtype)) if q is None else q
        rows = c["rows"].to(dtype)
        back = convT(operand(dtype, qp, qn), rows if dual else rows[:kr])
    else:
        assert dtype == torch.float64 and q is None
        back = emulate(convT, operand(torch.float32, c["qp"], c["qn"]), c["rows"] if dual else c["rows"][:kr], pairs)
    out = c["xs"].to(dtype)[m2i] * back
    return out + c["addend"].to(dtype) if addend else out


def layered(c, dtype, alpha=ALPHA, beta=BETA):
    """The reference's two steps in `dtype`: the Pool2d rule - the winner of each window gets x_w (R / safe(x_w)) - then the Conv2d rule
    R_in = xs (alpha convT(R / safe(Z+), W+) - beta convT(R / safe(Z-), W-)).  No addend."""
    m2i, kr = c["map2img"], c["kr"]
    xs, rows, a, r = (c[n].to(dtype) for n in ("xs", "rows", "a", "r"))
    pooled, idx = F.max_pool2d(a, 2, 2, return_indices=True)
    s = r / _safe(pooled[m2i])
    r_full = a[m2i] * F.max_unpool2d(s, idx[m2i], 2, 2, output_size=a.shape[-2:])
    zp, zn = F.conv2d(xs, rows[:kr], padding=1), F.conv2d(xs, rows[kr:], padding=1)
    shape = (r.shape[0], c["n_oc"]) + c["hw"]
    convT = lambda t, wt: torch.nn.grad.conv2d_input(shape, wt, t, padding=1)
    return xs[m2i] * (alpha * convT(r_full / _safe(zp[m2i]), rows[:kr]) - beta * convT(r_full / _safe(zn[m2i]), rows[kr:]))


def cached(c, what, fn):
    """per-case CPU results, computed once per process"""
    key = (c["name"], what)
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def fit(c):
    """(worst six-product error / bound, least witness margin) of a case over its RUNS: with and without the addend, and the W+ half
    alone (beta = 0)"""
    from conftest import rel_err
    from fp64_anchor import C, FLOOR, SIX, THREE
    worst, least = 0., float("inf")
    for addend, beta in RUNS:
        kw = dict(addend=addend, beta=beta)
        ref64 = reference(c, torch.float64, **kw)
        bound = C * max(rel_err(reference(c, torch.float32, **kw), ref64), FLOOR)
        worst = max(worst, rel_err(reference(c, torch.float64, SIX, **kw), ref64) / bound)
        least = min(least, rel_err(reference(c, torch.float64, THREE, **kw), ref64) / bound)
    return worst, least


if __name__ == "__main__":      # prints the REDRAW table: per case the first draw that is fit (margin kept clear of the limit: 2.5)
    import sys
    table = {}
    specs = EDGE_CASES + (PROD_CASES if "--prod" in sys.argv else [])
    for spec in specs:
        for draw in range(64):
            REDRAW[spec[0]] = draw
            _CACHE.pop(spec[0], None)
            worst, least = fit(case(spec[0], 1, 1) if spec in PROD_CASES else case(spec[0]))
            if worst <= 1 and least >= 2.5:
                break
        else:
            raise SystemExit("no fit draw for " + spec[0])
        if draw:
            table[spec[0]] = draw
    print("REDRAW =", table)
