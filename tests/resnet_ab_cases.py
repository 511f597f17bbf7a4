"""The general alpha-beta rule on the batched ResNet engine on the CPU, shared by tests/test_resnet_ab_host.py and
tests/test_gpu_resnet_ab.py:

  * the tensors of the kernel tests of `lrpx_conv_geom_ab` / `lrpx_conv_geom_ab_b6` and the operation they implement in any precision
    and from bf16 plane products.  The host test decides on the CPU that exactly these tensors are fit for the fp32-grade criterion
    of tests/fp64_anchor.py (the six-product emulation passes the bound, the three-product witness misses it by WITNESS_MARGIN); the
    GPU test builds them with the same functions.  Data as in tests/resnet_b6_cases.py: r carries a heavy tail, exp(2 randn).  W+ and
    W- contributions have opposite signs (qn < 0, scale2 = -beta < 0, W- <= 0 against qp > 0, alpha > 0, W+ >= 0), so they cancel.
  * the DUAL-COEFFICIENT FORMULATION of the whole net in torch (fp64 in the host test): per image qp, qn per conv and (c1, c2) per
    Add; per map one transposed contraction per conv over the stacked rows [W+ ; W-]."""
import torch
import torch.nn.functional as F

from fp64_anchor import emulate

ALPHA, BETA = 2., 1.                     # of the kernel tests
N_MAPS, MAP2IMG = 3, [1, 0, 1]
GEOMS = {"pw": (1, 1, 0), "pws2": (1, 2, 0), "c3": (3, 1, 1), "c3s2": (3, 2, 1)}       # (kernel, stride, padding)

# (id, geometry, kr, n_oc, (h, w)): every kr x n_oc of the issue's lists at every geometry, and the stem on its split image (n_oc 8)
EDGE_CASES = [("%s_%d_%d" % (gname, kr, n_oc), g, kr, n_oc, (11, 9), False)
              for gname, g in GEOMS.items() for kr in (4, 20, 36, 52) for n_oc in (4, 8, 20, 36, 52)]
EDGE_CASES += [("stem7_%d" % kr, (7, 2, 3), kr, 8, (11, 9), True) for kr in (4, 20, 36, 52)]
PROD_CASES = [("pw_2048_512_7", (1, 1, 0), 2048, 512, (7, 7), False), ("c3s2_512_512_14", (3, 2, 1), 512, 512, (14, 14), False)]
# The draw of a case whose first draw is not fit for the criterion (tests/test_resnet_ab_host.py decides that on the CPU, from fp64,
# fp32 and the plane-product emulations alone - W+ against W- cancels, which lifts fp32's own error towards the three-product witness):
# the first later draw that is.  Found with `python tests/resnet_ab_cases.py`.
REDRAW = {'pw_20_52': 1, 'pws2_4_8': 1, 'pws2_52_20': 1, 'pws2_52_52': 2, 'c3_20_4': 1, 'c3_20_20': 1, 'c3_20_36': 1, 'c3_36_4': 1,
          'c3s2_20_4': 1, 'c3s2_36_20': 2, 'c3s2_52_4': 1, 'c3s2_52_8': 1, 'stem7_20': 2, 'stem7_36': 2, 'stem7_52': 1,
          'pw_2048_512_7': 1, 'c3s2_512_512_14': 18}
_CACHE = {}


def case(name):
    """dict of the CPU tensors (NCHW) of one case, built once per process and shared, read-only.  2 images, 3 maps on [1, 0, 1].
    w (kr, cin, k, k) is the conv's weight; x its input (the stem: signed, cin = 3); qp > 0, qn < 0 like 1 / Z+ and 1 / Z-."""
    if name in _CACHE:
        return _CACHE[name]
    _, (k, stride, padding), kr, n_oc, (h, w_), stem = next(c for c in EDGE_CASES + PROD_CASES if c[0] == name)
    cin = 3 if stem else n_oc
    g = torch.Generator().manual_seed(7000 + 131 * k + 17 * stride + 3 * kr + n_oc + 100003 * REDRAW.get(name, 0))
    oh, ow = (h + 2 * padding - k) // stride + 1, (w_ + 2 * padding - k) // stride + 1
    wt = torch.randn(kr, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    x = torch.randn(2, cin, h, w_, generator=g)
    if not stem:
        x = x.clamp(min=0)
    qp = torch.rand(2, kr, oh, ow, generator=g) + 0.5
    qn = -(torch.rand(2, kr, oh, ow, generator=g) + 0.5)
    r = torch.randn(N_MAPS, kr, oh, ow, generator=g)
    r = r * torch.exp(2 * torch.randn(N_MAPS, kr, oh, ow, generator=g))
    addend = torch.randn(N_MAPS, n_oc, h, w_, generator=g) * 0.1
    wp, wn = wt.clamp(min=0), wt.clamp(max=0)
    if stem:        # the split image [x+ | x- | 0 0] against the rows [W+ | W- | 0 0 ; W- | W+ | 0 0]
        zx, zw = torch.zeros(2, 8 - 2 * cin, h, w_), torch.zeros(kr, 8 - 2 * cin, k, k)
        xs = torch.cat([x.clamp(min=0), x.clamp(max=0), zx], 1)
        rows = torch.cat([torch.cat([wp, wn, zw], 1), torch.cat([wn, wp, zw], 1)], 0)
    else:
        xs, rows = x, torch.cat([wp, wn], 0)
    c = dict(name=name, geom=(k, k, stride, stride, padding, padding), kr=kr, n_oc=n_oc, hw=(h, w_), ohw=(oh, ow), xs=xs, rows=rows,
             qp=qp, qn=qn, r=r, addend=addend)
    _CACHE[name] = c
    return c


def reference(c, dtype, pairs=None, addend=True, alpha=ALPHA, beta=BETA):
    """out[m] = xs[img] * convT([(r[m] qp[img]) alpha | (r[m] qn[img]) (-beta)], [W+ ; W-]) (+ addend[m]), img = MAP2IMG[m]; NCHW.
    pairs=None: plainly in `dtype`.  Otherwise in fp64 from those plane products of the operand formed in fp32 in the kernel's order
    and the fp32 weight rows."""
    k, _, s, _, p, _ = c["geom"]
    shape = (N_MAPS, c["n_oc"]) + c["hw"]
    convT = lambda a, wt: torch.nn.grad.conv2d_input(shape, wt, a, stride=s, padding=p)
    if pairs is None:
        r, qp, qn, rows = (c[n].to(dtype) for n in ("r", "qp", "qn", "rows"))
        back = convT(torch.cat([(r * qp[MAP2IMG]) * alpha, (r * qn[MAP2IMG]) * (-beta)], 1), rows)
    else:
        assert dtype == torch.float64
        a32 = torch.cat([(c["r"] * c["qp"][MAP2IMG]) * alpha, (c["r"] * c["qn"][MAP2IMG]) * (-beta)], 1)
        back = emulate(convT, a32, c["rows"], pairs)
    out = c["xs"].to(dtype)[MAP2IMG] * back
    return out + c["addend"].to(dtype) if addend else out


def cached(c, what, fn):
    """per-case CPU results, computed once per process"""
    key = (c["name"], what)
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ---- the whole net in the engine's terms -------------------------------------------------------------------------------------------------
def _safe(z):
    return z + 1e-7 * (z == 0).to(z.dtype)


def ab_trace(plan, x):
    """per IMAGE: activations, qp and qn per conv, (c1, c2) per Add.  NCHW, in the dtype of x and the net."""
    act, qp, qn = {}, {}, {}

    def conv(i, inp, relu):
        cv = plan.convs[i]
        kh, kw, sh, sw, ph, pw = cv["geom"]
        wt, bn = cv["module"].weight.detach(), cv["bn"]
        wp, wn = wt.clamp(min=0), wt.clamp(max=0)
        kw_ = dict(stride=(sh, sw), padding=(ph, pw))
        y = F.conv2d(inp, wt, **kw_)
        if cv["nonneg"]:
            zp, zn = F.conv2d(inp, wp, **kw_), F.conv2d(inp, wn, **kw_)
        else:
            xp, xn = inp.clamp(min=0), inp.clamp(max=0)
            zp = F.conv2d(xp, wp, **kw_) + F.conv2d(xn, wn, **kw_)
            zn = F.conv2d(xn, wp, **kw_) + F.conv2d(xp, wn, **kw_)
        sd = torch.sqrt(bn.running_var + bn.eps)
        w = (bn.weight.detach() / sd)[:, None, None]
        b = (bn.bias.detach() - (bn.running_mean * bn.weight.detach()) / sd)[:, None, None]
        xw = (y * w).abs()
        f = xw / _safe(xw + b.abs())
        qp[i], qn[i] = f / _safe(zp), f / _safe(zn)
        a = y * w + b
        act[i] = a.clamp(min=0) if relu else a
        return act[i]
    pk = plan.pool
    a0 = conv(0, x, True)
    pooled, pool_idx = F.max_pool2d(a0, pk[:2], pk[2:4], pk[4:], return_indices=True)
    outs, coef = [], []
    cur = pooled
    for blk in plan.blocks:
        y3 = conv(blk["conv3"], conv(blk["conv2"], conv(blk["conv1"], cur, True), True), False)
        short = conv(blk["downsample"], cur, False) if blk["downsample"] is not None else cur
        s = y3 + short
        half = 0.5 * (s == 0).to(s.dtype)
        den = s + 0.01 * s.sign()
        coef.append((torch.nan_to_num(y3 / den, nan=0.0) + half, torch.nan_to_num(short / den, nan=0.0) + half))
        cur = s.clamp(min=0)
        outs.append(cur)
    return dict(x=x, act=act, qp=qp, qn=qn, pooled=pooled, pool_idx=pool_idx, outs=outs, coef=coef)


def ab_relevance(plan, tr, r, img, alpha, beta):
    """per MAP: one transposed contraction per conv over kappa in [0, 2 cout), A = [(R qp) alpha | (R qn) (-beta)], rows [W+ ; W-]"""
    sel = lambda t: t[img:img + 1]

    def convT(i, r_out, x_in, stem=False):
        cv = plan.convs[i]
        kh, kw, sh, sw, ph, pw = cv["geom"]
        wt = cv["module"].weight.detach()
        wp, wn = wt.clamp(min=0), wt.clamp(max=0)
        a = torch.cat([(r_out * sel(tr["qp"][i])) * alpha, (r_out * sel(tr["qn"][i])) * (-beta)], 1)
        if stem:    # the split image [x+ | x-], rows [W+ | W- ; W- | W+], then the fold
            xs = torch.cat([x_in.clamp(min=0), x_in.clamp(max=0)], 1)
            rows = torch.cat([torch.cat([wp, wn], 1), torch.cat([wn, wp], 1)], 0)
        else:
            xs, rows = x_in, torch.cat([wp, wn], 0)
        out = xs * torch.nn.grad.conv2d_input(xs.shape, rows, a, stride=(sh, sw), padding=(ph, pw))
        return out[:, :x_in.shape[1]] + out[:, x_in.shape[1]:] if stem else out
    for bi in range(len(plan.blocks) - 1, -1, -1):
        blk = plan.blocks[bi]
        x_in = sel(tr["outs"][bi - 1] if bi > 0 else tr["pooled"])
        c1, c2 = tr["coef"][bi]
        r1, r2 = r * sel(c1), r * sel(c2)
        rb = convT(blk["conv2"], convT(blk["conv3"], r1, sel(tr["act"][blk["conv2"]])), sel(tr["act"][blk["conv1"]]))
        if blk["downsample"] is not None:
            r2 = convT(blk["downsample"], r2, x_in)
        r = convT(blk["conv1"], rb, x_in) + r2
    a0 = sel(tr["act"][0])
    s = r / _safe(sel(tr["pooled"]))
    grad = torch.zeros_like(a0).flatten(2).scatter_add_(2, sel(tr["pool_idx"]).flatten(2), s.flatten(2)).view(a0.shape)
    return convT(0, a0 * grad, sel(tr["x"]), stem=True)


def fit(c):
    """(worst six-product error / bound, least witness margin) of a case over its two runs (with and without the addend)"""
    from conftest import rel_err
    from fp64_anchor import C, FLOOR, SIX, THREE
    worst, least = 0., float("inf")
    for addend in (True, False):
        ref64 = reference(c, torch.float64, addend=addend)
        bound = C * max(rel_err(reference(c, torch.float32, addend=addend), ref64), FLOOR)
        worst = max(worst, rel_err(reference(c, torch.float64, SIX, addend=addend), ref64) / bound)
        least = min(least, rel_err(reference(c, torch.float64, THREE, addend=addend), ref64) / bound)
    return worst, least


if __name__ == "__main__":      # prints the REDRAW table: per case the first draw that is fit (margin kept clear of the limit: 2.5)
    table = {}
    for spec in EDGE_CASES + PROD_CASES:
        for draw in range(64):
            REDRAW[spec[0]] = draw
            _CACHE.pop(spec[0], None)
            worst, least = fit(case(spec[0]))
            if worst <= 1 and least >= 2.5:
                break
        else:
            raise SystemExit("no fit draw for " + spec[0])
        if draw:
            table[spec[0]] = draw
    print("REDRAW =", table)
