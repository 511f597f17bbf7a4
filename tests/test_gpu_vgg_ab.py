"""The alpha-beta rule on the exact splits through VGG16 and the caption engines: `conv_geom_ab(pool=2)` in both
arithmetics on the cases of tests/vgg_ab_cases.py, `lrpx_vgg16_ab_coef` against torch, `Vgg16.relevance_alpha_beta(conv_mode=1)`
against an fp64 walk on the trace's own activations, and the `lrp_params` switch of GridTDEngine / AOAEngine / AdaAttEngine."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lrp_amd  # noqa: F401
import vgg_ab_cases as V
from conftest import GOLDEN, rel_err
from fp64_anchor import THREE, fp32_grade

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden_resnet import bottleneck_net  # noqa: E402

GUARD = 4096
SENTINEL = 12345.0
GEOM3 = (3, 3, 1, 1, 1, 1)


def _mods():
    from lrp_amd import _lib, ops
    return _lib, ops


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def to_nhwc(t):
    """CPU NCHW -> device (n, H W, c)"""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).contiguous().cuda()


def to_nchw(t, h, w):
    return t.view(t.shape[0], h, w, -1).permute(0, 3, 1, 2).cpu()


def safe(z):
    return z + 1e-7 * (z == 0).to(z.dtype)


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """an output of `shape` embedded in a larger allocation filled with a sentinel"""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
        self.view = self.buf[GUARD:GUARD + n].view(*shape)

    def check(self, what):
        torch.cuda.synchronize()
        assert (self.buf[:GUARD] == SENTINEL).all(), what + ": wrote before its output"
        assert (self.buf[-GUARD:] == SENTINEL).all(), what + ": wrote past its output"
        assert (self.view != SENTINEL).all(), what + ": left part of its output unwritten"
        assert torch.isfinite(self.view).all(), what + ": read beyond an operand (NaN surroundings)"


def in_nans(t):
    """the tensor on the device inside a NaN-filled allocation: a read beyond it poisons the result and is no fault"""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), device="cuda")
    view = buf[GUARD:GUARD + t.numel()].view(*t.shape)
    view.copy_(t)
    return view


def _run_case(c, b6, addend, beta, guarded):
    """the case on the device: (result NCHW on the CPU, fp64, fp32, three-product witness)"""
    _lib, ops = _mods()
    wrap = in_nans if guarded else (lambda t: t)
    dev = V.cached(c, "dev", lambda: {k: to_nhwc(c[k]) for k in ("r", "xs", "qp", "qn", "addend")})
    pack = ops.conv_geom_pack_bf16x3 if b6 else ops.conv_geom_pack
    h, w = c["hw"]
    n_maps, n_img, dual = c["r"].shape[0], c["xs"].shape[0], beta != 0.
    rows = c["rows"] if dual else c["rows"][:c["kr"]]
    out = Guarded(n_maps, h * w, c["n_oc"]) if guarded else None
    got = ops.conv_geom_ab(wrap(dev["r"]), pack(rows.cuda(), _lib.GEOM_BWD), n_maps, c["hw"], c["hw"], GEOM3, c["kr"], c["n_oc"],
                           wrap(dev["xs"]), wrap(dev["qp"]), q2=wrap(dev["qn"]) if dual else None, scale=V.ALPHA,
                           scale2=-beta if dual else 0., addend=wrap(dev["addend"]) if addend else None, map2img=_i32(c["map2img"]),
                           n_img=n_img, out=out.view if guarded else None, b6=b6, pool=2)
    what = f"conv_geom_ab(pool=2) b6={b6} {c['name']} addend={addend} beta={beta}"
    if guarded:
        out.check(what)
    torch.cuda.synchronize()
    kw = dict(addend=addend, beta=beta)
    refs = [V.cached(c, (name, addend, beta), fn) for name, fn in (
        ("ref64", lambda: V.reference(c, torch.float64, **kw)), ("ref32", lambda: V.reference(c, torch.float32, **kw)),
        ("three", lambda: V.reference(c, torch.float64, THREE, **kw)))]
    return [to_nchw(got, h, w), what] + refs


@pytest.mark.parametrize("b6", [False, True], ids=["fp32", "b6"])
@pytest.mark.parametrize("group", ["c10x6", "c11x9", "first10x6", "first11x9"])
def test_kernel_cases(group, b6):
    """kr in {4, 20, 36, 52} x n_oc in {4, 36, 68} (first-layer form: 8) at conv outputs 10 x 6 and 11 x 9, three maps on two images
    [1, 0, 1], with and without addend, and beta = 0: the pooled relevance sits inside NaNs (a read beyond the pooled map - row 5 of the
    5 x 4 map at 11 x 9 - poisons the result), nothing is written outside the output.  b6: fp32 grade with the witness margin; the fp32
    MFMA variant: the bound of its parent's test (tests/test_gpu_resnet_ab.py: the same criterion, the witness only reported)."""
    for spec in V.EDGE_CASES:
        if not spec[0].startswith(group + "_"):
            continue
        c = V.case(spec[0])
        for addend, beta in V.RUNS:           # the runs tests/test_vgg_ab_host.py found fit for the criterion, beta = 0 included
            got, what, ref64, ref32, three = _run_case(c, b6, addend, beta, True)
            fp32_grade(got, ref64, ref32, three, what, margin_min=None if b6 else 0)
        if spec[3] == (11, 9):              # the last row and column of the conv's output lie under no window: their taps add nothing
            assert torch.isfinite(got).all()


@pytest.mark.parametrize("b6", [False, True], ids=["fp32", "b6"])
@pytest.mark.parametrize("name", [c[0] for c in V.PROD_CASES])
def test_kernel_production_shapes(name, b6):
    """conv4_3's shape (512 -> 512 at 28 x 28, r at 14 x 14) and conv1_2's (64 -> 64 at 224 x 224), one map on one image"""
    got, what, ref64, ref32, three = _run_case(V.case(name, 1, 1), b6, False, V.BETA, False)
    fp32_grade(got, ref64, ref32, three, what, margin_min=None if b6 else 0)


def test_pool_descriptor_refusals():
    _lib, ops = _mods()
    import ctypes as C
    c = V.case("c10x6_4_4")
    dev = {k: to_nhwc(c[k]) for k in ("r", "xs", "qp", "qn")}
    pk = ops.conv_geom_pack(c["rows"].cuda(), _lib.GEOM_BWD)
    out = torch.empty(3, 60, 4, device="cuda")
    base = _lib.ConvGeomExDesc(_lib.ptr(dev["r"]), _lib.ptr(pk), None, _lib.ptr(dev["xs"]), _lib.ptr(dev["qp"]), None, _lib.ptr(_i32(c["map2img"])),
                               _lib.ptr(out), _lib.GEOM_BWD, 3, 2, 10, 6, 10, 6, *GEOM3, 8, 4)
    ab = _lib.ConvGeomAbDesc(base, _lib.ptr(dev["qn"]), 2., -1., 4)
    lib = _lib.load()
    for fn in (lib.lrpx_conv_geom_ab_pool, lib.lrpx_conv_geom_ab_pool_b6):
        for pool in (0, 1, 3, 4, -2):
            assert fn(C.byref(_lib.ConvGeomAbPoolDesc(ab, pool)), _lib.stream_ptr()) == _lib.EINVAL
        assert fn(None, _lib.stream_ptr()) == _lib.EINVAL
    with pytest.raises(ValueError, match="input must hold"):          # the size check uses the POOLED pixel count
        ops.conv_geom_ab(torch.zeros(3, 60, 4, device="cuda"), pk, 3, (10, 6), (10, 6), GEOM3, 4, 4, dev["xs"], dev["qp"], q2=dev["qn"],
                         scale2=-1., map2img=_i32(c["map2img"]), n_img=2, pool=2)
    torch.cuda.synchronize()


# ---- 2. the per-image coefficients -----------------------------------------------------------------------------------------------------------
def ulp_report(got, want, what):
    """at most 1 ulp apart, exact zeros and signs identical"""
    assert got.shape == want.shape
    gi, wi = got.contiguous().view(torch.int32).long(), want.contiguous().view(torch.int32).long()
    print(f"{what}: {int((gi != wi).sum())} of {got.numel()} elements differ from torch's fp32 expression")
    assert torch.equal(got == 0, want == 0) and torch.equal(torch.signbit(got), torch.signbit(want))
    assert int((gi - wi).abs().max()) <= 1
    assert torch.isfinite(got).all()


@pytest.mark.parametrize("c", [4, 36])
@pytest.mark.parametrize("hw", [(10, 6), (11, 9)])
def test_vgg16_ab_coef_vs_torch(hw, c):
    _lib, ops = _mods()
    g = torch.Generator().manual_seed(100 * hw[0] + c)
    n, (h, w) = 3, hw
    a = (torch.randn(n, c, h, w, generator=g).clamp(min=0) * 2).round() / 2           # quantised: ties and all-zero windows
    a[0, 0, 0:2, 0:2] = 0.5                                                           # a fully tied window: the first pixel wins
    a[1, 1, 2:4, 2:4] = 0.0                                                           # an all-zero window: no winner
    a[2, 2, 4:6, 0:2] = torch.tensor([[0.5, 1.5], [1.5, 1.0]])                        # a tie between the second and third pixel
    zp, zn = torch.randn(n, c, h, w, generator=g).abs(), -torch.randn(n, c, h, w, generator=g).abs()
    zp[:, 0, 1, :] = 0.0                                                              # exact zeros in Z+ only, Z- only, both
    zn[:, 1, :, 2] = 0.0
    zp[:, 3, 4, 1] = 0.0
    zn[:, 3, 4, 1] = 0.0
    pooled, idx = F.max_pool2d(a, 2, 2, return_indices=True)
    win = torch.zeros_like(a).flatten(2).scatter_(2, idx.flatten(2), (pooled != 0).float().flatten(2)).view(a.shape)
    assert win[0, 0, 0, 0] == 1 and win[0, 0, :2, :2].sum() == 1 and win[1, 1, 2:4, 2:4].sum() == 0 and win[2, 2, 4, 1] == 1 and win[2, 2, 5, 0] == 0
    zz = to_nhwc(torch.cat([zp, zn], 1))
    qp, qn = (torch.full((n, h * w, c), float("nan"), device="cuda") for _ in range(2))
    ops.vgg16_ab_coef(zz, qp, qn, n, hw, c, xpool=to_nhwc(a))
    torch.cuda.synchronize()
    gp, gn = to_nchw(qp, h, w), to_nchw(qn, h, w)
    assert torch.equal(gp != 0, win != 0) and torch.equal(gn != 0, win != 0)          # zeros and winners are F.max_pool2d's
    if h % 2:
        assert gp[:, :, h - 1].abs().sum() == 0 and gp[:, :, :, w - 1].abs().sum() == 0
    ulp_report(gp, torch.where(win != 0, 1 / safe(zp), torch.zeros(())), f"vgg16_ab_coef qp {hw} c {c}")
    ulp_report(gn, torch.where(win != 0, 1 / safe(zn), torch.zeros(())), f"vgg16_ab_coef qn {hw} c {c}")
    ops.vgg16_ab_coef(zz, qp, qn, n, hw, c)                                           # no pool above the conv: win = 1
    torch.cuda.synchronize()
    ulp_report(to_nchw(qp, h, w), 1 / safe(zp), "vgg16_ab_coef qp, no pool")
    ulp_report(to_nchw(qn, h, w), 1 / safe(zn), "vgg16_ab_coef qn, no pool")
    with pytest.raises(ValueError):
        ops.vgg16_ab_coef(zz, qp[:, :, :3].contiguous(), qn, n, hw, c)
    with pytest.raises(ValueError, match="c % 4"):
        ops.vgg16_ab_coef(torch.zeros(n, h * w, 6, device="cuda"), torch.zeros(n, h * w, 3, device="cuda"),
                          torch.zeros(n, h * w, 3, device="cuda"), n, hw, 3)


# ---- 3. the chain ------------------------------------------------------------------------------------------------------------------------------
def nchw(a, hw, dtype):
    """(pix, C) trace rows -> (1, C, hw, hw) on the CPU"""
    return a.to(dtype).cpu().view(hw, hw, -1).permute(2, 0, 1).unsqueeze(0).contiguous()


def pool_rule(x, r):
    """Pool2d rule, first maximum wins: x (1, C, 2h, 2w), r (1, C, h, w)"""
    z, idx = F.max_pool2d(x, 2, 2, return_indices=True)
    return x * F.max_unpool2d(r / safe(z), idx, 2, 2, output_size=x.shape[-2:])


def layered_walk(ctx, weights, r_feat, map2img, alpha, beta, zcache):
    """The rule walked layer by layer in fp64, in the reference's layer order (Pool2d rule, then Conv2d rule), ON THE GPU TRACE'S OWN
    ACTIVATIONS: no pool winner can differ (the approach of tests/test_gpu_alphabeta.py: fp64_walk)"""
    acts, _ = ctx.trace_views()
    w_of = dict(zip([l for l in range(17) if ctx.IS_CONV[l]], weights))
    outs = []
    for m, img in enumerate(map2img):
        r = r_feat[m].double().cpu().view(14, 14, 512).permute(2, 0, 1).unsqueeze(0)
        for l in range(16, -1, -1):
            hw = ctx.ACT_DIMS[l][0]
            x = nchw(acts[l][img], hw, torch.float64)
            if not ctx.IS_CONV[l]:
                r = pool_rule(x, r)
                continue
            w = w_of[l].double()
            wp, wn = w.clamp(min=0), w.clamp(max=0)
            if l == 0:                                      # act[0] = [x+ | x- | 0 0]
                xp, xn = x[:, 0:3], x[:, 3:6]
                if (l, img) not in zcache:
                    zcache[(l, img)] = (F.conv2d(xp, wp, padding=1) + F.conv2d(xn, wn, padding=1), F.conv2d(xp, wn, padding=1) + F.conv2d(xn, wp, padding=1))
                zp, zn = zcache[(l, img)]
                sp, sn = r / safe(zp), r / safe(zn)
                ct = lambda s, k: F.conv_transpose2d(s, k, padding=1)
                r = alpha * (xp * ct(sp, wp) + xn * ct(sp, wn)) - beta * (xp * ct(sn, wn) + xn * ct(sn, wp))
                continue
            if (l, img) not in zcache:
                zcache[(l, img)] = (F.conv2d(x, wp, padding=1), F.conv2d(x, wn, padding=1))
            zp, zn = zcache[(l, img)]
            r = x * (alpha * F.conv_transpose2d(r / safe(zp), wp, padding=1) - beta * F.conv_transpose2d(r / safe(zn), wn, padding=1))
        outs.append(r[0])
    return torch.stack(outs)


def folded_walk(ctx, weights, r_feat, map2img, alpha, beta, qcache):
    """The folded formulation of the chain in plain fp32 on the same activations: per conv qp / qn with the pool's winner factor, the
    relevance read at the pooled resolution, one transposed contraction over the rows [W+ ; W-]"""
    acts, _ = ctx.trace_views()
    w_of = dict(zip([l for l in range(17) if ctx.IS_CONV[l]], weights))
    outs = []
    for m, img in enumerate(map2img):
        r = r_feat[m].float().cpu().view(14, 14, 512).permute(2, 0, 1).unsqueeze(0)
        for l in [l for l in range(16, -1, -1) if ctx.IS_CONV[l]]:
            hw = ctx.ACT_DIMS[l][0]
            x = nchw(acts[l][img], hw, torch.float32)
            w = w_of[l].float()
            wp, wn = w.clamp(min=0), w.clamp(max=0)
            if l == 0:
                z2 = torch.zeros(64, 2, 3, 3)
                rows = torch.cat([torch.cat([wp, wn, z2], 1), torch.cat([wn, wp, z2], 1)], 0)
            else:
                rows = torch.cat([wp, wn], 0)
            pooled = l + 1 < 17 and not ctx.IS_CONV[l + 1]
            if (l, img) not in qcache:
                win = V.winners(nchw(acts[l + 1][img], hw, torch.float32)) if pooled else 1.
                k = rows.shape[0] // 2
                qcache[(l, img)] = (win / safe(F.conv2d(x, rows[:k], padding=1)), win / safe(F.conv2d(x, rows[k:], padding=1)))
            qp, qn = qcache[(l, img)]
            if pooled:
                r = r.repeat_interleave(2, 2).repeat_interleave(2, 3)
            a = torch.cat([(r * qp) * alpha, (r * qn) * (-beta)], 1)
            r = x * F.conv_transpose2d(a, rows, padding=1)
        outs.append(r[0, 0:3] + r[0, 3:6])
    return torch.stack(outs)


@pytest.fixture(scope="module")
def chain():
    """one VGG16 context with a 2-image trace, 3 + 6 sparse signed maps, shared by the chain tests (which never call forward())"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import types
    from lrp_amd import ops, weights
    sd = weights.make_gridtd_state(seed=3, vocab_size=307)
    names = [k for k in sd if k.startswith("img_encoder.encoder.") and k.endswith(".weight")]
    ws = [torch.from_numpy(np.asarray(sd[k])).float() for k in names]
    bs = [torch.from_numpy(np.asarray(sd[k.replace(".weight", ".bias")])).float() for k in names]
    ctx = ops.Vgg16([w.cuda() for w in ws], [b.cuda() for b in bs])
    ctx.forward(torch.from_numpy(weights.make_images(5, 2)).cuda())
    g = torch.Generator().manual_seed(11)
    n = 2 * ctx.AB1_BLOCK + 3
    r_feat = torch.randn(n, 196, 512, generator=g) * (torch.rand(n, 196, 512, generator=g) < 0.3)          # sparse, signed relevance
    m2i = [0, 0, 1] + [int(v) for v in torch.randint(0, 2, (n - 3,), generator=g)]
    torch.cuda.synchronize()
    return types.SimpleNamespace(ctx=ctx, ws=ws, r_feat=r_feat.cuda(), map2img=m2i, m2i=_i32(m2i), z={}, q={})


@pytest.mark.parametrize("alpha,beta", [(2., 1.), (1.5, .5)], ids=["a2_b1", "a1.5_b0.5"])
def test_chain_vs_the_fp64_walk(chain, alpha, beta):
    """2 images, 3 sparse signed maps, conv_mode=1: rel_err < 1e-4 per map against the fp64 walk in the reference's layer order, and
    fp32 grade (C x max(e32, FLOOR)) with e32 the folded formulation in plain fp32 on the same activations.
    MI355X, e / e32 / ratio per map - a2_b1: see DESIGN.md 5.17 (copied from this test's output)."""
    ctx = chain.ctx
    got = ctx.relevance_alpha_beta(chain.r_feat[:3], chain.m2i[:3], alpha, beta, conv_mode=1)
    torch.cuda.synchronize()
    assert got.shape == (3, 3, 224, 224) and torch.isfinite(got).all()
    ref64 = layered_walk(ctx, chain.ws, chain.r_feat[:3], chain.map2img[:3], alpha, beta, chain.z)
    ref32 = folded_walk(ctx, chain.ws, chain.r_feat[:3], chain.map2img[:3], alpha, beta, chain.q)
    for m in range(3):
        e, e32, ratio, _ = fp32_grade(got[m].cpu(), ref64[m], ref32[m], ref32[m], f"relevance_alpha_beta(conv_mode=1) a{alpha} b{beta} map {m}",
                                      margin_min=0)
        print(f"chain a{alpha} b{beta} map {m}: e {e:.3e}  e32 {e32:.3e}  e/e32 {ratio:.2f}")
        assert e < 1e-4


def test_chain_block_independence_linearity_and_modes(chain):
    ctx, r, m2i = chain.ctx, chain.r_feat, chain.m2i
    B = ctx.AB1_BLOCK
    assert r.shape[0] > 2 * B
    all_maps = ctx.relevance_alpha_beta(r, m2i, 2., 1., conv_mode=1).clone()
    # a map computed alone is itself in the batch (first block, a middle block's first map, the last short block)
    for m in (0, 2, B, r.shape[0] - 1):
        assert torch.equal(ctx.relevance_alpha_beta(r[m:m + 1], m2i[m:m + 1], 2., 1., conv_mode=1), all_maps[m:m + 1]), m
    # more maps than one block equal the blocks computed separately - and other cuts than the blocks'
    for step in (B, 5):
        cuts = [(lo, min(lo + step, 2 * B)) for lo in range(0, 2 * B, step)]
        parts = torch.cat([ctx.relevance_alpha_beta(r[lo:hi], m2i[lo:hi], 2., 1., conv_mode=1).clone() for lo, hi in cuts])
        assert torch.equal(parts, all_maps[:2 * B]), step
    # linearity, out(alpha, beta) = alpha out(1, 0) + beta out(0, 1) to the existing linearity test's 1e-5: a statement about ONE conv
    # (through a chain every layer's input depends on both, the map is a polynomial of degree 13 in them), as in
    # tests/test_gpu_alphabeta.py - here conv4_3's shape under its pool, on the exact splits
    c = V.case("conv4_3", 1, 1)
    _lib, ops = _mods()
    dev = {k: to_nhwc(c[k]) for k in ("r", "xs", "qp", "qn")}
    pk = ops.conv_geom_pack_bf16x3(c["rows"].cuda(), _lib.GEOM_BWD)
    run = lambda a, b: ops.conv_geom_ab(dev["r"], pk, 1, (28, 28), (28, 28), GEOM3, 512, 512, dev["xs"], dev["qp"], q2=dev["qn"], scale=a,
                                        scale2=-b, n_img=1, b6=True, pool=2).double()
    e = rel_err((2. * run(1., 0.) + 1. * run(0., 1.)).cpu(), run(2., 1.).cpu())
    print(f"out(2,1) vs 2 out(1,0) + out(0,1) at conv4_3 under its pool: {e:.2e}")
    assert e < 1e-5
    # beta = 0 contracts over W+ alone and is the dual contraction with scale2 = 0 to rounding; conv_mode=0 stays today's path
    b0 = ctx.relevance_alpha_beta(r[:3], m2i[:3], 1.5, 0., conv_mode=1)
    mode0 = ctx.relevance_alpha_beta(r[:3], m2i[:3], 1.5, 0.)
    torch.cuda.synchronize()
    assert rel_err(b0.cpu(), mode0.cpu().double()) < 1e-4
    assert torch.equal(ctx.relevance_alpha_beta(r[:3], m2i[:3], 2., 1., conv_mode=0), ctx.relevance_alpha_beta(r[:3], m2i[:3], 2., 1.))
    for mode in (2, 3):
        with pytest.raises(ValueError, match="conv_mode"):
            ctx.relevance_alpha_beta(r[:3], m2i[:3], 2., 1., conv_mode=mode)
    with pytest.raises(ValueError, match="finite"):
        ctx.relevance_alpha_beta(r[:3], m2i[:3], float("nan"), 1., conv_mode=1)


def test_chain_launches_and_replica(chain):
    """another (alpha, beta) on the same trace does no forward work: 13 transposed launches, four of them under a pool, and the fold;
    a replica shares the packs and makes its own coefficients and workspace"""
    ctx = chain.ctx
    _lib, ops = _mods()
    before = dict(ops.LAUNCHES)
    ctx.relevance_alpha_beta(chain.r_feat[:1], chain.m2i[:1], 3., 2., conv_mode=1)
    d = {k: v - before.get(k, 0) for k, v in ops.LAUNCHES.items() if v != before.get(k, 0)}
    assert not any(k[0] in ("conv_geom_ex_b6_blocked", "vgg16_ab_coef") for k in d), d          # no forward work
    assert d == {("conv_geom_ab_dual_b6", _lib.GEOM_BWD): 9, ("conv_geom_ab_dual_b6_pool", _lib.GEOM_BWD): 4, ("resnet_stem_fold", None): 1}, d
    rep = ctx.replica()
    assert rep._ab1 is None and rep._ab1_packs is ctx._ab1_packs          # one holder, whoever fills it first
    rep.trace, rep.n_img, rep._trace_serial = ctx.trace, ctx.n_img, 1   # (a trace to run on: the parent's, read-only)
    before = dict(ops.LAUNCHES)
    got = rep.relevance_alpha_beta(chain.r_feat[:1], chain.m2i[:1], 3., 2., conv_mode=1)
    d = {k: v - before.get(k, 0) for k, v in ops.LAUNCHES.items() if v != before.get(k, 0)}
    assert d.get(("conv_geom_ex_b6_blocked", _lib.GEOM_FWD)) == 13 and d.get(("vgg16_ab_coef", None)) == 13, d      # its own coefficients
    assert rep._ab1["bwd"] is ctx._ab1["bwd"] and rep._ab1["qp"][16] is not ctx._ab1["qp"][16] and rep._ab1["ws"] is not ctx._ab1["ws"]
    assert torch.equal(got, ctx.relevance_alpha_beta(chain.r_feat[:1], chain.m2i[:1], 3., 2., conv_mode=1))


@pytest.mark.parametrize("cin,cout,hw", [(64, 64, 12), (512, 64, 7)], ids=["18_stages", "144_stages"])
def test_blocked_forward_vs_fp64_and_the_plain_forward(cin, cout, hw):
    """`lrpx_conv_geom_ex_b6_blocked` alone: Z+ = conv(x, W+) of non-negative x at 2 and 18 flushes of the main accumulator, odd pixel
    counts, against fp64 - fp32 grade under the forward's constant (tests/fp64_anchor.py: C_FORWARD) - and against the plain forward
    on the same inputs: at 144 stages the plain order rounds 1728 times at the sum's full size and the blocked one 18 + 16 times, a
    ratio of 7 in the root of the counts; at least 2 is asserted (at 18 stages, 216 against 2 + 16, the figures are printed only).
    And its refusal of the transposed direction."""
    from fp64_anchor import C_FORWARD, emulate
    _lib, ops = _mods()
    g = torch.Generator().manual_seed(40 + cin)
    n = 2
    w = torch.randn(cout, cin, 3, 3, generator=g).clamp(min=0)
    x = torch.randn(n, cin, hw, hw, generator=g).clamp(min=0) * torch.exp(torch.randn(n, cin, hw, hw, generator=g))
    conv = lambda a, b: F.conv2d(a, b, padding=1)
    pk = ops.conv_geom_pack_bf16x3(w.cuda(), _lib.GEOM_FWD)
    run = lambda **kw: to_nchw(ops.conv_geom_ex(to_nhwc(x), pk, _lib.GEOM_FWD, n, (hw, hw), (hw, hw), GEOM3, cin, cout, b6=True, **kw), hw, hw)
    got, plain = run(blocked=True), run()
    torch.cuda.synchronize()
    ref64, ref32 = conv(x.double(), w.double()), conv(x, w)
    e, e32, _, _ = fp32_grade(got, ref64, ref32, emulate(conv, x, w, THREE), f"conv_geom_ex_b6_blocked {cin}->{cout} at {hw}x{hw}",
                              c=C_FORWARD, margin_min=0)
    ep = rel_err(plain, ref64)
    print(f"blocked {e:.2e}  plain {ep:.2e}  CPU fp32 {e32:.2e}")
    if cin == 512:
        assert e <= ep / 2
    with pytest.raises(ValueError, match="forward"):
        ops.conv_geom_ex(to_nhwc(x), pk, _lib.GEOM_BWD, n, (hw, hw), (hw, hw), GEOM3, cin, cout, x=to_nhwc(x), b6=True, blocked=True)
    with pytest.raises(ValueError, match="forward"):
        ops.conv_geom_ex(to_nhwc(x), pk, _lib.GEOM_FWD, n, (hw, hw), (hw, hw), GEOM3, cin, cout, blocked=True)
    import ctypes as C
    d = _lib.ConvGeomExDesc(_lib.ptr(to_nhwc(x)), _lib.ptr(pk), None, _lib.ptr(to_nhwc(x)), None, None, None, _lib.ptr(torch.empty(n, hw * hw, cout, device="cuda")),
                            _lib.GEOM_BWD, n, n, hw, hw, hw, hw, *GEOM3, cin, cout)
    assert _lib.load().lrpx_conv_geom_ex_b6_blocked(C.byref(d), _lib.stream_ptr()) == _lib.EINVAL
    assert _lib.load().lrpx_conv_geom_ex_b6_blocked(None, _lib.stream_ptr()) == _lib.EINVAL


# ---- 4. the caption engines --------------------------------------------------------------------------------------------------------------------
AB = {"alpha": 2., "beta": 1.}


def _tiny_net():
    from lrp_amd.LRPtools import lrp_modules
    seed = int(np.load(os.path.join(GOLDEN, "gridtd_resnet.npz"))["net_seed"])
    return bottleneck_net(np.random.RandomState(seed), lrp_modules.resAdd, 12, [1, 2, 1]).cuda()


def _build(kind, encoder):
    """(engine, images (2, ...), explain(engine, **kw) -> (maps, r_words, r_feat), explain_features or None)"""
    from lrp_amd import weights
    V_ = 307
    cap = torch.from_numpy(weights.make_captions(5, 2, 3, V_))
    if encoder == "vgg":
        x = torch.from_numpy(weights.make_images(2, 2))
        kw = {}
    else:
        x = torch.from_numpy(np.load(os.path.join(GOLDEN, "resnet_engine.npz"))["x"])[:2]
        kw = dict(encoder=_tiny_net())
    if kind == "gridtd":
        from lrp_amd.explainers.gridtd import GridTDEngine
        sd = weights.make_gridtd_state(seed=3, vocab_size=V_) if encoder == "vgg" else \
            weights.make_gridtd_resnet_state(seed=3, vocab_size=V_, feat_dim=192, num_pixels=12)
        eng = GridTDEngine(sd, **kw)
        run = lambda e, **k: e.explain_batch(x, cap, return_features=True, **k)[:3]
    elif kind == "aoa":
        from lrp_amd.explainers.aoa import AOAEngine, AOAResNetEngine
        if encoder == "vgg":
            eng = AOAEngine(weights.make_aoa_state(seed=3, vocab_size=V_))
        else:
            eng = AOAResNetEngine(weights.make_aoa_state(seed=3, vocab_size=V_, feat_dim=192, with_encoder=False), **kw)
        run = lambda e, **k: e.explain_batch(cap, 3, images=x, return_features=True, **k)[:3]
    else:
        from lrp_amd.explainers.adaatt import AdaAttEngine
        sd = weights.make_adaatt_state(seed=3, vocab_size=V_) if encoder == "vgg" else \
            weights.make_adaatt_state(seed=3, vocab_size=V_, feat_dim=192, num_pixels=12, encoder=None)
        eng = AdaAttEngine(sd, **kw)
        run = lambda e, **k: e.explain_batch(x, cap, return_features=True, **k)[:3]
    return eng, x, cap, run


@pytest.mark.parametrize("encoder", ["vgg", "tiny"])
@pytest.mark.parametrize("kind", ["gridtd", "aoa", "adaatt"])
def test_engines_under_lrp_params(kind, encoder):
    """B = 2, T = 3: with `lrp_params` set the maps are the encoder's `relevance_alpha_beta` fed the returned feature relevance, r_words
    and the feature relevance are the bits of the call without it, `accumulate` gives the running sums (one case with `lens`),
    alpha 1 / beta 0 is None; graph, replay and gradient entries are refused before any device work"""
    from lrp_amd import ops
    eng, x, cap, run = _build(kind, encoder)
    assert eng.lrp_params is None
    maps0, rw0, rf0 = (t.clone() for t in run(eng))
    eng.lrp_params = {"alpha": 1., "beta": 0.}
    maps1, _, _ = run(eng)
    assert torch.equal(maps1, maps0)
    eng.lrp_params = dict(AB)
    maps, rw, rf = (t.clone() for t in run(eng))
    assert torch.equal(rw, rw0) and torch.equal(rf, rf0)
    assert not torch.equal(maps, maps0) and torch.isfinite(maps).all()
    B, T = 2, 3
    row2img = torch.arange(B, device="cuda", dtype=torch.int32).repeat_interleave(T)
    feat = rf.reshape(B * T, *rf.shape[2:]).contiguous()
    kw = dict(conv_mode=1) if encoder == "vgg" else {}
    want = eng.cnn.relevance_alpha_beta(feat, row2img, 2., 1., **kw).clone()
    assert torch.equal(maps.reshape(want.shape), want)
    acc, _, _ = run(eng, accumulate=True, lens=[2, 3])
    shp = want.shape[1:]
    assert torch.equal(acc[1].reshape(3, *shp), ops.cumsum_maps(want[3:].contiguous(), 1, 3))
    assert torch.equal(acc[0, :2].reshape(2, *shp), ops.cumsum_maps(want[:2].contiguous(), 1, 2)) and torch.count_nonzero(acc[0, 2]) == 0
    rep = eng.replica()
    assert rep.lrp_params == AB
    streamed = list(eng.explain_stream([(x, cap)], 3, depth=1) if kind == "aoa" else eng.explain_stream([(x, cap)], depth=1))
    assert torch.equal(streamed[0][0], maps)
    # refusals: before any device work (the arguments would fail anything else)
    args = (None, 3) if kind == "aoa" else (None, None)
    for entry in ("explain_batch_graph", "explain_batch_replay"):
        with pytest.raises(NotImplementedError, match="lrp_params"):
            getattr(eng, entry)(*args, **(dict(images=None) if kind == "aoa" else {}))
    if kind != "adaatt":
        with pytest.raises(NotImplementedError, match="lrp_params"):
            eng.explain_batch_gradient(None, 3, None) if kind == "aoa" else eng.explain_batch_gradient(None, None)
    if kind == "aoa":
        with pytest.raises(ValueError, match="features"):
            eng.explain_batch(cap, 3, features=torch.zeros(2, 12, 192))
    if kind == "adaatt":
        with pytest.raises(ValueError, match="features"):
            eng.explain_features(torch.zeros(2, 12, 192), cap)
    for bad in ({"alpha": 2., "gamma": 1.}, {"alpha": float("nan")}, {"alpha": 2., "ignore_bias": False}):
        eng.lrp_params = bad
        with pytest.raises(ValueError, match="lrp_params"):
            run(eng)
    if encoder == "vgg":
        eng.lrp_params = dict(AB)
        eng.vgg.conv_mode = 0                                      # the context's resolved mode picks the path (and the trace's arithmetic)
        m0, _, rf_m0 = (t.clone() for t in run(eng))
        assert torch.equal(m0.reshape(want.shape), eng.cnn.relevance_alpha_beta(rf_m0.reshape(feat.shape).contiguous(), row2img, 2., 1.))
        for mode in (2, 3):
            eng.vgg.conv_mode = mode
            with pytest.raises(ValueError, match="conv modes 0 and 1"):
                run(eng)
    torch.cuda.synchronize()


def test_bottom_up_engine_refuses_lrp_params():
    from lrp_amd import weights
    from lrp_amd.explainers.gridtd import GridTDBUEngine
    eng = GridTDBUEngine(weights.make_gridtd_bu_state(seed=3, vocab_size=307))
    assert eng.lrp_params is None
    eng.lrp_params = dict(AB)
    with pytest.raises(ValueError, match="no encoder"):
        eng.explain_batch(None, None)


def test_dropin_honours_its_own_lrp_params():
    """ExplainGridTDAttention with `lrp_params` set equals its engine under the same rule; the shared engine's attribute is not written"""
    import types
    from lrp_amd import weights
    from lrp_amd.explainers.gridtd import ExplainGridTDAttention
    V_ = 307
    sd = weights.make_gridtd_state(seed=3, vocab_size=V_)
    word_map = {"w%d" % i: i for i in range(V_ - 4)}
    word_map.update({"<unk>": V_ - 4, "<start>": V_ - 3, "<end>": V_ - 2, "<pad>": V_ - 1})
    args = types.SimpleNamespace(embed_dim=512, hidden_dim=512, encoder='vgg16', weight='', save_path='', dataset='synthetic', height=224, width=224)
    ex = ExplainGridTDAttention(args, word_map, model=sd)
    assert ex.lrp_params is None and ex.engine.lrp_params is None
    img = torch.from_numpy(weights.make_images(2, 1))
    cap = [V_ - 3, 5, 9, 11]
    ex.get_hidden_parameters(img, cap)
    r_feat, _ = ex.explain_caption_wordt(1)
    preset = ex.explain_cnn(r_feat).clone()
    ex._img_grad = None
    ex.lrp_params = dict(AB)
    got = ex.explain_cnn(r_feat).clone()
    assert ex.engine.lrp_params is None and not torch.equal(got, preset)
    eng = ex.engine
    feat, row2img = ex._one_map(r_feat)
    want = eng.vgg.relevance_alpha_beta(feat, row2img, 2., 1., conv_mode=1)
    assert torch.equal(got, want)
    eng.lrp_params = dict(AB)
    maps, _ = eng.explain_batch(img, torch.tensor([cap]))
    eng.lrp_params = None
    assert torch.equal(maps[0, 1:2], got)
    ex.lrp_params = {"alpha": 2., "oops": 1.}
    with pytest.raises(ValueError, match="unknown keys"):
        ex.explain_cnn(r_feat)
