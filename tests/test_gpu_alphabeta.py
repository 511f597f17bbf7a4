"""GPU parity of the general alpha-beta Conv2d rule (beta != 0, with bias): the rule class, the two elementwise kernels, the
hook API with `lrp_params`, and the batched VGG16 path (ops.Vgg16.relevance_alpha_beta).

Bounds.  rel_err < 1e-4 is the project's parity contract (`rel_err` in conftest.py, the bound of every rule test
in test_gpu_hooks.py); the reference's own fp32 arithmetic stays within 1.6e-6 of fp64 for one layer and 1.1e-6 at the bottom of
the 13-conv chain on shared activations, so the contract leaves a margin of 60x and more and hides no failure.  The elementwise
kernels are held to 1 ulp against the same fp32 expression evaluated by torch on the device (one correctly rounded division and
one multiplication per element on both sides): an elementwise kernel has nothing to hide behind."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import lrp_amd  # noqa: F401
from conftest import GOLDEN, rel_err
from test_alphabeta_host import RULE_CASES, alpha_beta_parts, alpha_beta_rule, case_tag, safe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "alphabeta.npz"))


def rule(conv, x, r_out, params):
    from lrp_amd.LRPtools import lrp_modules
    conv.input = (x,)
    return lrp_modules.Conv2d().propagate_relevance(conv, None, (r_out,), "alpha_beta", params)[0]


def make_conv(w, b, dev):
    conv = nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1, bias=b is not None)
    conv.weight.data = torch.as_tensor(w).float()
    if b is not None:
        conv.bias.data = torch.as_tensor(b).float()
    return conv.to(dev).eval()


# ---- 1. the rule class against the reference's own results ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["signed", "relu"])
@pytest.mark.parametrize("case", RULE_CASES, ids=lambda c: case_tag(*c))
def test_rule_class_vs_reference_fixture(gpu, G, name, case):
    alpha, beta, ignore_bias = case
    conv = make_conv(G[name + "_w"], G[name + "_b"], gpu)
    got = rule(conv, torch.from_numpy(G[name + "_x"]).to(gpu), torch.from_numpy(G[name + "_rout"]).to(gpu),
               {"alpha": alpha, "beta": beta, "ignore_bias": ignore_bias})
    want = G[name + "_rin_" + case_tag(*case)]
    e = rel_err(got.cpu(), want)
    print(f"rule class {name} {case_tag(*case)}: rel_err {e:.2e}")
    assert got.shape == want.shape and e < 1e-4


# ---- 2. production shapes against the fp64 restatement ------------------------------------------------------------------------
SHAPES = [(3, 64, 224, True), (128, 128, 112, False), (256, 256, 56, False), (512, 512, 14, False)]


def production_inputs(cin, cout, hw, signed, seed):
    """two samples; |Z| ~ 1 and |b| ~ 0.1 as in the fixtures.  The 3-channel layer sums only 27 products per Z: over its 6.4 M outputs
    the lower tail of |Z| reaches 0.1, a bias of that size cancels some Z, and the reference's own fp32 arithmetic is then 2.0e-5 off
    fp64 (measured on the CPU; the precondition of the test below refuses such inputs).  There |b| ~ 0.03: 2.8e-7."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, cin, hw, hw, generator=g)
    if not signed:
        x = x.clamp(min=0)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin) ** 0.5)
    b = torch.randn(cout, generator=g) * (0.1 if cin >= 64 else 0.03)
    r = torch.randn(2, cout, hw, hw, generator=g)
    return x, w, b, r


@pytest.mark.parametrize("cin,cout,hw,signed", SHAPES, ids=lambda v: str(v))
def test_rule_class_at_production_shapes_vs_fp64(gpu, cin, cout, hw, signed):
    x, w, b, r = production_inputs(cin, cout, hw, signed, 1000 + hw)
    conv = make_conv(w, b, gpu)
    xg, rg = x.to(gpu), r.to(gpu)
    for ignore_bias, ab in ((True, ((2., 1.), (1.5, .5))), (False, ((2., 1.),))):
        bb = None if ignore_bias else b
        p64, n64 = alpha_beta_parts(x, w, bb, r, torch.float64)
        p32, n32 = alpha_beta_parts(x, w, bb, r, torch.float32)
        for alpha, beta in ab:
            want = alpha * p64 - beta * n64
            # a precondition on the INPUTS (it catches a bias that happens to cancel a Z), not an allowance for the GPU
            pre = rel_err(alpha * p32 - beta * n32, want)
            got = rule(conv, xg, rg, {"alpha": alpha, "beta": beta, "ignore_bias": ignore_bias})
            e = rel_err(got.cpu(), want)
            print(f"{cin}->{cout} @ {hw} {case_tag(alpha, beta, ignore_bias)}: fp32 CPU vs fp64 {pre:.2e}, GPU vs fp64 {e:.2e}")
            assert pre < 1e-5
            assert e < 1e-4


# ---- 3. the elementwise kernels alone ------------------------------------------------------------------------------------------
def ulp_report(got, want, what):
    """at most 1 ulp apart, exact zeros and signs identical; prints the number of elements that differ at all"""
    assert got.shape == want.shape
    gi, wi = got.contiguous().view(torch.int32).long(), want.contiguous().view(torch.int32).long()
    differ = int((gi != wi).sum())
    print(f"{what}: {differ} of {got.numel()} elements differ from torch's fp32 expression")
    assert torch.equal(got == 0, want == 0) and torch.equal(torch.signbit(got), torch.signbit(want))
    assert int((gi - wi).abs().max()) <= 1
    assert torch.isfinite(got).all()


def test_divide_alpha_beta_vs_torch(gpu):
    from lrp_amd import ops
    g = torch.Generator().manual_seed(7)
    n_img, pix, c = 4, 37, 24
    map2img = [0, 0, 3, 3, 3, 1, 0]                      # repeated images, image 2 skipped
    r = torch.randn(len(map2img), pix, c, generator=g)
    zp, zn = torch.randn(n_img, pix, c, generator=g).abs(), -torch.randn(n_img, pix, c, generator=g).abs()
    zp[:, 3, :5] = 0.0                                   # exact zeros in Z+ only
    zn[:, 5, 7:9] = 0.0                                  # ... in Z- only
    zp[:, 9, 11] = 0.0; zn[:, 9, 11] = 0.0               # ... in both
    r[2, 4] = 0.0                                        # zero relevance
    r, zp, zn = r.to(gpu), zp.to(gpu), zn.to(gpu)
    m2i = torch.tensor(map2img, dtype=torch.int32, device=gpu)
    for alpha, beta in ((2., 1.), (1.5, .5), (1., 0.), (3., 2.)):
        got = ops.divide_alpha_beta(r, zp, zn, m2i, alpha, beta)
        idx = m2i.long()
        want = torch.cat([alpha * (r / safe(zp[idx])), -beta * (r / safe(zn[idx]))], 2)
        ulp_report(got, want, f"divide_alpha_beta a{alpha} b{beta}")
    got = ops.divide_alpha_beta(r[:4], zp, zn, None, 2., 1.)      # null map2img = identity
    ulp_report(got, torch.cat([2. * (r[:4] / safe(zp)), -1. * (r[:4] / safe(zn))], 2), "divide_alpha_beta identity")
    with pytest.raises(ValueError):
        ops.divide_alpha_beta(r[:, :, :3].contiguous(), zp[:, :, :3].contiguous(), zn[:, :, :3].contiguous(), m2i, 2., 1.)
    with pytest.raises(ValueError, match="finite"):
        ops.divide_alpha_beta(r, zp, zn, m2i, float("nan"), 1.)


def pool_rule_torch(x, r_out, idx):
    """Pool2d rule on NHWC tensors, first maximum wins: x (n_img,2h,2w,c), r_out (n_maps,h,w,c) -> (n_maps,2h,2w,c)"""
    n, h2, w2, c = x.shape
    h, w = h2 // 2, w2 // 2
    xw = x.view(n, h, 2, w, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h, w, 4, c)
    m, am = xw[..., 0, :].clone(), torch.zeros(n, h, w, c, dtype=torch.long, device=x.device)
    for k in range(1, 4):
        up = xw[..., k, :] > m
        m, am = torch.where(up, xw[..., k, :], m), torch.where(up, torch.full_like(am, k), am)
    m, am = m[idx], am[idx]
    v = m * (r_out / safe(m))
    ri = torch.stack([torch.where(am == k, v, torch.zeros_like(v)) for k in range(4)], 3)       # (n_maps,h,w,4,c)
    nm = r_out.shape[0]
    return ri.view(nm, h, w, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(nm, h2, w2, c)


def test_maxpool_relevance_ab_vs_torch(gpu):
    from lrp_amd import ops
    g = torch.Generator().manual_seed(8)
    n_img, h, w, c = 3, 5, 6, 16
    map2img = [2, 0, 0, 2, 2]                            # image 1 skipped
    x = torch.randn(n_img, 2 * h, 2 * w, c, generator=g).clamp(min=0)
    x[0, 0:2, 0:2, 0] = 0.7                              # a tied window: the first pixel wins
    x[0, 2:4, 2:4, 1] = 0.0                              # an all-zero window
    x[2, 4:6, 0:2, 3] = torch.tensor([[0.1, 0.9], [0.9, 0.3]])      # a tie between the second and third pixel
    r_out = torch.randn(len(map2img), h, w, c, generator=g)
    zp, zn = torch.randn(n_img, 2 * h, 2 * w, c, generator=g).abs(), -torch.randn(n_img, 2 * h, 2 * w, c, generator=g).abs()
    zp[:, 0, :, 2] = 0.0
    zn[:, :, 1, 3] = 0.0
    zp[:, 4, 1, 3] = 0.0                                 # both zero at the winner of the second tie
    x, r_out, zp, zn = x.to(gpu), r_out.to(gpu), zp.to(gpu), zn.to(gpu)
    m2i = torch.tensor(map2img, dtype=torch.int32, device=gpu)
    idx = m2i.long()
    ri = pool_rule_torch(x, r_out, idx)
    assert ri[1, 0, 0, 0] != 0 and ri[1, 0, 1, 0] == 0 and ri[0, 5, 0, 3] == 0 and ri[0, 4, 1, 3] != 0      # (map 1 on image 0, map 0 on image 2)
    flat = lambda t: t.reshape(t.shape[0], -1, t.shape[-1]).contiguous()
    for alpha, beta in ((2., 1.), (1.5, .5), (3., 0.)):
        got = ops.maxpool2x2_relevance_ab(flat(x), flat(r_out), flat(zp), flat(zn), m2i, len(map2img), h, w, c, alpha, beta)
        want = torch.cat([alpha * (ri / safe(zp[idx])), -beta * (ri / safe(zn[idx]))], 3)
        ulp_report(got, flat(want), f"maxpool2x2_relevance_ab a{alpha} b{beta}")
    # the unfused pair gives the same bits: Pool2d rule, then the double division
    r_in, _ = ops.maxpool2x2_relevance(flat(x), flat(r_out), None, m2i, len(map2img), h, w, c)
    assert torch.equal(ops.divide_alpha_beta(r_in, flat(zp), flat(zn), m2i, 2., 1.),
                       ops.maxpool2x2_relevance_ab(flat(x), flat(r_out), flat(zp), flat(zn), m2i, len(map2img), h, w, c, 2., 1.))


# ---- 4. default parameters are untouched --------------------------------------------------------------------------------------
def test_default_parameters_take_the_old_path(gpu):
    L = np.load(os.path.join(GOLDEN, "layers.npz"))
    conv = make_conv(L["conv_w"], None, gpu)
    x, r = torch.from_numpy(L["conv_x"]).to(gpu), torch.from_numpy(L["conv_rout"]).to(gpu)
    outs = [rule(conv, x, r, p) for p in ({"alpha": 1., "beta": 0., "ignore_bias": True}, {}, None)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert rel_err(outs[0].cpu(), L["conv_rin"]) < 1e-4
    assert "_lrpx_pack" in conv.__dict__ and "_lrpx_pack_pn" not in conv.__dict__


def torch_vgg(sd, dev):
    from lrp_amd.LRPtools.lrp_wrapper import VGG16_FEATURES
    mods, cin, idx = [], 3, 0
    for v in VGG16_FEATURES:
        if v == 'M':
            mods.append(nn.MaxPool2d(2, 2)); idx += 1
        else:
            c = nn.Conv2d(cin, v, 3, padding=1)
            c.weight.data = torch.from_numpy(sd[f"img_encoder.encoder.{idx}.weight"])
            c.bias.data = torch.from_numpy(sd[f"img_encoder.encoder.{idx}.bias"])
            mods += [c, nn.ReLU(inplace=True)]; idx += 2; cin = v
    return nn.Sequential(*mods).to(dev).eval()


@pytest.fixture(scope="module")
def vgg(gpu):
    from lrp_amd import weights
    sd = weights.make_gridtd_state(seed=3, vocab_size=307)
    return torch_vgg(sd, gpu)


def test_add_lrp_on_vgg_keeps_the_fused_context_for_the_preset(gpu, vgg):
    from lrp_amd.LRPtools import lrp_wrapper
    lrp_wrapper.add_lrp(vgg)
    assert vgg._lrpx_ctx is not None and vgg._lrpx_params == {"alpha": 1., "beta": 0., "ignore_bias": True}
    lrp_wrapper.add_lrp(vgg, lrp_params={"alpha": 1., "beta": 0.})
    assert vgg._lrpx_ctx is not None
    lrp_wrapper.add_lrp(vgg, lrp_params={"ignore_bias": False})        # the generic leaf driver
    assert vgg._lrpx_ctx is None
    lrp_wrapper.add_lrp(vgg)
    assert vgg._lrpx_ctx is not None and "_lrpx_hooks" not in vgg.__dict__


# ---- 5. linearity and conservation ---------------------------------------------------------------------------------------------
def test_linearity_in_alpha_beta(gpu):
    x, w, b, r = production_inputs(256, 256, 56, False, 31)
    conv = make_conv(w, None, gpu)
    xg, rg = x.to(gpu), r.to(gpu)
    r21, r10, r11 = (rule(conv, xg, rg, {"alpha": a, "beta": bt}).double() for a, bt in ((2., 1.), (1., 0.), (1., 1.)))
    e = rel_err(r10 + r11, r21)
    print(f"R(2,1) vs R(1,0) + R(1,1): {e:.2e}")
    assert e < 1e-5


@pytest.mark.parametrize("alpha,beta", [(2., 1.), (1.5, .5), (3., 1.)])
def test_conservation(gpu, alpha, beta):
    """sum R_in = (alpha - beta) sum R on a signed random input without bias (all Z+ / Z- non-zero there)"""
    x, w, b, r = production_inputs(64, 64, 56, True, 32)
    conv = make_conv(w, None, gpu)
    got = rule(conv, x.to(gpu), r.to(gpu), {"alpha": alpha, "beta": beta}).double()
    want = (alpha - beta) * r.double().sum().item()
    print(f"conservation a{alpha} b{beta}: sum R_in {got.sum().item():.6f}, (alpha - beta) sum R {want:.6f}")
    assert abs(got.sum().item() - want) < 1e-4 * got.abs().sum().item()


# ---- 6. the hook API with lrp_params --------------------------------------------------------------------------------------------
def test_add_lrp_with_lrp_params_on_the_fixture_nets(gpu, G):
    from lrp_amd.LRPtools import lrp_wrapper, lrp_modules
    sys.path.insert(0, GOLDEN)
    from make_golden import toy_resnet
    from make_golden_alphabeta import mini_net
    net = mini_net(np.random.RandomState(int(G["mini_seed"]))).to(gpu)
    x, target = torch.from_numpy(G["mini_x"]).to(gpu), torch.from_numpy(G["mini_target"]).to(gpu)
    lrp_wrapper.add_lrp(net)
    r_default = net.compute_lrp(x.clone(), target=target)
    for ignore_bias in (True, False):
        lrp_wrapper.add_lrp(net, lrp_params={"alpha": 2., "beta": 1., "ignore_bias": ignore_bias})
        r = net.compute_lrp(x.clone(), target=target)
        e = rel_err(r.cpu(), G["mini_r_" + case_tag(2., 1., ignore_bias)])
        print(f"mini-net alpha2beta1 ignore_bias={ignore_bias}: {e:.2e}")
        assert e < 1e-4
    lrp_wrapper.add_lrp(net)
    assert torch.equal(net.compute_lrp(x.clone(), target=target), r_default)

    T = np.load(os.path.join(GOLDEN, "toy_resnet.npz"))
    toy = toy_resnet(np.random.RandomState(int(G["toy_seed"])), lrp_modules.resAdd, lrp_modules.resFlatten).to(gpu)
    lrp_wrapper.add_lrp(toy, lrp_params={"alpha": 2., "beta": 1., "ignore_bias": True})
    xs = torch.from_numpy(G["toy_x"]).to(gpu)
    r1 = toy.compute_lrp(xs, target=torch.from_numpy(G["toy_target"]).to(gpu))
    r2 = toy.compute_lrp(xs, target=torch.from_numpy(G["toy_target2"]).to(gpu))        # carries the .grad running sum
    e1, e2 = rel_err(r1.cpu(), G["toy_r1"]), rel_err(r2.cpu(), G["toy_r2"])
    print(f"toy residual net alpha2beta1: {e1:.2e} (first call), {e2:.2e} (running sum of two calls)")
    assert e1 < 1e-4 and e2 < 1e-4
    # conv2 of the toy net has no bias: with ignore_bias=False the reference's result is the noise of a fresh layer's bias - refused
    with pytest.raises(ValueError, match="without bias"):
        lrp_wrapper.add_lrp(toy, lrp_params={"alpha": 2., "beta": 1., "ignore_bias": False})
    lrp_wrapper.add_lrp(toy)
    r = toy.compute_lrp(torch.from_numpy(T["x"]).to(gpu), target=torch.from_numpy(T["target"]).to(gpu))
    assert rel_err(r.cpu(), T["r1"]) < 1e-4


# ---- 7. the batched VGG16 path --------------------------------------------------------------------------------------------------
def nchw(a, hw):
    """(pix, C) trace rows -> (1, C, hw, hw) fp64 on the CPU"""
    return a.double().cpu().view(hw, hw, -1).permute(2, 0, 1).unsqueeze(0).contiguous()


def fp64_walk(ctx, weights64, r_feat, map2img, alpha, beta):
    """The rule walked layer by layer in fp64 ON THE GPU TRACE'S OWN ACTIVATIONS: no pool winner can differ"""
    acts, _ = ctx.trace_views()
    convs = [l for l in range(17) if ctx.IS_CONV[l]]
    w_of = dict(zip(convs, weights64))
    zcache, outs = {}, []
    for m, img in enumerate(map2img):
        r = r_feat[m].double().cpu().view(14, 14, 512).permute(2, 0, 1).unsqueeze(0)
        for l in range(16, -1, -1):
            hw = ctx.ACT_DIMS[l][0]
            x = nchw(acts[l][img], hw)
            if not ctx.IS_CONV[l]:
                r = pool_rule_torch(x.permute(0, 2, 3, 1).contiguous(), r.permute(0, 2, 3, 1).contiguous(), torch.tensor([0])).permute(0, 3, 1, 2)
                continue
            w = w_of[l]
            if l == 0:
                p, n = alpha_beta_parts(x[:, 0:3] + x[:, 3:6], w, None, r)          # act[0] = [x+ | x- | 0 0]
                r = alpha * p - beta * n
                continue
            wp, wn = w.clamp(min=0), w.clamp(max=0)                                 # x >= 0: Z+ = conv(x,W+), Z- = conv(x,W-)
            if (l, img) not in zcache:
                zcache[(l, img)] = (F.conv2d(x, wp, padding=1), F.conv2d(x, wn, padding=1))
            zp, zn = zcache[(l, img)]
            r = x * (alpha * F.conv_transpose2d(r / safe(zp), wp, padding=1) - beta * F.conv_transpose2d(r / safe(zn), wn, padding=1))
        outs.append(r[0])
    return torch.stack(outs)


def test_vgg16_relevance_alpha_beta(gpu, vgg):
    from lrp_amd import ops, weights
    from lrp_amd.LRPtools import lrp_wrapper
    lrp_wrapper.add_lrp(vgg, lrp_params={"alpha": 2., "beta": 1., "ignore_bias": True})
    ctx = vgg._lrpx_ctx
    assert ctx is not None
    img = torch.from_numpy(weights.make_images(5, 2)).to(gpu)
    g = torch.Generator().manual_seed(11)
    r_feat = torch.randn(9, 196, 512, generator=g).to(gpu)
    r_feat = r_feat * (torch.rand(9, 196, 512, generator=g) < 0.3).to(gpu)           # sparse, signed relevance
    map9 = [0, 0, 1, 0, 1, 1, 0, 1, 0]
    m2i = torch.tensor(map9, dtype=torch.int32, device=gpu)
    ctx.forward(img)
    got = ctx.relevance_alpha_beta(r_feat[:3], m2i[:3], 2., 1.)
    assert got.shape == (3, 3, 224, 224)
    convs = [m for m in vgg if isinstance(m, nn.Conv2d)]
    want = fp64_walk(ctx, [c.weight.detach().double().cpu() for c in convs], r_feat[:3], map9[:3], 2., 1.)
    errs = [rel_err(got[m].cpu(), want[m]) for m in range(3)]
    print("relevance_alpha_beta vs the fp64 walk on the trace's activations, per map:", ["%.2e" % e for e in errs])
    assert max(errs) < 1e-4
    # a map computed alone equals itself inside the batch
    for m in (0, 1):
        assert torch.equal(ctx.relevance_alpha_beta(r_feat[m:m + 1], m2i[m:m + 1], 2., 1.), got[m:m + 1])
    # more maps than one block: the same maps computed block by block
    assert len(map9) > ctx.AB_BLOCK
    all9 = ctx.relevance_alpha_beta(r_feat, m2i, 2., 1.)
    B = ctx.AB_BLOCK
    parts = torch.cat([ctx.relevance_alpha_beta(r_feat[lo:lo + B], m2i[lo:lo + B], 2., 1.) for lo in range(0, 9, B)])
    assert torch.equal(all9, parts) and torch.equal(all9[:3], got)
    # through the hook API: the same tensor, and the .grad running sum on a second call
    target = ops.nhwc_to_nchw(r_feat[[0, 2]].contiguous(), 512, 14, 14)               # map 0 on image 0, map 2 on image 1
    sample = img.clone()
    out1 = vgg.compute_lrp(sample, target=target)
    assert torch.equal(out1, got[[0, 2]])
    out2 = vgg.compute_lrp(sample, target=target)
    assert torch.equal(out2, 2 * out1)
    with pytest.raises(ValueError, match="finite"):
        ctx.relevance_alpha_beta(r_feat[:3], m2i[:3], float("inf"), 1.)
