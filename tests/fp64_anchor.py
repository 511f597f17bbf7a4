"""The fp32-grade criterion of the exact arithmetic (conv mode 1) and of the fp32 MFMA mode (conv mode 0), anchored in fp64.

Mode 1 splits every fp32 operand exactly into three bf16 planes (x == p0 + p1 + p2, each plane the round-to-nearest-even bf16
of the remainder: csrc/conv_bf16x6.h, split3) and keeps the six plane products whose plane indices sum to <= 2, accumulated in
fp32.  The dropped products are 2^-24 of a term and below: the arithmetic is at least as fine as fp32's.  A kernel that keeps
fewer products - three (hi.hi, hi.mid, mid.hi) is 16-bit-grade arithmetic - still passes a 1e-4 bound with a wide margin,
so the bound here is relative to what plain fp32 itself reaches on the SAME operation and inputs:

    e   = rel_err(got,   ref64)      the kernel against an fp64 evaluation of the operation it implements
    e32 = rel_err(ref32, ref64)      a plain fp32 torch CPU evaluation of that same operation on the same fp32 inputs
    e  <= C * max(e32, FLOOR)

and every use of the bound shows that it has teeth: an fp64 emulation of the three-product arithmetic on the same inputs
(`witness`) must miss it by at least WITNESS_MARGIN.  No flat allowance, no quota of points above the bound."""
import torch

from conftest import rel_err

# C: from the first MI355X run of tests/test_gpu_fp64_anchor.py (printed per layer / per map).  Worst e / max(e32, FLOOR) of the
# relevance kernels: 4.46 (b6_28_rel, conv4_1) per layer, 5.85 (mode 1, a 320-map chain) end to end; the per-layer three-product
# witnesses sit >= 12.5x above fp32 there, so C may not exceed 6.25 - 6 is both above every observation and below that.
C = 6.0
# the forward: activations are non-negative, so the error of dropped plane products averages out over K instead of adding up -
# a three-product forward is only 2.1x fp32's error at conv5_1's Z+ - and the fp32 MFMA forward (mode 0, one fmaf chain over up to
# 4608 terms per K range) reached 12.8x the blocked CPU sum's error at conv5_3 (mode 1: 6.6x): twice that, no witness margin
C_FORWARD = 26.0
FLOOR = 1e-7                   # fp32's half-ulp is 6e-8: below this nothing is distinguishable from fp32 rounding of the output
WITNESS_MARGIN = 2.0

SIX = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))      # what conv mode 1 keeps
THREE = ((0, 0), (0, 1), (1, 0))                            # 16-bit-grade arithmetic: the regression the bound must catch


def bf16_split3(x):
    """fp32 tensor -> three fp32 tensors holding bf16 values, x == p0 + p1 + p2 exactly (the kernels' split3)"""
    x = torch.as_tensor(x).float()
    p0 = x.bfloat16().float()
    r1 = x - p0                                # exact: x and p0 agree in their top 8 significand bits
    p1 = r1.bfloat16().float()
    p2 = (r1 - p1).bfloat16().float()          # at most 8 bits are left: exact
    return p0, p1, p2


def emulate(op, a, b, pairs):
    """fp64 value of the bilinear `op(a, b)` (a conv, transposed conv or matrix product) evaluated from the plane products
    `pairs` of the exact bf16 splits of the fp32 operands a and b: sum over (i, j) in pairs of op(a_i, b_j), in fp64
    (the products of bf16 planes are exact in the kernels; fp64 keeps their sum exact enough to show what the pairs lose).
    Grouped by the plane of `a`: at most three evaluations of `op`."""
    pa, pb = bf16_split3(a), bf16_split3(b)
    out = None
    for i in range(3):
        js = [j for (ii, j) in pairs if ii == i]
        if not js:
            continue
        bsum = sum(pb[j].double() for j in js)          # sums of bf16 planes: exact in fp64
        t = op(pa[i].double(), bsum)
        out = t if out is None else out + t
    return out


def fp32_grade(got, ref64, ref32, witness, what, c=None, floor=None, margin_min=None):
    """assert that `got` is fp32 grade against `ref64` (see the module docstring) and that the three-product `witness` misses the
    bound by `margin_min` (WITNESS_MARGIN; 0 only reports it); prints one line and returns (e, e32, e / e32, witness margin)"""
    c = C if c is None else c
    floor = FLOOR if floor is None else floor
    margin_min = WITNESS_MARGIN if margin_min is None else margin_min
    ref64 = torch.as_tensor(ref64).double()
    e = rel_err(got, ref64)
    e32 = rel_err(ref32, ref64)
    bound = c * max(e32, floor)
    ew = rel_err(witness, ref64)
    margin = ew / bound
    ratio = e / max(e32, 1e-300)
    print(f"fp64 anchor {what}: e {e:.2e}  e32 {e32:.2e}  e/e32 {ratio:.2f}  bound {bound:.2e}  "
          f"three-product witness {ew:.2e} = {margin:.1f}x the bound")
    assert e <= bound, f"{what}: not fp32 grade: rel_err vs fp64 {e:.3e} > {c} x max(fp32's {e32:.3e}, {floor:.0e})"
    assert margin >= margin_min, (f"{what}: the bound cannot tell 16-bit-grade arithmetic apart here (witness {ew:.3e} is "
                                      f"only {margin:.2f}x the bound {bound:.3e}): use heavier-tailed data")
    return e, e32, ratio, margin


# ---- the operations of the VGG16 relevance chain, in any precision ----------------------------------------------------------

def convT(s, w):
    return torch.nn.functional.conv_transpose2d(s, w, padding=1)


def rel_mul(x, s, w, pairs=None):
    """the REL_MUL layer of the relevance chain: x * convT(s, w) for non-negative x, s = R / safe(Z+), w = W+ (times the layer's
    power-of-two channel scales, which commute with everything here).  pairs=None: plain evaluation in the dtype of the inputs;
    otherwise fp64 from the given plane products of s and w (x multiplies in fp64)."""
    if pairs is None:
        return x * convT(s, w)
    return x.double() * emulate(convT, s, w, pairs)


def safe_div(r, z):
    """LRPtools/utils.py:16-18: only exact zeros are stabilised"""
    return r / (z + 1e-7 * (z == 0).to(z.dtype))


def conv_rule(x, w, r, dtype, pairs=None):
    """alpha1beta0 rule of one conv layer (oracle.conv_alpha1beta0) with x, w cast to `dtype`; pairs: the transposed convs
    from those plane products of (S in fp32, W in fp32) - S is formed in fp64 then rounded to fp32, as the kernel receives it"""
    x, w, r = x.to(dtype), w.to(dtype), r.to(dtype)
    wp, wn = w.clamp(min=0), w.clamp(max=0)
    xp, xn = x.clamp(min=0), x.clamp(max=0)
    F = torch.nn.functional
    z = F.conv2d(xp, wp, padding=1)
    if (xn != 0).any():
        z = z + F.conv2d(xn, wn, padding=1)
    s = safe_div(r, z)
    if pairs is None:
        out = xp * convT(s, wp)
        if (xn != 0).any():
            out = out + xn * convT(s, wn)
        return out
    s32 = s.float()
    out = xp.double() * emulate(convT, s32, wp.float(), pairs)
    if (xn != 0).any():
        out = out + xn.double() * emulate(convT, s32, wn.float(), pairs)
    return out


def maxpool_rule(x, r):
    """oracle.maxpool_rule: winner-take-all (first maximum) of every 2x2 window"""
    F = torch.nn.functional
    z, idx = F.max_pool2d(x, 2, 2, return_indices=True)
    s = safe_div(r, z)
    if idx.shape[0] != s.shape[0]:
        idx = idx.expand(s.shape[0], -1, -1, -1)
    return x * F.max_unpool2d(s, idx, 2, 2, output_size=x.shape[-2:])


def vgg_chain(layers, weights, saved, r_feat, dtype, pairs_at=None):
    """the 13-layer relevance chain (oracle.vgg_lrp) in `dtype`; pairs_at: {layer index: pairs} evaluates those conv layers from
    plane products (fp64), the others plainly.  `layers` = oracle.vgg_layers(), `weights[l]` the conv weight of layer l,
    `saved[l]` the (fp32) input of layer l for ONE image (the pool winners are those of `saved`, in every precision)."""
    r = r_feat.to(dtype)
    pairs_at = pairs_at or {}
    for l in range(len(layers) - 1, -1, -1):
        x = saved[l]
        if layers[l][0] == "conv":
            pairs = pairs_at.get(l)
            r = conv_rule(x, weights[l], r, torch.float64 if pairs else dtype, pairs).to(dtype)
        else:
            r = maxpool_rule(x.to(dtype), r)
    return r
