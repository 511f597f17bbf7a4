"""Host tests of the Winograd F(2x2,3x3) form of the conv-mode-1 relevance convs (csrc/conv_wino_b6.h), emulated in the kernel's
operation order (tests/wino_emulation.py) and held to the fp32-grade criterion of tests/fp64_anchor.py with its C unchanged: every
layer the kernel is built for at its production K and n_oc (one image, one map), the 13-layer chain with those layers emulated,
and the transformed weights U against an fp64 evaluation.  No GPU."""
import pytest
import torch

import fp64_anchor as A
import wino_emulation as W
from test_fp64_anchor_host import heavy, vgg_case  # noqa: F401  (the module-scoped oracle case)

# (name, chain layer, hw, K, n_oc): the relevance convs that are not under a pool, K >= 256
WINO_LAYERS = [("conv3_1", 6, 56, 256, 128), ("conv3_2", 7, 56, 256, 256), ("conv4_1", 10, 28, 512, 256), ("conv4_2", 11, 28, 512, 512),
               ("conv5_1", 14, 14, 512, 512), ("conv5_2", 15, 14, 512, 512), ("conv5_3", 16, 14, 512, 512)]


@pytest.mark.parametrize("layer", WINO_LAYERS, ids=[w[0] for w in WINO_LAYERS])
def test_emulated_layer_is_fp32_grade(vgg_case, layer):
    """(the seed 200 + l is one at which the three-product witness of every layer clears its margin: a property of the data and of
    the references alone, found without the emulation)"""
    name, l, hw, K, n_oc = layer
    layers, ws, saved, _ = vgg_case
    assert layers[l][0] == "conv" and saved[l].shape[1:] == (n_oc, hw, hw) and ws[l].shape[:2] == (K, n_oc)
    x, wp = saved[l], ws[l].clamp(min=0)
    with torch.no_grad():
        z = torch.nn.functional.conv2d(x, wp, padding=1)
        s = A.safe_div(heavy((1, K, hw, hw), 200 + l), z).float()
        got = W.wino_rel_mul(x, s, wp)
        ref64 = A.rel_mul(x.double(), s.double(), wp.double())
        ref32 = A.rel_mul(x, s, wp)
        three = A.rel_mul(x, s, wp, A.THREE)
    A.fp32_grade(got, ref64, ref32, three, f"host Winograd emulation {name}")


def test_emulated_chain_is_fp32_grade(vgg_case):
    """one map through all 13 layers, the seven Winograd layers emulated, the others plain fp32"""
    layers, ws, saved, feats = vgg_case
    r = heavy(feats.shape, 5) * (feats > 0)
    with torch.no_grad():
        ref64 = A.vgg_chain(layers, ws, saved, r, torch.float64)
        ref32 = A.vgg_chain(layers, ws, saved, r, torch.float32)
        three = A.vgg_chain(layers, ws, saved, r, torch.float64, {l: A.THREE for l in ws})
        got = W.chain_with_wino(layers, ws, saved, r, {w[1] for w in WINO_LAYERS})
    A.fp32_grade(got, ref64, ref32, three, "host chain, Winograd layers emulated")


def test_transformed_weights_are_the_rounded_fp64_value(vgg_case):
    """U of conv4_2: the three bf16 planes sum exactly to the fp32 U, and U is within half an ulp of G g G^T evaluated in fp64"""
    _, ws, _, _ = vgg_case
    wp = ws[11].clamp(min=0)
    u = W.wino_u(wp)
    p0, p1, p2 = A.bf16_split3(u)
    assert torch.equal((p0.double() + p1.double()) + p2.double(), u.double())
    g = wp.flip(2, 3).double()
    u64 = torch.einsum("ir,kors,js->ijko", W.G, g, W.G).reshape(16, *wp.shape[:2])
    # half an ulp of u: 2^(exponent - 24); frexp's exponent is one above floor(log2)
    ulp_half = torch.exp2(torch.frexp(u.double())[1].double() - 1 - 24)
    assert ((u.double() - u64).abs() <= ulp_half * (1 + 1e-9)).all()
