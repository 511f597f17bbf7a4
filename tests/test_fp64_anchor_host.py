"""Host tests of the fp32-grade criterion (tests/fp64_anchor.py): on one production layer and on one whole chain map, with the
oracle's VGG16 weights and activations, a plain fp32 evaluation passes it, the three-product (16-bit-grade) emulation fails it by
the witness margin, and the six-product emulation of conv mode 1 sits within FLOOR of fp64.  No GPU: what the GPU tests of
tests/test_gpu_fp64_anchor.py hold the kernels to, shown to tell the two arithmetics apart."""
import pytest
import torch

import fp64_anchor as A
from conftest import rel_err


@pytest.fixture(scope="module")
def vgg_case():
    import lrp_amd  # noqa: F401
    from lrp_amd import weights
    from oracle import lrp_oracle as O
    sdt = O.state_to_torch(weights.make_gridtd_state(seed=5, vocab_size=32))
    img = torch.from_numpy(weights.make_images(7, 1))
    with torch.no_grad():
        feats, _, saved = O.vgg_forward(sdt, img)
    layers = O.vgg_layers()
    ws = {l: sdt[f"img_encoder.encoder.{idx}.weight"] for l, (kind, idx, _, _) in enumerate(layers) if kind == "conv"}
    return layers, ws, saved, feats


def heavy(shape, seed, spread=4.0):
    """signed heavy-tailed relevance, randn * exp(spread * randn)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * torch.exp(spread * torch.randn(*shape, generator=g))


def test_criterion_on_conv4_2_relevance(vgg_case):
    """conv4_2's REL_MUL layer (28 x 28, 512 -> 512), 2 maps: out = X * convT(S, W+) on the layer's own X and S = R / safe(Z+).
    The fp32 stand-in for a kernel sums the two K halves separately (the order a K-split kernel uses)."""
    layers, ws, saved, _ = vgg_case
    l = 11
    assert layers[l][0] == "conv" and saved[l].shape[1:] == (512, 28, 28)
    x, wp = saved[l], ws[l].clamp(min=0)
    z = torch.nn.functional.conv2d(x, wp, padding=1)
    s = A.safe_div(heavy((2, 512, 28, 28), 11), z).float()
    with torch.no_grad():
        for i in range(2):
            si = s[i:i + 1]
            ref64 = A.rel_mul(x.double(), si.double(), wp.double())
            ref32 = A.rel_mul(x, si, wp)
            stand_in = x * (A.convT(si[:, :256], wp[:256]) + A.convT(si[:, 256:], wp[256:]))
            three = A.rel_mul(x, si, wp, A.THREE)
            six = A.rel_mul(x, si, wp, A.SIX)
            A.fp32_grade(stand_in, ref64, ref32, three, f"host conv4_2 map {i}: fp32 K-split stand-in")
            assert rel_err(six, ref64) <= A.FLOOR, rel_err(six, ref64)
            with pytest.raises(AssertionError, match="not fp32 grade"):
                A.fp32_grade(three, ref64, ref32, three, f"host conv4_2 map {i}: three products as the kernel")


def test_criterion_on_a_whole_chain_map(vgg_case):
    """one map through all 13 layers: the fp32 chain passes, the three-product chain fails, the six-product chain is fp64"""
    layers, ws, saved, feats = vgg_case
    r = heavy(feats.shape, 5) * (feats > 0)
    all3 = {l: A.THREE for l in ws}
    with torch.no_grad():
        ref64 = A.vgg_chain(layers, ws, saved, r, torch.float64)
        ref32 = A.vgg_chain(layers, ws, saved, r, torch.float32)
        three = A.vgg_chain(layers, ws, saved, r, torch.float64, all3)
        six = A.vgg_chain(layers, ws, saved, r, torch.float64, {l: A.SIX for l in ws})
    # the stand-in: fp32 again, but every relevance conv summed as its two K halves
    stand_in = _k_split_chain(layers, ws, saved, r)
    A.fp32_grade(stand_in, ref64, ref32, three, "host chain: fp32 K-split stand-in")
    assert rel_err(six, ref64) <= A.FLOOR, rel_err(six, ref64)
    with pytest.raises(AssertionError, match="not fp32 grade"):
        A.fp32_grade(three, ref64, ref32, three, "host chain: three products as the kernel")


def _k_split_chain(layers, ws, saved, r):
    F = torch.nn.functional
    with torch.no_grad():
        for l in range(len(layers) - 1, -1, -1):
            x = saved[l]
            if layers[l][0] == "conv":
                w = ws[l]
                wp, wn = w.clamp(min=0), w.clamp(max=0)
                xp, xn = x.clamp(min=0), x.clamp(max=0)
                s = A.safe_div(r, F.conv2d(xp, wp, padding=1) + F.conv2d(xn, wn, padding=1))
                h = s.shape[1] // 2

                def ct(wv):
                    return A.convT(s[:, :h], wv[:h]) + A.convT(s[:, h:], wv[h:])
                r = xp * ct(wp) + (xn * ct(wn) if l == 0 else 0)
            else:
                r = A.maxpool_rule(x, r)
    return r
