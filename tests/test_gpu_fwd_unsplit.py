"""The UNSPLIT exact-split forward kernels at 56 / 28 / 14 (launch_b6_{56,28,14}_fwd: conv_f16x3.h with B6 and the FWD_DUAL
epilogue), launched directly by descriptor.  The forward trace of conv mode 1 runs these map sizes K-split through the PLAIN
kernels and fwd_dual_finish (tests/test_gpu_fp64_anchor.py::test_forward_trace_is_fp32_grade), so a descriptor is the only way
to these three launchers.

Criterion: the one that test applies to their K-split siblings - fp64_anchor.fp32_grade with C_FORWARD, relative to plain fp32's
own error on the same inputs, witness margin reported only (non-negative sums average the dropped plane products out).

Worst e / max(e32, FLOOR) observed on an MI355X: 11.05 (act of the 14 x 14 case with 512 input channels, e 2.15e-6 against
fp32's 1.94e-7; its Z+ 5.53); 2.9 - 5.0 in the three 64-channel cases.  Bound: C_FORWARD = 26."""
import pytest
import torch
import torch.nn.functional as F

import fp64_anchor as A

pytestmark = pytest.mark.gpu

# (hw, cin, cout, n_img): one launcher per map size, more than one image (3 at 14 x 14: an odd number of 196-pixel maps against
# the tiles' row count), and the longest K loop of the chain (conv5_x: 512 channels = 32 K-chunks x 9 taps in ONE accumulator)
CASES = [(56, 64, 32, 2), (28, 64, 32, 2), (14, 64, 32, 3), (14, 512, 32, 1)]


@pytest.mark.parametrize("hw,cin,cout,n_img", CASES, ids=[f"{c[0]}-{c[1]}x{c[3]}" for c in CASES])
def test_unsplit_b6_forward_is_fp32_grade(hw, cin, cout, n_img):
    """act = relu(conv(x, w) + b) and Z+ = conv(x, w+) of ONE launch (weights stacked [w; relu(w)], oc_split = cout) on
    non-negative input, against an fp64 conv2d of the same fp32 operands"""
    from lrp_amd import _lib, ops
    from test_gpu_vgg import from_nhwc, to_nhwc
    g = torch.Generator().manual_seed(1000 * hw + cin)
    x = F.relu(torch.randn(n_img, cin, hw, hw, generator=g))
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = 0.05 * torch.randn(cout, generator=g)
    wcat = torch.cat([w, F.relu(w)])
    wb = ops.pack_weights_bf16x3(wcat.cuda(), 2 * cout, cin, _lib.PACK_FWD)
    act = torch.full((n_img, hw * hw, cout), float("nan"), device="cuda")
    zpos = torch.full((n_img, hw * hw, cout), float("nan"), device="cuda")
    ops.conv_mfma(to_nhwc(x).cuda(), wb, n_img, hw, cin, 2 * cout, 9, _lib.EPI_FWD_DUAL, oc_split=cout, bias=b.cuda(),
                  out0=act, out1=zpos, bf16x6=1)
    torch.cuda.synchronize()
    got_a, got_z = from_nhwc(act.cpu(), cout, hw, hw), from_nhwc(zpos.cpu(), cout, hw, hw)
    assert torch.isfinite(got_a).all() and torch.isfinite(got_z).all()
    bias = torch.cat([b, torch.zeros(cout)]).view(1, -1, 1, 1)

    def split(y):
        return F.relu(y[:, :cout]), y[:, cout:]
    conv = lambda a, k: F.conv2d(a, k, padding=1)                                    # noqa: E731
    a64, z64 = split(conv(x.double(), wcat.double()) + bias.double())
    a32, z32 = split(conv(x, wcat) + bias)
    a3, z3 = split(A.emulate(conv, x, wcat, A.THREE) + bias.double())
    what = f"unsplit b6 forward {hw}x{hw} {cin}->{cout} x{n_img}"
    A.fp32_grade(got_a, a64, a32, a3, what + " act", c=A.C_FORWARD, margin_min=0)
    A.fp32_grade(got_z, z64, z32, z3, what + " Z+", c=A.C_FORWARD, margin_min=0)
