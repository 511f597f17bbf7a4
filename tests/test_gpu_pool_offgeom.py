"""The max-pool kernels of the ResNet engine (lrpx_resnet_maxpool_fwd / _rel / _grad, NHWC with map2img) and the NCHW MaxPool2d rule
(lrpx_maxpool_rule) on the GPU at windows no test has run: rectangular kernels and strides, a stride above the kernel (pixels in no
window: exact zeros), a 1 x 1 window with a stride, a 5 x 5 / 2 window (a pixel wins up to nine windows) and padding on one axis only.

Data as in test_maxpool_grad_is_exact (tests/test_gpu_resnet_grad.py): x >= 0 with a plateau of ties and an all-zero region (the first
element of a window wins), g_out in eighths, so sums are exact in any order.  fwd and grad are exact against torch; rel and the NCHW rule
meet `assert_pool_grade` of tests/test_gpu_resnet.py against fp64 (C * FLOOR, and the same set of non-zero positions)."""
import pytest
import torch
import torch.nn.functional as F

import lrp_amd  # noqa: F401
from test_gpu_resnet import assert_pool_grade

pytestmark = pytest.mark.gpu

WINDOWS = [(2, 3, 2, 1, 0, 1), (2, 2, 3, 3, 0, 0), (1, 1, 2, 2, 0, 0), (5, 5, 2, 2, 2, 2), (3, 2, 1, 2, 1, 0)]
IDS = ["k%dx%d_s%dx%d_p%dx%d" % w for w in WINDOWS]
H, W, CH, N_IMG, MAP2IMG = 11, 13, 6, 2, [1, 0, 1]
_CACHE = {}


def _i32(v):
    return torch.tensor([int(a) for a in v], dtype=torch.int32, device="cuda")


def _rows(t_nchw):
    n, c, h, w = t_nchw.shape
    return t_nchw.permute(0, 2, 3, 1).reshape(n, h * w, c).float().contiguous().cuda()


def _nchw(rows, h, w):
    return rows.cpu().view(rows.shape[0], h, w, -1).permute(0, 3, 1, 2)


def data(win):
    """(x per image, g_out in eighths per map, r_out per map, pooled x, winner indices per map), built once per window and shared"""
    if win not in _CACHE:
        kh, kw, sh, sw, ph, pw = win
        oh, ow = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        gen = torch.Generator().manual_seed(780 + WINDOWS.index(win))
        x = torch.rand(N_IMG, CH, H, W, generator=gen) + 0.25
        x[0, :, :5, :6] = 0.0
        x[1, 1, 3:7, 4:9] = 1.75
        x[1, 2, 6, 8] = 2.5       # a peak at an even row and column: it wins all nine 5 x 5 / 2 windows that hold it
        g_out = torch.randint(-40, 41, (len(MAP2IMG), CH, oh, ow), generator=gen).float() / 8
        r_out = torch.randn(len(MAP2IMG), CH, oh, ow, generator=gen)
        y, idx = F.max_pool2d(x, (kh, kw), (sh, sw), (ph, pw), return_indices=True)
        _CACHE[win] = dict(x=x, g_out=g_out, r_out=r_out, y=y, idx=idx[MAP2IMG], ohw=(oh, ow))
    return _CACHE[win]


def scatter(d, values):
    """every window's value to its first maximum, summed per pixel, in the dtype of `values`"""
    return torch.zeros(len(MAP2IMG), CH, H * W, dtype=values.dtype).scatter_add_(2, d["idx"].flatten(2), values.flatten(2)).view(
        len(MAP2IMG), CH, H, W)


def rel_reference(d):
    """the Pool2d rule in fp64: R_in = x * sum over the windows a pixel wins of R_out / safe(z)"""
    x, r = d["x"].double()[MAP2IMG], d["r_out"].double()
    z = d["y"].double()[MAP2IMG]
    return x * scatter(d, r / (z + 1e-7 * (z == 0).double()))


def unreached(win):
    """bool (H, W): pixels that lie in no window"""
    kh, kw, sh, sw, ph, pw = win
    cover = torch.nn.grad.conv2d_input((1, 1, H, W), torch.ones(1, 1, kh, kw), torch.ones((1, 1) + data(win)["ohw"]), stride=(sh, sw),
                                       padding=(ph, pw))[0, 0]
    return cover == 0


@pytest.mark.parametrize("win", WINDOWS, ids=IDS)
def test_maxpool_fwd_is_exact(win):
    from lrp_amd import ops
    d = data(win)
    oh, ow = d["ohw"]
    y = torch.full((N_IMG, oh * ow, CH), float("nan")).cuda()
    ops.resnet_maxpool_fwd(_rows(d["x"]), y, N_IMG, (H, W), (oh, ow), CH, win)
    assert torch.equal(_nchw(y, oh, ow), d["y"])


@pytest.mark.parametrize("win", WINDOWS, ids=IDS)
def test_maxpool_grad_is_exact(win):
    from lrp_amd import ops
    d = data(win)
    got = torch.full((len(MAP2IMG), H * W, CH), float("nan")).cuda()
    ops.resnet_maxpool_grad(_rows(d["x"]), _rows(d["g_out"]), _i32(MAP2IMG), got, len(MAP2IMG), N_IMG, (H, W), d["ohw"], CH, win)
    got = _nchw(got, H, W)
    assert torch.equal(got, scatter(d, d["g_out"]))
    dead = unreached(win)
    assert (dead.sum() > H * W // 2) == (win in (WINDOWS[1], WINDOWS[2])) and not got[:, :, dead].any()      # a stride above the kernel
    if win == WINDOWS[3]:         # the peak collects nine windows
        wins = torch.zeros(N_IMG, CH, H * W).scatter_add_(2, d["idx"][[1, 0]].flatten(2), torch.ones(N_IMG, CH, d["idx"][0, 0].numel()))
        assert wins.max() == 9


@pytest.mark.parametrize("win", WINDOWS, ids=IDS)
def test_maxpool_rel_against_fp64(win):
    from lrp_amd import ops
    d = data(win)
    got = torch.full((len(MAP2IMG), H * W, CH), float("nan")).cuda()
    ops.resnet_maxpool_rel(_rows(d["x"]), _rows(d["r_out"]), _i32(MAP2IMG), got, len(MAP2IMG), N_IMG, (H, W), d["ohw"], CH, win)
    got = _nchw(got, H, W)
    assert torch.isfinite(got).all()
    assert_pool_grade(got, rel_reference(d), "resnet_maxpool_rel %s" % (win,))
    assert not got[:, :, unreached(win)].any()


@pytest.mark.parametrize("win", WINDOWS, ids=IDS)
def test_maxpool_rule_nchw_against_fp64(win):
    from lrp_amd import ops
    d = data(win)
    got = ops.maxpool_rule(d["x"][MAP2IMG].contiguous().cuda(), d["r_out"].cuda(), win[:2], win[2:4], win[4:]).cpu()
    assert torch.isfinite(got).all()
    assert_pool_grade(got, rel_reference(d), "maxpool_rule %s" % (win,))
    assert not got[:, :, unreached(win)].any()
