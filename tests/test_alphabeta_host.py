"""Host side of the general alpha-beta Conv2d rule (beta != 0, with bias; LRPtools/lrp_modules.py:124-150 of the reference):
the formulas restated in torch reproduce the reference's own results (tests/golden/alphabeta.npz, written by
tests/golden/make_golden_alphabeta.py), the C ABI carries the new symbols / constants / version, the new entry points
validate their arguments before any launch, and the parameter plumbing of `add_lrp` raises where it must.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import lrp_amd  # noqa: F401
from lrp_amd import _lib
from conftest import GOLDEN, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE_CASES = [(2., 1., True), (1.5, .5, True), (2., 1., False), (1., 0., False), (3., 0., True)]
NEW_SYMBOLS = ("lrpx_divide_alpha_beta", "lrpx_maxpool2x2_relevance_ab")


def case_tag(alpha, beta, ignore_bias):
    return "a%g_b%g_%s" % (alpha, beta, "nobias" if ignore_bias else "bias")


def safe(z):
    """LRPtools/utils.py:16-18: exact zeros only"""
    return z + 1e-7 * (z == 0).to(z.dtype)


def alpha_beta_parts(x, w, b, r, dtype=torch.float64):
    """(R_pos, R_neg) of the rule restated (3x3 / pad 1 / stride 1), in `dtype`; b = None: ignore_bias.
        Z+ = conv(x+,W+) + conv(x-,W-) (+ b)     Z- = conv(x-,W+) + conv(x+,W-) (+ b)        S+- = R / safe(Z+-)
        R_pos = x+ convT(S+,W+) + x- convT(S+,W-)      R_neg = x- convT(S-,W+) + x+ convT(S-,W-)"""
    x, w, r = (torch.as_tensor(t).to(dtype) for t in (x, w, r))
    xp, xn, wp, wn = x.clamp(min=0), x.clamp(max=0), w.clamp(min=0), w.clamp(max=0)
    conv = lambda a, k: F.conv2d(a, k, padding=1)
    convt = lambda s, k: F.conv_transpose2d(s, k, padding=1)
    zp, zn = conv(xp, wp) + conv(xn, wn), conv(xn, wp) + conv(xp, wn)
    if b is not None:
        bb = torch.as_tensor(b).to(dtype).view(1, -1, 1, 1)
        zp, zn = zp + bb, zn + bb
    sp, sn = r / safe(zp), r / safe(zn)
    r_pos = xp * convt(sp, wp) + xn * convt(sp, wn)
    r_neg = xn * convt(sn, wp) + xp * convt(sn, wn)
    return r_pos, r_neg


def alpha_beta_rule(x, w, b, r, alpha, beta, dtype=torch.float64):
    """R_in = alpha R_pos - beta R_neg  (lrp_modules.py:136-147)"""
    r_pos, r_neg = alpha_beta_parts(x, w, b, r, dtype)
    return alpha * r_pos - beta * r_neg


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "alphabeta.npz"))


@pytest.mark.parametrize("name", ["signed", "relu"])
@pytest.mark.parametrize("case", RULE_CASES, ids=lambda c: case_tag(*c))
def test_restatement_reproduces_the_reference(G, name, case):
    """fp32 restatement vs the reference's Conv2d().propagate_relevance: 1e-5 of max|R| (measured: 0 without bias - the same
    ATen calls in the same order - and 1.6e-6 with: the reference adds b+ and b- in two steps); the fp64 one within 1e-5 too."""
    alpha, beta, ignore_bias = case
    want = G[name + "_rin_" + case_tag(*case)]
    b = None if ignore_bias else G[name + "_b"]
    for dtype in (torch.float32, torch.float64):
        got = alpha_beta_rule(G[name + "_x"], G[name + "_w"], b, G[name + "_rout"], alpha, beta, dtype)
        e = rel_err(got, want)
        print(f"{name} {case_tag(*case)} {dtype}: {e:.2e}")
        assert e < 1e-5


def test_alpha2beta1_is_not_alpha1beta0(G):
    """what the rule class returned before it read lrp_params: off by about half of the map's own maximum on these inputs"""
    for name in ("signed", "relu"):
        a1b0 = alpha_beta_rule(G[name + "_x"], G[name + "_w"], None, G[name + "_rout"], 1., 0.)
        assert rel_err(a1b0, G[name + "_rin_a2_b1_nobias"]) > 0.3


def test_conservation_and_linearity_of_the_restatement():
    """alpha - beta = 1 without bias: sum R_in = sum R where Z+ and Z- are non-zero; R(2,1) = R(1,0) + R(1,1)"""
    rs = np.random.RandomState(3)
    x, w = rs.standard_normal((1, 5, 9, 9)), rs.standard_normal((7, 5, 3, 3)) * 0.3
    r = rs.standard_normal((1, 7, 9, 9))
    r21, r10, r11 = (alpha_beta_rule(x, w, None, r, a, b) for a, b in ((2., 1.), (1., 0.), (1., 1.)))
    assert abs(r21.sum().item() - r.sum()) < 1e-9 * np.abs(r).sum() and abs(r10.sum().item() - r.sum()) < 1e-9 * np.abs(r).sum()
    assert rel_err(r10 + r11, r21) < 1e-12


def header_text():
    src = open(os.path.join(ROOT, "include", "lrpx.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_and_library_exports_the_new_symbols():
    src = header_text()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src), s + " not declared in include/lrpx.h"
        assert hasattr(lib, s), s + " not exported by liblrpx.so"
        assert s in _lib.SIGNATURES


def test_pack_constants_match_the_header():
    enum = dict((k, int(v)) for k, v in re.findall(r"\bLRPX_(PACK_[A-Z_]+)\s*=\s*(\d+)", header_text()))
    old = ["PACK_FWD_DUAL", "PACK_BWD_POS", "PACK_BWD_FIRST", "PACK_BWD_PLAIN", "PACK_DENSE_T", "PACK_DENSE", "PACK_FWD",
           "PACK_FWD_DUAL_FIRST"]
    new = ["PACK_FWD_PN", "PACK_FWD_PN_FIRST", "PACK_BWD_PN", "PACK_BWD_PN_FIRST"]
    assert [enum[k] for k in old] == list(range(8)) and [enum[k] for k in new] == [8, 9, 10, 11]
    for k in old + new:
        assert getattr(_lib, k) == enum[k], k
    assert len(enum) == 12


def test_version_is_101():
    assert _lib.load().lrpx_version() == 101
    assert "101" in open(os.path.join(ROOT, "include", "lrpx.h")).read().split("int lrpx_version")[0][-400:]
    assert "101" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_new_entry_points_validate_on_the_host():
    """null pointers, bad sizes, non-finite factors: EINVAL with a message, before any launch (no device here)"""
    lib = _lib.load()
    assert lib.lrpx_divide_alpha_beta(None, None, None, None, None, 1, 1, 4, 2., 1., None) == _lib.EINVAL
    assert b"null" in lib.lrpx_last_error_string()
    assert lib.lrpx_maxpool2x2_relevance_ab(None, None, None, None, None, None, 1, 1, 1, 4, 2., 1., None) == _lib.EINVAL
    assert b"null" in lib.lrpx_last_error_string()
    # the packers that split the operands keep refusing the new modes
    for fn in ("lrpx_pack_weights_bf16x3", "lrpx_pack_weights_f16x2"):
        assert getattr(lib, fn)(None, 32, 32, 9, _lib.PACK_BWD_PN, None, None) == _lib.EINVAL
    assert lib.lrpx_pack_weights(None, 1, 1, 9, _lib.PACK_BWD_PN_FIRST, 16, None, None) == _lib.EINVAL
    assert b"null" in lib.lrpx_last_error_string()
    assert lib.lrpx_pack_weights(None, 1, 1, 9, 12, 16, None, None) == _lib.EINVAL


def test_add_lrp_merges_lrp_params_over_the_preset():
    from lrp_amd.LRPtools import lrp_wrapper, lrp_modules
    assert lrp_wrapper.merge_lrp_params() == {"alpha": 1., "beta": 0., "ignore_bias": True}
    assert lrp_wrapper.merge_lrp_params({"alpha": 2., "beta": 1.}) == {"alpha": 2., "beta": 1., "ignore_bias": True}
    assert lrp_wrapper.merge_lrp_params({"ignore_bias": False}) == {"alpha": 1., "beta": 0., "ignore_bias": False}
    assert lrp_modules.alpha_beta_params(None) == (1., 0., True) and lrp_modules.alpha_beta_params({}) == (1., 0., True)
    assert lrp_modules.alpha_beta_params({"alpha": 2, "beta": 1, "ignore_bias": 0}) == (2., 1., False)
    for bad in ({"alpha": math.nan}, {"beta": math.inf}, {"alpha": -math.inf, "beta": 1.}):
        with pytest.raises(ValueError, match="finite"):
            lrp_wrapper.merge_lrp_params(bad)
        with pytest.raises(ValueError, match="finite"):
            lrp_modules.Conv2d().propagate_relevance(nn.Conv2d(2, 2, 3, padding=1), None, (torch.zeros(1, 2, 4, 4),), "alpha_beta", bad)
        with pytest.raises(ValueError, match="finite"):
            lrp_wrapper.add_lrp(nn.Sequential(nn.Conv2d(2, 2, 3, padding=1), nn.ReLU()), lrp_params=bad)


def test_ignore_bias_false_on_a_bias_free_conv_is_refused():
    """the reference's clones keep the random bias of a fresh nn.Conv2d there (lrp_modules.py:58-76): noise"""
    from lrp_amd.LRPtools import lrp_wrapper, lrp_modules
    conv = nn.Conv2d(2, 2, 3, padding=1, bias=False)
    conv.input = (torch.zeros(1, 2, 4, 4),)
    with pytest.raises(ValueError, match="without bias"):
        lrp_modules.Conv2d().propagate_relevance(conv, None, (torch.zeros(1, 2, 4, 4),), "alpha_beta", {"ignore_bias": False})
    with pytest.raises(ValueError, match="without bias"):
        lrp_wrapper.add_lrp(nn.Sequential(conv, nn.ReLU()), lrp_params={"alpha": 2., "beta": 1., "ignore_bias": False})
    assert lrp_modules.conv_rule_params(conv, {"alpha": 2., "beta": 1.}) == (2., 1., True)
    assert lrp_modules.conv_rule_params(nn.Conv2d(2, 2, 3), {"ignore_bias": False}) == (1., 0., False)
