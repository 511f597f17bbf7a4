"""Thin torch-tensor wrappers over the lrpx C ABI (include/lrpx.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every computation is a
hand-written HIP kernel inside csrc/liblrpx.so.  All tensors are CUDA(=HIP) float32 contiguous;
activations are NHWC ([maps, H*W, C])."""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import (ConvDesc, EPI_FIRST, EPI_FWD_DUAL, EPI_PLAIN, EPI_REL, EPI_REL_MUL, PACK_BWD_FIRST, PACK_BWD_POS,
                   PACK_DENSE, PACK_DENSE_T, PACK_FWD_DUAL, STAB_EPS, STAB_NONE, STAB_SAFE, check, ptr, stream_ptr)


def _dev(t):
    if t is not None and not t.is_cuda:
        raise ValueError("lrpx ops need device tensors (there is no CPU path)")
    return t


def conv_kc(hw, taps, cin):
    return _lib.load().lrpx_conv_kc(hw, taps, cin)


def pack_weights(w, cout, cin, taps, mode, kc):
    """w: conv (cout,cin,3,3) or dense 2-D matrix on device -> packed fragment-major tensor."""
    lib = _lib.load()
    _dev(w)
    if mode in (PACK_FWD_DUAL,):
        n_oc, k = 2 * cout, cin
    elif mode in (PACK_BWD_POS, _lib.PACK_BWD_PLAIN, PACK_DENSE_T):
        n_oc, k = cin, cout
    elif mode == PACK_BWD_FIRST:
        n_oc, k = 2 * cin, cout
    elif mode in (_lib.PACK_FWD_PN, _lib.PACK_FWD_PN_FIRST):
        n_oc, k = 2 * cout, (cin if mode == _lib.PACK_FWD_PN else 2 * cin)
    elif mode in (_lib.PACK_BWD_PN, _lib.PACK_BWD_PN_FIRST):
        n_oc, k = (cin if mode == _lib.PACK_BWD_PN else 2 * cin), 2 * cout
    else:
        n_oc, k = cout, cin
    n = lib.lrpx_packed_floats(n_oc, k, taps, kc)
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    check(lib.lrpx_pack_weights(ptr(w.contiguous()), cout, cin, taps, mode, kc, ptr(out), stream_ptr()))
    return out


def pack_weights_bf16x3(w, cout, cin, mode, taps=9):
    """3x3 conv weights (taps = 9) or a dense (cout, cin) matrix (taps = 1; PACK_BWD_PLAIN = the transposed product of the epsilon
    rules, as pack_weights_f16x2) -> three bf16 planes, w == p0 + p1 + p2 exactly, in fragment layout (for conv_mfma(..., bf16x6=1))."""
    lib = _lib.load()
    n_oc, k = (cout, cin) if mode == _lib.PACK_FWD else (cin, cout)
    out = torch.empty(lib.lrpx_packed_bf16x3_bytes(n_oc, k, taps) // 2, dtype=torch.int16, device=w.device)
    check(lib.lrpx_pack_weights_bf16x3(ptr(w.contiguous()), cout, cin, taps, mode, ptr(out), stream_ptr()))
    return out


def pack_weights_wino_b6(w, cout, cin, mode):
    """3x3 relevance weights (PACK_BWD_POS / PACK_BWD_PLAIN) in the Winograd F(2x2,3x3) form of conv mode 1: U = G g G^T per transform
    position, fp64 -> one rounding to fp32 -> three bf16 planes (for conv_mfma(..., bf16x6=1, wpacked_wino=...); csrc/conv_wino_b6.h)."""
    lib = _lib.load()
    out = torch.empty(lib.lrpx_packed_wino_b6_bytes(cin, cout) // 2, dtype=torch.int16, device=w.device)
    check(lib.lrpx_pack_weights_wino_b6(ptr(w.contiguous()), cout, cin, mode, ptr(out), stream_ptr()))
    return out


def set_b6_wino(bits):
    """lrpx_set_b6_wino: bit mask of the map sizes (56: 1, 28: 2, 14: 4) whose conv-mode-1 relevance convs run as Winograd
    (+ 8: the kernel's legacy patch staging, without column sharing between lanes - the same bits; default 15); returns the previous mask"""
    return _lib.load().lrpx_set_b6_wino(int(bits))


def pack_weights_f16x2(w, cout, cin, mode, taps=9):
    """3x3 conv weights (taps = 9) or a dense (cout, cin) matrix (taps = 1) -> layer-scaled fp16 hi/lo planes in fragment
    layout (for conv_mfma(..., f16x3=1)).  Dense: PACK_BWD_PLAIN = the transposed product  out[m, i] = sum_o a[m, o] w[o, i]
    of the epsilon rules (what PACK_DENSE_T is for the fp32 kernels)."""
    lib = _lib.load()
    n_oc, k = (cout, cin) if mode == _lib.PACK_FWD else (cin, cout)
    out = torch.empty(lib.lrpx_packed_f16x2_bytes(n_oc, k, taps) // 4, dtype=torch.float32, device=w.device)
    check(lib.lrpx_pack_weights_f16x2(ptr(w.contiguous()), cout, cin, taps, mode, ptr(out), stream_ptr()))
    return out


def pack_weights_f16f8(w, cout, cin, mode):
    """3x3 conv weights for conv_mfma(..., f16x3=2): fp16 hi planes + block-scaled fp6 fields of the cross-product operands."""
    lib = _lib.load()
    n_oc, k = (cin, cout)
    out = torch.empty(lib.lrpx_packed_f16f8_bytes(n_oc, k) // 4, dtype=torch.float32, device=w.device)
    check(lib.lrpx_pack_weights_f16f8(ptr(w.contiguous()), cout, cin, mode, ptr(out), stream_ptr()))
    return out


def zeros_arena(device, shapes):
    """{name: shape} -> {name: zero tensor}, all views of ONE allocation cleared by ONE fill (every view starts on a 256-byte boundary).
    A decoder trace is 11 - 21 small tensors: allocated one by one they cost a fill launch each (~5 us apiece on the stream)."""
    offs, total = {}, 0
    for k, shp in shapes.items():
        n = 1
        for d in shp:
            n *= int(d)
        offs[k] = (total, n)
        total += -(-n // 64) * 64
    flat = zeros(total, device=device)
    return {k: flat[o:o + n].view(*shapes[k]) for k, (o, n) in offs.items()}


def decoder_f16(mode=None):
    """Do the decoders' GEMMs (the (word, pixel) rules, the lock-step gate rules, the plain linears of a trace, the (T,V) scores) run on
    the fp16 split-product kernels (csrc/dense_f16x3.hip: two fp16 halves behind a power-of-two scale per ROW - 22 operand bits, 1.5 - 2.4x
    the decoder throughput)?  They FOLLOW the process's conv mode: in the default, exact mode 1 (and mode 0) every contraction of the
    path is fp32 arithmetic - the decoders on the fp32 MFMA (v_mfma_f32_16x16x4_f32 / 32x32x2) and fp32 VALU kernels, as the reference's
    `lrp_linear_eps` (models/gridTDmodel.py:744-765) and its nn.Linear forwards are - and only the opt-in speed modes 2 / 3 take the
    split products.  LRPX_DECODER_F16=0 / 1 overrides (A/B).  Read at every call of an engine (the packs of both kinds are built
    with the engine; `engine.force_f16 = True / False` pins one engine)."""
    v = os.environ.get("LRPX_DECODER_F16", "")
    if v != "":
        return v != "0"
    return (_lib.load().lrpx_set_conv_mode(-1) if mode is None else int(mode)) >= 2          # (mode: an engine's per-context conv mode)


def zeros(*shape, dtype=torch.float32, device="cuda"):
    """a zero tensor cleared THROUGH THE LIBRARY (lrpx_zero) on the current stream: a recorded step (_lib.Recording) then holds the
    clear like any other launch of the step (a `torch.zeros` would run once, at recording time, and never again)"""
    if torch.device(device).type != "cuda":          # (host-logic tests: layout checks of the arena without a GPU)
        return torch.zeros(*shape, dtype=dtype, device=device)
    t = torch.empty(*shape, dtype=dtype, device=device)
    if t.numel():
        check(_lib.load().lrpx_zero(ptr(t), t.numel() * t.element_size(), stream_ptr()))
    return t


def amax_maps(s, n_maps):
    """Float bits of max|s[n]| per map (int32 tensor): the operand scale an f16x3 convolution needs for its input."""
    s = _dev(s)
    out = torch.empty(n_maps, dtype=torch.int32, device=s.device)
    check(_lib.load().lrpx_amax_maps(ptr(s), n_maps, s.numel() // n_maps, ptr(out), stream_ptr()))
    return out


def conv_desc(inp, wpacked, n_maps, hw, cin, n_oc, taps, epi, *, pix_per_map=0, stab=STAB_NONE, oc_split=0,
              relu=0, bias=None, x=None, u=None, zdiv=None, map2img=None, out0=None, out1=None, bf16x6=0,
              f16x3=0, in_amax=None, out1_amax=None, pool_am=None, out0_amax=None, blocked=0, tile_group=0, out_chunk=0,
              in_chunked=0, wpacked_wino=None):
    """the lrpx_conv_desc of one contraction (the tensors must outlive its use: the descriptor holds raw pointers).
    tile_group / out_chunk / in_chunked: the tile-order hint and the K-chunked S layouts the VGG16 chain sets (include/lrpx.h)"""
    d = ConvDesc()
    d.in_, d.wpacked = ptr(_dev(inp)), ptr(_dev(wpacked))
    d.n_maps, d.hw, d.cin, d.n_oc, d.taps, d.pix_per_map = n_maps, hw, cin, n_oc, taps, pix_per_map
    d.epi, d.stab, d.oc_split, d.relu = epi, stab, oc_split, relu
    d.bf16x6, d.f16x3 = bf16x6, f16x3
    d.in_amax, d.out1_amax, d.pool_am, d.out0_amax = ptr(in_amax), ptr(out1_amax), ptr(pool_am), ptr(out0_amax)
    d.bias, d.x, d.u, d.zdiv, d.map2img = ptr(bias), ptr(x), ptr(u), ptr(zdiv), ptr(map2img)
    d.out0, d.out1 = ptr(out0), ptr(out1)
    d.blocked = blocked
    d.tile_group, d.out_chunk, d.in_chunked = tile_group, out_chunk, in_chunked
    d.wpacked_wino = ptr(_dev(wpacked_wino)) if wpacked_wino is not None else None
    return d


def nhwc_to_blocked(src, n_groups, pix_per_group, c):
    """NHWC [n_groups][pix][c] -> the BLOCKED layout of the mode-3 relevance kernels (csrc/blocked.h), one block set per group"""
    lib = _lib.load()
    dst = torch.zeros(n_groups * lib.lrpx_blocked_floats(pix_per_group, c), dtype=torch.float32, device=src.device)
    check(lib.lrpx_nhwc_to_blocked(ptr(_dev(src)), ptr(dst), n_groups, pix_per_group, c, stream_ptr()))
    return dst


def blocked_to_nhwc(src, n_groups, pix_per_group, c, out=None):
    if out is None:
        out = torch.empty(n_groups, pix_per_group, c, dtype=torch.float32, device=src.device)
    check(_lib.load().lrpx_blocked_to_nhwc(ptr(src), ptr(out), n_groups, pix_per_group, c, stream_ptr()))
    return out


def _conv_rel_mul_blocked(inp, wpacked, n_maps, hw, cin, n_oc, taps, epi, **kw):
    """The f16x3 = 2 REL_MUL kernels take `in` BLOCKED and, except the 224 x 224 one, x and the output too (the fused VGG16 chain
    keeps them so end to end).  For callers with NHWC tensors - the single-layer parity tests - convert at this boundary: in as one
    block set over all maps, x as one block set per image, the output back into the caller's tensor."""
    lib = _lib.load()
    ncol = kw.get("oc_split") or n_oc
    pin = (hw // 2) ** 2 if kw.get("pool_am") is not None else hw * hw
    x, out0, out1 = kw.get("x"), kw.get("out0"), kw.get("out1")
    kw = dict(kw)
    inb = nhwc_to_blocked(inp, 1, n_maps * pin, cin)
    if hw == 224:                      # conv1_2's kernel: NHWC multiplicand and output
        kw["blocked"] = 1
        d = conv_desc(inb, wpacked, n_maps, hw, cin, n_oc, taps, epi, **kw)
        check(lib.lrpx_conv_mfma(C.byref(d), stream_ptr()))
        return
    kw["blocked"] = 7
    if x is not None:
        kw["x"] = nhwc_to_blocked(x, x.shape[0], hw * hw, ncol)
    ob = None
    if out0 is not None or out1 is not None:
        ob = torch.zeros(lib.lrpx_blocked_floats(n_maps * hw * hw, ncol), dtype=torch.float32, device=inp.device)
        kw["out0"] = ob if out0 is not None else None
        kw["out1"] = ob if out1 is not None else None
    d = conv_desc(inb, wpacked, n_maps, hw, cin, n_oc, taps, epi, **kw)
    check(lib.lrpx_conv_mfma(C.byref(d), stream_ptr()))
    blocked_to_nhwc(ob, 1, n_maps * hw * hw, ncol, out=out0 if out0 is not None else out1)


def conv_mfma(inp, wpacked, n_maps, hw, cin, n_oc, taps, epi, **kw):
    if kw.get("f16x3") == 2 and epi == EPI_REL_MUL and not kw.get("blocked"):
        return _conv_rel_mul_blocked(inp, wpacked, n_maps, hw, cin, n_oc, taps, epi, **kw)
    d = conv_desc(inp, wpacked, n_maps, hw, cin, n_oc, taps, epi, **kw)
    check(_lib.load().lrpx_conv_mfma(C.byref(d), stream_ptr()))


def conv_geom_pack(w, direction):
    """w (cout, cin, kh, kw) on the device -> the packed fragments of `lrpx_conv_geom` for that direction (_lib.GEOM_FWD: K = cin,
    columns = cout; _lib.GEOM_BWD: K = cout, columns = cin).  Stacks of W+ / W- are built by the caller before packing."""
    lib = _lib.load()
    cout, cin, kh, kw = _dev(w).shape
    n_oc, k = (cout, cin) if direction == _lib.GEOM_FWD else (cin, cout)
    out = torch.empty(lib.lrpx_conv_geom_packed_floats(n_oc, k, kh * kw), dtype=torch.float32, device=w.device)
    check(lib.lrpx_conv_geom_pack(ptr(w.to(torch.float32).contiguous()), cout, cin, kh, kw, direction, ptr(out), stream_ptr()))
    return out


def conv_geom_pack_bf16x3(w, direction):
    """w (cout, cin, kh, kw) on the device -> the bf16x3 fragments of `lrpx_conv_geom_ex_b6` for that direction (as `conv_geom_pack`):
    every weight split exactly into three bf16 planes (csrc/conv_geom_b6.hip).  A uint8 tensor."""
    lib = _lib.load()
    cout, cin, kh, kw = w.shape
    k, n_oc = (cin, cout) if direction == _lib.GEOM_FWD else (cout, cin)
    out = torch.empty(lib.lrpx_conv_geom_packed_bf16x3_bytes(n_oc, k, kh * kw), dtype=torch.uint8, device=w.device)
    check(lib.lrpx_conv_geom_pack_bf16x3(ptr(w.to(torch.float32).contiguous()), cout, cin, kh, kw, direction, ptr(out), stream_ptr()))
    return out


def conv_geom(inp, wpacked, direction, n, hw, ohw, geom, k, n_oc, bias=None, x=None, out=None):
    """The runtime-geometry conv engine (csrc/conv_geom.hip), NHWC fp32.  hw = (H, W) the conv's input map, ohw = (OH, OW) its
    output map, geom = (kh, kw, sh, sw, ph, pw).  GEOM_FWD: inp (n, H W, k) -> out (n, OH OW, n_oc) (+ bias);
    GEOM_BWD: inp (n, OH OW, k) -> out (n, H W, n_oc) = x * convT(inp).  LAUNCHES counts it under 'conv_geom'."""
    _count("conv_geom", direction)
    pix =hw[0] * hw[1] if direction == _lib.GEOM_BWD else ohw[0] * ohw[1]
    if out is None:
        out = torch.empty(n, pix, n_oc, dtype=torch.float32, device=inp.device)
    d = _lib.ConvGeomDesc(ptr(_dev(inp)), ptr(_dev(wpacked)), ptr(_dev(bias)), ptr(_dev(x)), ptr(_dev(out)), direction,
                          n, hw[0], hw[1], ohw[0], ohw[1], *geom, k, n_oc)
    check(_lib.load().lrpx_conv_geom(C.byref(d), stream_ptr()))
    return out


def maxpool_rule(x, r_out, kernel, stride, padding):
    """Pool2d rule of an nn.MaxPool2d with any window (lrpx_maxpool_rule): x (N, C, H, W), r_out (N, C, OH, OW) contiguous fp32"""
    n, c, h, w = _dev(x).shape
    r_in = torch.empty_like(x)
    check(_lib.load().lrpx_maxpool_rule(ptr(x), ptr(_dev(r_out)), ptr(r_in), n * c, h, w, r_out.shape[2], r_out.shape[3],
                                        kernel[0], kernel[1], stride[0], stride[1], padding[0], padding[1], stream_ptr()))
    return r_in


def nchw_to_nhwc(src, c_pad=None):
    n, c, h, w = src.shape
    c_pad = c_pad or c
    dst = torch.empty(n, h * w, c_pad, dtype=torch.float32, device=src.device)
    check(_lib.load().lrpx_nchw_to_nhwc(ptr(src.contiguous()), ptr(dst), n, c, h * w, c_pad, stream_ptr()))
    return dst


def nhwc_to_nchw(src, c, h, w):
    n, p, c_src = src.shape
    dst = torch.empty(n, c, h, w, dtype=torch.float32, device=src.device)
    check(_lib.load().lrpx_nhwc_to_nchw(ptr(src), ptr(dst), n, c, p, c_src, stream_ptr()))
    return dst


def maxpool2x2_fwd(x, n, h, w, c):
    y = torch.empty(n, (h // 2) * (w // 2), c, dtype=torch.float32, device=x.device)
    check(_lib.load().lrpx_maxpool2x2_fwd(ptr(x), ptr(y), n, h, w, c, stream_ptr()))
    return y


def maxpool2x2_relevance(x, r_out, zdiv, map2img, n_maps, h_out, w_out, c, want_r=True, want_s=False):
    r_in = torch.empty(n_maps, 4 * h_out * w_out, c, dtype=torch.float32, device=x.device) if want_r else None
    s_out = torch.empty(n_maps, 4 * h_out * w_out, c, dtype=torch.float32, device=x.device) if want_s else None
    check(_lib.load().lrpx_maxpool2x2_relevance(ptr(x), ptr(r_out), ptr(zdiv), ptr(map2img), ptr(r_in), ptr(s_out),
                                                n_maps, h_out, w_out, c, 0, stream_ptr()))
    return r_in, s_out


def divide_stab(r, z, map2img, stab):
    n = r.shape[0]
    s = torch.empty_like(r)
    check(_lib.load().lrpx_divide_stab(ptr(r), ptr(z), ptr(map2img), ptr(s), n, r[0].numel(), stab, stream_ptr()))
    return s


def divide_alpha_beta(r, zpos, zneg, map2img, alpha, beta, out=None):
    """r (n_maps, pix, c), zpos / zneg (n_img, pix, c) -> s2 (n_maps, pix, 2c) = [alpha r/safe(z+) | -beta r/safe(z-)]: the two divisions
    of the general alpha-beta Conv2d rule in one pass (lrpx_divide_alpha_beta)"""
    n, pix, c = r.shape
    s2 = torch.empty(n, pix, 2 * c, dtype=torch.float32, device=r.device) if out is None else out
    check(_lib.load().lrpx_divide_alpha_beta(ptr(_dev(r)), ptr(_dev(zpos)), ptr(_dev(zneg)), ptr(map2img), ptr(s2), n, pix, c,
                                             float(alpha), float(beta), stream_ptr()))
    return s2


def maxpool2x2_relevance_ab(x, r_out, zpos, zneg, map2img, n_maps, h_out, w_out, c, alpha, beta, out=None):
    """the Pool2d rule fused with `divide_alpha_beta` by the Z+ / Z- of the conv below the pool: x, zpos, zneg (n_img, 4 h_out w_out, c),
    r_out (n_maps, h_out w_out, c) -> s2 (n_maps, 4 h_out w_out, 2c)  (lrpx_maxpool2x2_relevance_ab)"""
    s2 = torch.empty(n_maps, 4 * h_out * w_out, 2 * c, dtype=torch.float32, device=x.device) if out is None else out
    check(_lib.load().lrpx_maxpool2x2_relevance_ab(ptr(_dev(x)), ptr(_dev(r_out)), ptr(_dev(zpos)), ptr(_dev(zneg)), ptr(map2img), ptr(s2),
                                                   n_maps, h_out, w_out, c, float(alpha), float(beta), stream_ptr()))
    return s2


def cumsum_maps(maps, n_img, t_per_img, out=None):
    """running sums over the words of each image: what `explain_caption` returns (lrp_wrapper.py:64-82 quirk)"""
    if out is None:
        out = torch.empty_like(maps)
    check(_lib.load().lrpx_cumsum_maps(ptr(maps), ptr(out), n_img, t_per_img, maps[0].numel(), stream_ptr()))
    return out


def gather_rows(src, rows):
    """src (R, ...) 4-byte items, rows int32 (n,) on device -> (n, ...) = src[rows] (lrpx_gather_rows)"""
    src = _dev(src).contiguous()
    n = rows.shape[0]
    out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if n:
        check(_lib.load().lrpx_gather_rows(ptr(src), ptr(rows), ptr(out), n, src[0].numel(), stream_ptr()))
    return out


def scatter_maps(compact, rg, accumulate=False):
    """compact (n_valid, ...) results of the valid (image, word) rows of `rg` (explainers.ragged.RaggedRows) -> the padded
    (B*T, ...) layout: the rows themselves (accumulate: per-image running sums, the `explain_caption` quirk) and exact zeros
    behind every image's last word."""
    out = torch.empty((rg.B * rg.T,) + tuple(compact.shape[1:]), dtype=torch.float32, device=rg.rows.device)
    per = out[0].numel()
    if rg.n == 0:
        return out.zero_()
    check(_lib.load().lrpx_scatter_maps(ptr(_dev(compact).contiguous()), ptr(out), rg.B, rg.T, ptr(rg.lens), ptr(rg.offs), per,
                                        1 if accumulate else 0, stream_ptr()))
    return out


def check_relevance(buf, finite=True, nonzero=False):
    """The reference's inline asserts (lrp_modules.py:154-155, lrp_wrapper.py:81); syncs the stream."""
    check(_lib.load().lrpx_check(ptr(buf), buf.numel(), (1 if finite else 0) | (2 if nonzero else 0), stream_ptr()))


_EXPAND_CACHE = {}


def pyramid_expand_matrix(p, upscale, device="cuda"):
    """`skimage.transform.pyramid_expand(cam, upscale)` of a (p x p) map as ONE matrix: E = M cam M^T, M (p*upscale, p).
    scikit-image (the reference pins none; 0.16 was current for its PyTorch 1.4) computes
      resize(cam, order=1, mode='reflect', anti_aliasing=False): output row o samples the input at (o + 0.5) / upscale - 0.5,
          linear interpolation, out-of-range neighbours mirrored without repeating the edge (index -1 -> 1, p -> p - 2);
      ndi.gaussian_filter(sigma = 2 * upscale / 6, truncate 4, mode='reflect'): 2 * int(4 sigma + 0.5) + 1 taps, edge-repeating
          reflection (index -1 -> 0).
    Both are linear and separable, so they compose into M = Gauss @ Bilinear (built in float64 on the host, stored fp32)."""
    key = (p, upscale, str(device))
    if key not in _EXPAND_CACHE:
        import math
        import numpy as np
        hw = p * upscale
        Bm = np.zeros((hw, p))
        for o in range(hw):
            r = (o + 0.5) / upscale - 0.5
            r0 = math.floor(r)
            d = r - r0
            for idx, wgt in ((r0, 1.0 - d), (r0 + 1, d)):
                idx = -idx if idx < 0 else (2 * (p - 1) - idx if idx > p - 1 else idx)
                Bm[o, idx] += wgt
        sigma = 2.0 * upscale / 6.0
        lw = int(4.0 * sigma + 0.5)
        w = np.exp(-0.5 * (np.arange(-lw, lw + 1) / sigma) ** 2)
        w /= w.sum()
        G = np.zeros((hw, hw))
        for o in range(hw):
            for k in range(-lw, lw + 1):
                i = o + k
                i = -i - 1 if i < 0 else (2 * hw - 1 - i if i >= hw else i)
                G[o, i] += w[k + lw]
        _EXPAND_CACHE[key] = torch.from_numpy((G @ Bm).astype(np.float32)).to(device).contiguous()
    return _EXPAND_CACHE[key]


def guided_gradcam(guided_maps, cam, p=14):
    """guided_maps (N,C,HW,HW) * pyramid_expand(cam (N, p*p), upscale = HW / p)  (models/gridTDmodel.py:1826-1829)"""
    n, c, hw, _ = guided_maps.shape
    out = torch.empty_like(guided_maps)
    m = pyramid_expand_matrix(p, hw // p, guided_maps.device)
    check(_lib.load().lrpx_guided_gradcam(ptr(_dev(guided_maps).contiguous()), ptr(cam.contiguous()), ptr(m), ptr(out), n, p,
                                          hw, c, stream_ptr()))
    return out


def expand_maps(maps, hw, head=None, normalize=False, out=None):
    """Feature-resolution heat maps at image size: maps (R, P) or (R, NH, P) with P = p*p -> (R, hw, hw), each map
    `skimage.transform.pyramid_expand(a.reshape(p, p), upscale = hw / p)` - bit for bit the factor `guided_gradcam` multiplies by - and,
    normalize=True, divided by its max |.| as `evaluation.project_maxabs` would (evaluation.py:198-211, :390-407, :483-501, :744-750).
    head=None on (R, NH, P) is `np.mean(attention, axis=0)` (:202), head=k is `alphas[t][k]` (:744)."""
    if maps.dim() not in (2, 3):
        raise ValueError("expand_maps: maps must be (R, P) or (R, NH, P), got {}".format(tuple(maps.shape)))
    if maps.dim() == 2 and head is not None:
        raise ValueError("expand_maps: head selects among (R, NH, P) maps, got {}".format(tuple(maps.shape)))
    rows, heads, pp = maps.shape[0], (1 if maps.dim() == 2 else maps.shape[1]), maps.shape[-1]
    p = int(round(pp ** 0.5))
    if p * p != pp:
        raise ValueError("expand_maps: {} values per map are not a square grid".format(pp))        # the reference fails at `reshape`
    hw = int(hw)
    if hw <= 0 or hw % p:
        raise ValueError("expand_maps: the image size {} is not a multiple of the grid size {}".format(hw, p))    # ... at `mask * image`
    if head is not None and not 0 <= int(head) < heads:
        raise ValueError("expand_maps: head {} of {}".format(head, heads))
    _dev(maps)
    if out is None:
        out = torch.empty(rows, hw, hw, device=maps.device, dtype=torch.float32)
    elif tuple(out.shape) != (rows, hw, hw) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != maps.device:
        raise ValueError("expand_maps: out must be a contiguous float32 ({}, {}, {}) tensor on the maps' device".format(rows, hw, hw))
    if rows == 0:
        return out
    m = pyramid_expand_matrix(p, hw // p, maps.device)
    check(_lib.load().lrpx_expand_maps(ptr(maps.to(torch.float32).contiguous()), ptr(m), ptr(out), rows, heads,
                                       -1 if head is None else int(head), p, hw, 1 if normalize else 0, stream_ptr()))
    return out


class Vgg16:
    """VGG16 encoder context: packed weights + per-batch trace (device memory owned by torch)."""

    def __init__(self, weights, biases):
        lib = _lib.load()
        dev = weights[0].device
        self.device = dev
        self.packed = torch.empty(lib.lrpx_vgg16_packed_bytes() // 4, dtype=torch.float32, device=dev)
        ws = [w.contiguous() for w in weights]
        bs = [b.contiguous() for b in biases]
        wp = (C.c_void_p * 13)(*[w.data_ptr() for w in ws])
        bp = (C.c_void_p * 13)(*[b.data_ptr() for b in bs])
        check(lib.lrpx_vgg16_pack(wp, bp, ptr(self.packed), stream_ptr()))
        torch.cuda.current_stream().synchronize()   # ws/bs may be temporaries
        # the image-gradient chains in conv mode 3 keep the 1e-4 grade only while the rows of a 16-row weight slice stay within ~2^6 of
        # each other (lrpx_vgg16_row_spread, include/lrpx.h): beyond that this context runs them on the fp16 split products (mode 2)
        off = (lib.lrpx_vgg16_row_spread(ptr(self.packed)) - self.packed.data_ptr()) // 4
        spread = self.packed[off: off + 17].cpu()
        self.row_spread = float(max(spread[l] for l in range(17) if self.IS_CONV[l] and l > 0))
        self.grad_mode2 = self.row_spread > self.GRAD_SPREAD_MAX
        self.trace = None
        self.n_img = 0
        self._ws = None
        self._weights = ws              # (the model's own fp32 tensors where it has them: the alpha-beta packs are built from these on demand)
        self._ab = None                 # relevance_alpha_beta: packs, Z+ / Z- of the current trace, workspace
        self._ab1 = None                # relevance_alpha_beta(conv_mode=1): coefficients of the current trace, workspace
        self._ab1_packs = {"fwd": {}, "bwd": {}, "bwd_pos": {}, "rows": {}}     # ... its packs: ONE holder, shared with every replica, filled on demand
        self._trace_serial = 0
        # per-context matrix-core mode (None = the process default of lrpx_set_conv_mode / lrpx_set_forward_f16): carried in
        # every call (lrpx_vgg16_opts), so contexts with different modes can be in flight on different streams / threads
        self.conv_mode = None
        self.forward_f16 = None

    # Where the 64 comes from.  The mode-3 gradient kernels carry the two cross products (2^-11 of a product each)
    # as fp6 e2m3 fields behind ONE block scale per 16-row weight slice: a row whose maximum is s times below its slice's has its fields
    # rounded with a half-step of up to s / 60 of their own size (e2m3: half-step 2^-4 at field 1, slice maximum at >= 3.75).  A product
    # of such a row is therefore off by <= 2 x 2^-11 x s / 60 = s x 1.6e-5 of ITSELF, random sign.  An output element sums >= 9 x 16 =
    # 144 products of a slice and the chain has 12 such layers: if it were carried by the smallest rows alone its error would be about
    # s x 1.6e-5 x sqrt(12 / 144) = s x 4.7e-6, i.e. 1e-4 at s ~ 21; elements that large rows feed as well (all of them, with random
    # weights and gradients) dilute that by the rows' own ratio.  Measured on the oracle's activations: 7.6e-6 at s = 63
    # (tests/test_gpu_guided.py::test_gradient_chain_at_the_row_spread_boundary), 8.4e-5 at a slice spread of 2^13 and 1.1e-4 at 2^25
    # (log-normal rows, tests/test_gpu_vgg.py::test_chain_hostile_weights_all_modes): 64 keeps a 4x margin to the contract where the
    # model above would allow ~21 in the worst case and the data allow ~2^13.  Conv mode 1 (the default) has no such rule: exact splits.
    GRAD_SPREAD_MAX = 64.0
    feat_hw = (14, 14)              # the feature map of the 224 x 224 images this context is built for (ResNetEncoder.feat_hw: per trace)

    def _opts(self, layer_ms=None, grad=False):
        o = _lib.VggOpts()
        o.conv_mode = -1 if self.conv_mode is None else int(self.conv_mode)
        if grad and self.grad_mode2:
            cm, ff = C.c_int(0), C.c_int(0)
            check(_lib.load().lrpx_vgg16_resolve_opts(C.byref(o), C.byref(cm), C.byref(ff)))
            if cm.value == 3:
                o.conv_mode = 2
        o.forward_f16 = -1 if self.forward_f16 is None else int(self.forward_f16)
        o.layer_ms = layer_ms
        return C.byref(o)

    def replica(self):
        """Same packed weights, own trace / workspace buffers (for a second batch in flight on another stream)."""
        import copy
        r = copy.copy(self)
        r.trace, r.n_img, r._ws = None, 0, None
        r._ab, r._trace_serial = None, 0
        r._ab1 = None                   # (the mode-1 packs stay shared through `_ab1_packs`, whoever fills them first)
        if hasattr(r, "_ws_multi"):
            del r._ws_multi
        return r

    def forward(self, img_nchw):
        """Encoder.forward + trace (models/gridTDmodel.py:40-43).  Returns features (B,196,512) NHWC (a view
        into the trace)."""
        lib = _lib.load()
        n = img_nchw.shape[0]
        assert tuple(img_nchw.shape[1:]) == (3, 224, 224)
        need = lib.lrpx_vgg16_trace_bytes(n) // 4
        if self.trace is None or self.trace.numel() < need or self.n_img != n:
            self.trace = torch.empty(need, dtype=torch.float32, device=self.device)
        self.n_img = n
        self._trace_serial += 1         # (Z+ / Z- kept by relevance_alpha_beta belong to the previous trace)
        check(lib.lrpx_vgg16_forward_ex(ptr(self.packed), ptr(img_nchw.contiguous()), n, ptr(self.trace), None,
                                        self._opts(), stream_ptr()))
        off = lib.lrpx_vgg16_trace_features(ptr(self.trace), n) - self.trace.data_ptr()
        return self.trace[off // 4: off // 4 + n * 196 * 512].view(n, 196, 512)

    # (hw, channels) of act[l] for l = 0..17 and of zpos[l]
    ACT_DIMS = [(224, 8), (224, 64), (224, 64), (112, 64), (112, 128), (112, 128), (56, 128), (56, 256), (56, 256),
                (56, 256), (28, 256), (28, 512), (28, 512), (28, 512), (14, 512), (14, 512), (14, 512), (14, 512)]
    IS_CONV = [1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1]

    def channel_scales(self, layer):
        """rs (cout,) of conv layer `layer` (0..16): the trace keeps Z+ of that layer as rs[c] * conv(X, W+)[c] and the relevance
        packs carry rs[c] * W+[c, :] (exact powers of two; lrpx_vgg16_channel_scales, include/lrpx.h)."""
        n = C.c_int(0)
        p = _lib.load().lrpx_vgg16_channel_scales(ptr(self.packed), int(layer), C.byref(n))
        if not p:
            raise ValueError(f"layer {layer} is not a conv layer of VGG16 cfg 'D'")
        off = (p - self.packed.data_ptr()) // 4
        return self.packed[off: off + n.value]

    def trace_views(self):
        """Views of the saved per-layer tensors (what `module.input` is to the reference's hooks):
        ([act[0..17]] as (n_img, hw*hw, C), [zpos[l] or None]); zpos[l] is Z+ of conv l TIMES `channel_scales(l)` per channel."""
        lib = _lib.load()
        n = self.n_img
        a_off = (C.c_size_t * 18)()
        z_off = (C.c_size_t * 17)()
        check(lib.lrpx_vgg16_trace_layout(n, a_off, z_off))
        acts, zs = [], []
        for l in range(18):
            hw, c = self.ACT_DIMS[l]
            acts.append(self.trace[a_off[l]: a_off[l] + n * hw * hw * c].view(n, hw * hw, c))
        for l in range(17):
            if self.IS_CONV[l]:
                c = self.ACT_DIMS[l + 1][1]
                hw = self.ACT_DIMS[l][0]
                zs.append(self.trace[z_off[l]: z_off[l] + n * hw * hw * c].view(n, hw * hw, c))
            else:
                zs.append(None)
        return acts, zs

    def derive(self):
        """Recompute the trace tensors derived from the activations (call after writing into `trace_views()`)."""
        check(_lib.load().lrpx_vgg16_trace_derive(ptr(self.trace), self.n_img, stream_ptr()))

    def gradient(self, d_feat_nhwc, map2img=None, out=None):
        """explain_cnn of the plain-gradient explainer (models/gridTDmodel.py:1507-1521): the autograd gradient of the
        encoder output w.r.t. the image for (N,196,512) output gradients -> (N,3,224,224)."""
        return self.guided_backprop(d_feat_nhwc, map2img, out, _fn="lrpx_vgg16_gradient_ex")

    def guided_backprop(self, d_feat_nhwc, map2img=None, out=None, _fn="lrpx_vgg16_guided_backprop_ex"):
        """explain_cnn of the guided-backprop explainer (models/gridTDmodel.py:1702-1723): (N,196,512) gradient at
        the encoder output -> (N,3,224,224) image gradient with the guided ReLU rule."""
        lib = _lib.load()
        n_maps = d_feat_nhwc.shape[0]
        need = lib.lrpx_vgg16_workspace_bytes(n_maps) // 4
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
        if out is None:
            out = torch.empty(n_maps, 3, 224, 224, dtype=torch.float32, device=self.device)
        check(getattr(lib, _fn)(ptr(self.packed), ptr(self.trace), self.n_img, ptr(d_feat_nhwc.contiguous()),
                                ptr(map2img), n_maps, ptr(self._ws), ptr(out), self._opts(grad=True), stream_ptr()))
        return out

    # ---- the general alpha-beta rule through the encoder --------------------------------------------------------
    AB_BLOCK = 8        # maps per pass at 224 x 224; the deeper stages take as many maps as the same workspace holds (relevance_alpha_beta)
    AB_STAGES = ((16, 15, 14), (12, 11, 10), (8, 7, 6), (4, 3), (1, 0))      # conv layers of one map size, top down (a pool between two stages)

    def _ab_state(self):
        """packs of the 13 conv layers for the general rule (built once per context) and the workspace of one block of maps"""
        if self._ab is None:
            lib = _lib.load()
            st = {"fwd": {}, "bwd": {}, "neg": {}, "serial": -1, "zpos": {}, "zneg": {}}
            convs = [l for l in range(17) if self.IS_CONV[l]]
            for l, w in zip(convs, self._weights):
                hw, cout, cin = self.ACT_DIMS[l][0], int(w.shape[0]), int(w.shape[1])
                k_in = self.ACT_DIMS[l][1]                 # channels of act[l]: 8 = [x+ | x- | 0 0] for conv1_1, cin above
                kc_f, kc_b = conv_kc(hw, 9, k_in), conv_kc(hw, 9, 2 * cout)
                first = l == 0
                st["fwd"][l] = pack_weights(w, cout, cin, 9, _lib.PACK_FWD_PN_FIRST if first else _lib.PACK_FWD_PN, kc_f)
                st["bwd"][l] = pack_weights(w, cout, cin, 9, _lib.PACK_BWD_PN_FIRST if first else _lib.PACK_BWD_PN, kc_b)
                st["neg"][l] = lib.lrpx_packed_floats(cout, k_in, 9, kc_f)      # channel-block major: where the Z- half starts
            self._ab = st
        return self._ab

    def _ab_zpn(self, st):
        """Z+ = conv(x, W+) and Z- = conv(x, W-) of the 13 conv layers from the trace's activations, per IMAGE (conv1_1 on the split
        image: Z+ = x+ W+ + x- W-, Z- = x+ W- + x- W+); kept until the next forward()."""
        if st["serial"] == self._trace_serial:
            return
        acts, _ = self.trace_views()
        n = self.n_img
        for l in st["fwd"]:
            hw, k_in = self.ACT_DIMS[l]
            cout = self.ACT_DIMS[l + 1][1]
            for name, pk in (("zpos", st["fwd"][l]), ("zneg", st["fwd"][l][st["neg"][l]:])):
                z = st[name].get(l)
                if z is None or z.shape[0] != n:
                    z = st[name][l] = torch.empty(n, hw * hw, cout, dtype=torch.float32, device=self.device)
                conv_mfma(acts[l], pk, n, hw, k_in, cout, 9, EPI_PLAIN, oc_split=cout, out0=z)
        st["serial"] = self._trace_serial

    def relevance_alpha_beta(self, r_feat_nhwc, map2img=None, alpha=2., beta=1., out=None, layer_ms=None, conv_mode=0):
        """compute_lrp (LRPtools/lrp_wrapper.py:63-87) with the preset's Conv2d rule replaced by the general alpha-beta rule without
        bias, R = alpha * lrp_backward(PosNetConv) - beta * lrp_backward(NegNetConv) (lrp_modules.py:124-150), for N maps:
        (N,196,512) -> (N,3,224,224); maps of one image share that image's trace through `map2img` (null = map n on image n), the
        same contract as `relevance()`.  ReLU passes relevance through, MaxPool2d routes it to the first maximum (:172-195).

        Z+ / Z- of the 13 conv layers come from the trace's activations, one pass per layer per IMAGE at the first call after a
        `forward()` (about 108 MB per image, kept until the next `forward()`).  Then per layer, top down: [alpha R/safe(Z+) |
        -beta R/safe(Z-)] in one pass (fused with the Pool2d rule under the four pools), and ONE transposed conv over the stacked
        K = 2 cout with the activations as multiplicand.  Every contraction is the fp32 MFMA (`lrpx_conv_mfma` without split
        operands) whatever the process's or the context's conv mode is: the grade of conv mode 0.

        The maps are walked in blocks so that the workspace is bounded whatever N is: AB_BLOCK = 8 maps at 224 x 224, where S2 of
        conv1_2 is 25.7 MB per map, and at the deeper stages as many maps as fit the same S2 buffer (16 at 112^2, 32 at 56^2, 64 at
        28^2, 256 at 14^2 - 8 maps of 14 x 14 pixels are 28 workgroups, a launch that leaves most of the chip idle).  A stage hands
        its blocks on to the stage below, so each of the five stages owns two relevance buffers of 8 x 224^2 x 64 floats beside
        the one S2 buffer of 8 x 224^2 x 128 floats: 8 x 224^2 x (128 + 10 x 64) x 4 = 1 233 125 376 bytes.  A map's result does
        not depend on the blocks it travels in.
        layer_ms: a list of 17 floats - the call then adds each layer's milliseconds (HIP events, one wait per layer: profiling).

        conv_mode=0 (the default) is everything above.  conv_mode=1 runs the rule in the exact bf16-split arithmetic of conv mode 1 on
        the runtime-geometry engine, the design of `ResNetEncoder.relevance_alpha_beta`: per image and forward()
        the coefficients qp = win / safe(Z+), qn = win / safe(Z-) (`_ab1_coef`; win: the Pool2d rule of a pool above the conv as a
        0 / 1 factor), then per map 13 launches of `conv_geom_ab(b6=True)` - the operand (R qp) alpha | (R qn) (-beta) is formed
        while the tile is gathered, under the four pools from the relevance at the POOLED resolution (pool=2) - and one
        `resnet_stem_fold`.  No S2, no Pool2d pass; beta == 0 contracts over W+ alone.  The maps travel in blocks of AB1_BLOCK
        through two relevance buffers; no kernel has atomics, a map's result does not depend on its block.  Modes 2 / 3: ValueError."""
        alpha, beta = float(alpha), float(beta)
        if not (alpha == alpha and beta == beta and abs(alpha) != float("inf") and abs(beta) != float("inf")):
            raise ValueError("relevance_alpha_beta: alpha and beta must be finite")
        if isinstance(conv_mode, bool) or conv_mode not in (0, 1):
            raise ValueError("relevance_alpha_beta: conv_mode is 0 (fp32 MFMA) or 1 (exact bf16 split), got {!r}".format(conv_mode))
        if self.trace is None:
            raise ValueError("relevance_alpha_beta: no trace - call forward() first")
        r_feat_nhwc = _dev(r_feat_nhwc).contiguous()
        n_maps = r_feat_nhwc.shape[0]
        if tuple(r_feat_nhwc.shape[1:]) != (196, 512):
            raise ValueError("relevance_alpha_beta: r_feat_nhwc must be (N, 196, 512)")
        if map2img is None:
            if n_maps != self.n_img:
                raise ValueError("relevance_alpha_beta: without map2img there is one map per image of the trace")
            map2img = torch.arange(n_maps, dtype=torch.int32, device=self.device)
        if conv_mode == 1:
            return self._ab1_chain(r_feat_nhwc, map2img.contiguous(), alpha, beta, out, layer_ms)
        st = self._ab_state()
        self._ab_zpn(st)
        if out is None:
            out = torch.empty(n_maps, 3, 224, 224, dtype=torch.float32, device=self.device)
        px = int(self.AB_BLOCK) * 224 * 224
        ws = st.get("ws")
        if ws is None or ws.numel() != px * (128 + 64 * 2 * len(self.AB_STAGES)):
            ws = st["ws"] = torch.empty(px * (128 + 64 * 2 * len(self.AB_STAGES)), dtype=torch.float32, device=self.device)
        self._ab_walk(st, 0, r_feat_nhwc, map2img.contiguous(), out, alpha, beta, layer_ms, self.trace_views()[0], px)
        return out

    def _ab_walk(self, st, si, r_in, map2img, out, alpha, beta, layer_ms, acts, px):
        """stage `si` of relevance_alpha_beta for the maps of r_in - the relevance at the output of the stage's top conv or, with a
        pool above it, behind that pool - block by block, each block handed on to the stage below; the last stage writes `out`"""
        lib = _lib.load()
        layers = self.AB_STAGES[si]
        ws = st["ws"]
        s2_ws = ws[:px * 128]
        r_ws = [ws[px * (128 + 64 * (2 * si + k)): px * (128 + 64 * (2 * si + k + 1))] for k in (0, 1)]
        hw = self.ACT_DIMS[layers[0]][0]
        block = min(px * 128 // (hw * hw * 2 * self.ACT_DIMS[l + 1][1]) for l in layers)
        for lo in range(0, r_in.shape[0], block):
            nb = min(block, r_in.shape[0] - lo)
            r, m2i = r_in[lo: lo + nb], map2img[lo: lo + nb]
            cur = 0
            for l in layers:
                if layer_ms is not None:
                    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    ev[0].record()
                k_in, cout = self.ACT_DIMS[l][1], self.ACT_DIMS[l + 1][1]
                s2 = s2_ws[: nb * hw * hw * 2 * cout].view(nb, hw * hw, 2 * cout)
                if l + 1 < 17 and not self.IS_CONV[l + 1]:          # r is the relevance BEHIND the pool above this conv
                    maxpool2x2_relevance_ab(acts[l + 1], r, st["zpos"][l], st["zneg"][l], m2i, nb, hw // 2, hw // 2, cout, alpha, beta, out=s2)
                else:
                    divide_alpha_beta(r, st["zpos"][l], st["zneg"][l], m2i, alpha, beta, out=s2)
                r_new = r_ws[cur][: nb * hw * hw * k_in].view(nb, hw * hw, k_in)
                conv_mfma(s2, st["bwd"][l], nb, hw, 2 * cout, -(-k_in // 32) * 32, 9, EPI_REL, oc_split=k_in, x=acts[l], map2img=m2i, out0=r_new)
                r, cur = r_new, 1 - cur
                if layer_ms is not None:
                    ev[1].record()
                    ev[1].synchronize()
                    layer_ms[l] += ev[0].elapsed_time(ev[1])
            if si + 1 < len(self.AB_STAGES):
                self._ab_walk(st, si + 1, r, m2i, out[lo: lo + nb], alpha, beta, layer_ms, acts, px)
                continue
            # conv1_1 left [x+ convT(.) | x- convT(.) | 0 0] in 8 channels: join the halves into the NCHW result
            tmp = r_ws[cur][: nb * 3 * 224 * 224].view(nb, 3, 224, 224)
            o = out[lo: lo + nb]
            check(lib.lrpx_nhwc_to_nchw(ptr(r), ptr(o), nb, 3, 224 * 224, 8, stream_ptr()))
            check(lib.lrpx_nhwc_to_nchw(_lib.ptr_at(r, 3), ptr(tmp), nb, 3, 224 * 224, 8, stream_ptr()))
            check(lib.lrpx_accumulate(ptr(o), ptr(tmp), o.numel(), stream_ptr()))

    # ---- the same rule on the exact bf16 splits: relevance_alpha_beta(conv_mode=1) ---------------------------------
    AB1_BLOCK = 16      # maps per pass: two relevance buffers of 16 x 224^2 x 64 floats
    AB1_COEF_FLOATS = 4 * 224 * 224 * 128       # the [Z+ | Z-] rows of one coefficient pass: 4 images at conv1_2, more where the maps are smaller
    _GEOM3 = (3, 3, 1, 1, 1, 1)

    def _ab1_state(self):
        """bf16x3 packs of the 13 convs, built once per context from `self._weights`: `fwd`, the columns [W+ | W-] (conv1_1 on the
        split image [x+ | x- | 0 0]: Z+ = x+ W+ + x- W-, Z- = x+ W- + x- W+) and `bwd`, the transposed pack of the rows [W+ ; W-]
        (conv1_1: [W+ | W- | 0 0 ; W- | W+ | 0 0]); `bwd_pos`, the W+ rows alone, at the first call with beta == 0.  The packs live in
        `_ab1_packs`, one holder that a context and all its replicas share (a replica made before the first alpha-beta call
        included); coefficients and workspace are per context."""
        st = self._ab1_packs
        if not st["fwd"]:
            convs = [l for l in range(17) if self.IS_CONV[l]]
            for l, w in zip(convs, self._weights):
                wt = w.detach().to(torch.float32)
                wpos, wneg = wt.clamp(min=0), wt.clamp(max=0)
                if l == 0:
                    pad = torch.zeros(wt.shape[0], 8 - 2 * wt.shape[1], 3, 3, device=self.device)
                    wpos, wneg = torch.cat([wpos, wneg, pad], 1), torch.cat([wneg, wpos, pad], 1)
                rows = torch.cat([wpos, wneg], 0)
                st["fwd"][l] = conv_geom_pack_bf16x3(rows, _lib.GEOM_FWD)
                st["bwd"][l] = conv_geom_pack_bf16x3(rows, _lib.GEOM_BWD)
                st["rows"][l] = wpos
            torch.cuda.current_stream().synchronize()
        if self._ab1 is None:
            self._ab1 = dict(st, serial=-1, qp={}, qn={}, ws=None)      # (the pack dicts themselves: shared)
        return self._ab1

    def _ab1_coef(self, st):
        """qp = win / safe(Z+), qn = win / safe(Z-) of the 13 convs, per IMAGE, from the trace's activations: one stacked forward
        contraction [Z+ | Z-] (`conv_geom_ex`, exact splits, blocked sums) and one streaming pass (`vgg16_ab_coef`) per conv, a few images at a time;
        win is the Pool2d rule of the pool above conv1_2 / 2_2 / 3_3 / 4_3 from that pool's input.  Independent of alpha and beta;
        kept until the next forward() (13.5 M floats per image and coefficient: 108 MB per image)."""
        if st["serial"] == self._trace_serial:
            return
        acts, _ = self.trace_views()
        n = self.n_img
        for l in st["fwd"]:
            hw, k_in = self.ACT_DIMS[l]
            cout = self.ACT_DIMS[l + 1][1]
            pooled = l + 1 < 17 and not self.IS_CONV[l + 1]
            for name in ("qp", "qn"):
                if st[name].get(l) is None or st[name][l].shape[0] != n:
                    st[name][l] = torch.empty(n, hw * hw, cout, dtype=torch.float32, device=self.device)
            step = max(1, min(n, self.AB1_COEF_FLOATS // (hw * hw * 2 * cout)))
            zz = torch.empty(step, hw * hw, 2 * cout, dtype=torch.float32, device=self.device)
            for lo in range(0, n, step):
                nb = min(step, n - lo)
                conv_geom_ex(acts[l][lo: lo + nb], st["fwd"][l], _lib.GEOM_FWD, nb, (hw, hw), (hw, hw), self._GEOM3, k_in, 2 * cout,
                             out=zz[:nb], b6=True, blocked=True)
                vgg16_ab_coef(zz[:nb], st["qp"][l][lo: lo + nb], st["qn"][l][lo: lo + nb], nb, (hw, hw), cout,
                              xpool=acts[l + 1][lo: lo + nb] if pooled else None)
        st["serial"] = self._trace_serial

    def _ab1_chain(self, r_feat, map2img, alpha, beta, out, layer_ms):
        """relevance_alpha_beta(conv_mode=1) for checked arguments: block by block, top down, 13 `conv_geom_ab` + `resnet_stem_fold`"""
        st = self._ab1_state()
        self._ab1_coef(st)
        dual = beta != 0.
        if not dual and not st["bwd_pos"]:
            for l, wpos in st["rows"].items():
                st["bwd_pos"][l] = conv_geom_pack_bf16x3(wpos, _lib.GEOM_BWD)
            torch.cuda.current_stream().synchronize()
        packs = st["bwd"] if dual else st["bwd_pos"]
        n_maps = r_feat.shape[0]
        if out is None:
            out = torch.empty(n_maps, 3, 224, 224, dtype=torch.float32, device=self.device)
        map2img = check_map2img(map2img, n_maps, self.n_img)
        per = 224 * 224 * 64
        if st["ws"] is None or st["ws"].numel() != 2 * int(self.AB1_BLOCK) * per:
            st["ws"] = torch.empty(2 * int(self.AB1_BLOCK) * per, dtype=torch.float32, device=self.device)
        bufs = (st["ws"][: int(self.AB1_BLOCK) * per], st["ws"][int(self.AB1_BLOCK) * per:])
        acts = self.trace_views()[0]
        layers = [l for l in range(16, -1, -1) if self.IS_CONV[l]]
        for lo in range(0, n_maps, int(self.AB1_BLOCK)):
            nb = min(int(self.AB1_BLOCK), n_maps - lo)
            r, m2i, cur = r_feat[lo: lo + nb], map2img[lo: lo + nb], 0
            for l in layers:
                ev = _events(layer_ms)
                hw, k_in = self.ACT_DIMS[l]
                cout = self.ACT_DIMS[l + 1][1]
                pooled = l + 1 < 17 and not self.IS_CONV[l + 1]           # r is the relevance BEHIND the pool above this conv
                r_new = bufs[cur][: nb * hw * hw * k_in].view(nb, hw * hw, k_in)
                conv_geom_ab(r, packs[l], nb, (hw, hw), (hw, hw), self._GEOM3, cout, k_in, acts[l], st["qp"][l],
                             q2=st["qn"][l] if dual else None, scale=alpha, scale2=-beta if dual else 0., map2img=m2i, n_img=self.n_img,
                             out=r_new, validate=False, b6=True, pool=2 if pooled else 1)
                r, cur = r_new, 1 - cur
                if ev is not None:
                    ev[1].record()
                    ev[1].synchronize()
                    layer_ms[l] += ev[0].elapsed_time(ev[1])
            # conv1_1 left [x+ convT(.) | x- convT(.) | 0 0] in 8 channels: join the halves into the NCHW result
            resnet_stem_fold(r, out[lo: lo + nb], nb, 3, 3, 8, 224 * 224)
        return out

    def relevance(self, r_feat_nhwc, map2img=None, out=None, streams=1, layer_ms=None):
        """compute_lrp (LRPtools/lrp_wrapper.py:63-87) for N maps: (N,196,512) -> (N,3,224,224).
        streams=2 splits the maps over two HIP streams (maps are independent): the HBM-bound pool / first-layer
        kernels and the tail wave of each MFMA launch of one half overlap with MFMA work of the other half.
        layer_ms: a ctypes (c_float * 17) array - this call then times its conv launches with HIP events of its own and
        waits for them (profiling; one stream only)."""
        lib = _lib.load()
        n_maps = r_feat_nhwc.shape[0]
        r_feat_nhwc = r_feat_nhwc.contiguous()
        if out is None:
            out = torch.empty(n_maps, 3, 224, 224, dtype=torch.float32, device=self.device)
        if streams <= 1 or n_maps < 2 * streams or map2img is None:
            need = lib.lrpx_vgg16_workspace_bytes(n_maps) // 4
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
            if layer_ms is None and self.conv_mode is None:
                # plain entry point: honours the thread's legacy lrpx_vgg16_layer_timing switch
                check(lib.lrpx_vgg16_relevance(ptr(self.packed), ptr(self.trace), self.n_img, ptr(r_feat_nhwc),
                                               ptr(map2img), n_maps, ptr(self._ws), ptr(out), stream_ptr()))
            else:
                lm = None if layer_ms is None else C.cast(layer_ms, C.POINTER(C.c_float))
                check(lib.lrpx_vgg16_relevance_ex(ptr(self.packed), ptr(self.trace), self.n_img, ptr(r_feat_nhwc),
                                                  ptr(map2img), n_maps, ptr(self._ws), ptr(out), self._opts(lm),
                                                  stream_ptr()))
            return out
        per = -(-n_maps // streams)
        need = lib.lrpx_vgg16_workspace_bytes(per) // 4
        if getattr(self, "_ws_multi", None) is None or self._ws_multi[0].numel() < need or len(self._ws_multi) < streams:
            self._ws_multi = [torch.empty(need, dtype=torch.float32, device=self.device) for _ in range(streams)]
            self._side = [torch.cuda.Stream() for _ in range(streams)]
        cur = torch.cuda.current_stream()
        for i in range(streams):
            lo, hi = i * per, min((i + 1) * per, n_maps)
            if lo >= hi:
                break
            st = self._side[i]
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                check(lib.lrpx_vgg16_relevance_ex(ptr(self.packed), ptr(self.trace), self.n_img, ptr(r_feat_nhwc[lo:hi]),
                                                  ptr(map2img[lo:hi]), hi - lo, ptr(self._ws_multi[i]), ptr(out[lo:hi]),
                                                  self._opts(), C.c_void_p(st.cuda_stream)))
        for i in range(streams):
            cur.wait_stream(self._side[i])
        return out


# ---- the batched bottleneck-ResNet encoder engine ------------------------------------------------------------------
LAUNCHES = {}        # (wrapper name, direction) -> calls since the process started: the tests' evidence of what a pass launches


def _count(name, direction=None):
    LAUNCHES[(name, direction)] = LAUNCHES.get((name, direction), 0) + 1


def check_map2img(map2img, n_maps, n_img):
    """map2img (n_maps,) int32 on the device with every entry in [0, n_img) - checked on the HOST (one small copy), before any kernel
    sees it: the kernels index the per-image operands with it unchecked.  LrpxError otherwise."""
    if not (isinstance(map2img, torch.Tensor) and map2img.dtype == torch.int32 and map2img.dim() == 1 and map2img.shape[0] == n_maps):
        raise _lib.LrpxError("map2img must be an int32 tensor of n_maps = {} entries (LRPX_EINVAL)".format(n_maps))
    _dev(map2img)
    if n_maps:
        host = map2img.cpu()
        lo, hi = int(host.min()), int(host.max())
        if lo < 0 or hi >= n_img:
            raise _lib.LrpxError("map2img entry {} outside [0, {}) (LRPX_EINVAL)".format(lo if lo < 0 else hi, n_img))
    return map2img.contiguous()


def _conv_geom_desc(fn, direction, inp, wpacked, n, hw, ohw, geom, k, n_oc, k_inp, kname, operands, bias, x, q, addend, map2img, n_img, out,
                    validate, pix_inp=None):
    """What the `conv_geom_ex` / `_ab` / `_grad` wrappers share, each refusal once under the wrapper's name `fn`: the shapes of the
    transposed direction's per-image `operands` = (name, tensor, kind, required), kind 'x' (n_img, H W, n_oc) | 'q' (n_img, OH OW, k_inp)
    | 'k' (k_inp,), of the addend and of the input (k_inp channels, named `kname`; k is the contraction's length), `check_map2img`
    where asked, `out` allocated or refused.  pix_inp: the pixels per map of the input where they are not the source map's (the pooled
    operand of `conv_geom_ab(pool=2)`).  -> (the base ConvGeomExDesc, out)."""
    bwd = direction == _lib.GEOM_BWD
    pix_in, pix_out = (ohw[0] * ohw[1], hw[0] * hw[1]) if bwd else (hw[0] * hw[1], ohw[0] * ohw[1])
    if bwd:
        n_img = n if n_img is None else n_img
        for name, t, kind, required in operands:
            want = (n_img, pix_out, n_oc) if kind == "x" else (n_img, pix_in, k_inp) if kind == "q" else (k_inp,)
            if (required if t is None else tuple(t.shape) != want):
                raise ValueError("{}: {} must be {}".format(fn, name, {"x": "(n_img, H W, n_oc)", "q": "(n_img, OH OW, {})".format(kname),
                                                                          "k": "({},)".format(kname)}[kind]))
        if addend is not None and tuple(addend.shape) != (n, pix_out, n_oc):
            raise ValueError("{}: addend must have the output's shape".format(fn))
        if map2img is not None and validate:
            map2img = check_map2img(map2img, n, n_img)
    pix_inp = pix_in if pix_inp is None else pix_inp
    if inp.numel() != n * pix_inp * k_inp:
        raise ValueError("{}: the input must hold n x pixels x {} = {} x {} x {} floats".format(fn, kname, n, pix_inp, k_inp))
    if out is None:
        out = torch.empty(n, pix_out, n_oc, dtype=torch.float32, device=inp.device)
    elif out.numel() != n * pix_out * n_oc:
        raise ValueError("{}: the output must hold n x pixels x n_oc floats".format(fn))
    return _lib.ConvGeomExDesc(ptr(_dev(inp)), ptr(_dev(wpacked)), ptr(_dev(bias)), ptr(_dev(x)), ptr(_dev(q)), ptr(_dev(addend)),
                               ptr(_dev(map2img)), ptr(_dev(out)), direction, n, n_img or 0, hw[0], hw[1], ohw[0], ohw[1], *geom, k, n_oc), out


def conv_geom_ex(inp, wpacked, direction, n, hw, ohw, geom, k, n_oc, bias=None, x=None, q=None, addend=None, map2img=None, n_img=None,
                 out=None, validate=True, b6=False, blocked=False):
    """`lrpx_conv_geom_ex` (csrc/conv_geom.hip; b6: `lrpx_conv_geom_ex_b6`, csrc/conv_geom_b6.hip, the exact bf16-split arithmetic of
    conv mode 1, with wpacked from `conv_geom_pack_bf16x3`), NHWC fp32; hw / ohw / geom as `conv_geom`.  GEOM_FWD: inp (n, H W, k) -> out
    (n, OH OW, n_oc) (+ bias).  GEOM_BWD: inp (n maps, OH OW, k) -> out (n, H W, n_oc) = x[img] * convT(inp * q[img]) + addend with
    img = map2img[m] (None: identity); x (n_img, H W, n_oc), q (n_img, OH OW, k), addend like out.  validate: check map2img on the host
    first (`check_map2img`; a caller that already has passes False).  blocked (b6, GEOM_FWD only): `lrpx_conv_geom_ex_b6_blocked`, the same
    sums in a blocked order - fewer roundings at the running sum's size, for the Z+ / Z- of the alpha-beta coefficients."""
    if blocked and (not b6 or direction != _lib.GEOM_FWD):
        raise ValueError("conv_geom_ex: blocked goes with b6 and the forward direction")
    d, out = _conv_geom_desc("conv_geom_ex", direction, inp, wpacked, n, hw, ohw, geom, k, n_oc, k, "k",
                             (("x", x, "x", True), ("q", q, "q", False)), bias, x, q, addend, map2img, n_img, out, validate)
    if blocked:
        _count("conv_geom_ex_b6_blocked", direction)
        check(_lib.load().lrpx_conv_geom_ex_b6_blocked(C.byref(d), stream_ptr()))
        return out
    if b6:
        _count("conv_geom_ex_b6", direction)
        check(_lib.load().lrpx_conv_geom_ex_b6(C.byref(d), stream_ptr()))
        return out
    _count("conv_geom_ex", direction)
    check(_lib.load().lrpx_conv_geom_ex(C.byref(d), stream_ptr()))
    return out


def conv_geom_ab(inp, wpacked, n, hw, ohw, geom, kr, n_oc, x, q, q2=None, scale=1., scale2=0., addend=None, map2img=None, n_img=None,
                 out=None, validate=True, b6=False, pool=1):
    """`lrpx_conv_geom_ab` (b6: `lrpx_conv_geom_ab_b6`): the transposed direction of `conv_geom_ex` with two coefficients, the general
    alpha-beta rule of a conv without bias (include/lrpx.h).  inp (n maps, OH OW, kr) -> out (n, H W, n_oc) =
    x[img] * (convT((inp q[img]) scale, W+) + convT((inp q2[img]) scale2, W-)) + addend; q / q2 (n_img, OH OW, kr).  wpacked: the
    transposed pack of the rows [W+ ; W-] (2 kr of them) - or, with q2 None (beta == 0), of W+ alone: the contraction then runs over
    kr only.  LAUNCHES counts the two under 'conv_geom_ab_dual' and 'conv_geom_ab' (b6: + '_b6').
    pool=2 (`lrpx_conv_geom_ab_pool`, `_b6`): the conv sits directly under a 2x2 / stride-2 max-pool and inp is the
    relevance BEHIND the pool, (n maps, (OH // 2) (OW // 2), kr); q / q2 stay at the conv's resolution and carry the pool's winner
    factor (`vgg16_ab_coef`).  LAUNCHES: the same names + '_pool'.  Any other pool but 1 is refused."""
    if pool not in (1, 2):
        raise ValueError("conv_geom_ab: pool is 1 (none) or 2 (kernel = stride = 2, no padding, floor mode), got {!r}".format(pool))
    base, out = _conv_geom_desc("conv_geom_ab", _lib.GEOM_BWD, inp, wpacked, n, hw, ohw, geom, kr if q2 is None else 2 * kr, n_oc, kr, "kr",
                                (("x", x, "x", True), ("q", q, "q", True), ("q2", q2, "q", False)), None, x, q, addend, map2img, n_img, out,
                                validate, pix_inp=(ohw[0] // 2) * (ohw[1] // 2) if pool == 2 else None)
    d = _lib.ConvGeomAbDesc(base, ptr(_dev(q2)), scale, scale2, kr)
    name = "conv_geom_ab" + ("" if q2 is None else "_dual") + ("_b6" if b6 else "") + ("_pool" if pool == 2 else "")
    _count(name, _lib.GEOM_BWD)
    lib = _lib.load()
    if pool == 2:
        dp = _lib.ConvGeomAbPoolDesc(d, 2)
        check((lib.lrpx_conv_geom_ab_pool_b6 if b6 else lib.lrpx_conv_geom_ab_pool)(C.byref(dp), stream_ptr()))
        return out
    check((lib.lrpx_conv_geom_ab_b6 if b6 else lib.lrpx_conv_geom_ab)(C.byref(d), stream_ptr()))
    return out


def vgg16_ab_coef(zz, qp, qn, n_img, ohw, c, xpool=None):
    """`lrpx_vgg16_ab_coef`: zz (n_img, OH OW, 2c) = [Z+ | Z-] -> qp, qn (n_img, OH OW, c) = win / safe(Z+), win / safe(Z-); xpool
    (n_img, OH OW, c), the input of the 2x2 max-pool above the conv: win = 1 at each window's first non-zero maximum, 0 elsewhere
    (None: win = 1).  The per-image coefficients of `conv_geom_ab` on VGG16."""
    pix = ohw[0] * ohw[1]
    for name, t, ch in (("zz", zz, 2 * c), ("qp", qp, c), ("qn", qn, c), ("xpool", xpool, c)):
        if t is not None and (_dev(t).numel() != n_img * pix * ch or not t.is_contiguous() or t.dtype != torch.float32):
            raise ValueError("vgg16_ab_coef: {} must be contiguous fp32 of n_img x OH OW x {} = {} x {} x {}".format(name, ch, n_img, pix, ch))
    _count("vgg16_ab_coef")
    check(_lib.load().lrpx_vgg16_ab_coef(ptr(zz), ptr(xpool), ptr(qp), ptr(qn), n_img, ohw[0], ohw[1], c, stream_ptr()))


def conv_geom_grad(inp, wpacked, n, hw, ohw, geom, k, n_oc, mask=None, scale=None, clamp=False, addend=None, map2img=None, n_img=None,
                   out=None, validate=True, b6=False):
    """`lrpx_conv_geom_grad` (b6: `lrpx_conv_geom_grad_b6`): the transposed direction for the gradient chain (include/lrpx.h, DESIGN.md
    5.12).  inp (n maps, OH OW, k) -> out (n, H W, n_oc) = convT(scale * (mask[img] > 0 ? (clamp ? max(inp, 0) : inp) : 0), W) + addend
    with wpacked the transposed pack of the RAW weights; mask (n_img, OH OW, k), scale (k,), addend like out, each optional.
    LAUNCHES counts it under 'conv_geom_grad' (b6: 'conv_geom_grad_b6')."""
    base, out = _conv_geom_desc("conv_geom_grad", _lib.GEOM_BWD, inp, wpacked, n, hw, ohw, geom, k, n_oc, k, "k",
                                (("mask", mask, "q", False), ("scale", scale, "k", False)), None, None, None, addend, map2img, n_img, out,
                                validate)
    d = _lib.ConvGeomGradDesc(base, ptr(_dev(mask)), ptr(_dev(scale)), 1 if clamp else 0)
    _count("conv_geom_grad_b6" if b6 else "conv_geom_grad", _lib.GEOM_BWD)
    lib = _lib.load()
    check((lib.lrpx_conv_geom_grad_b6 if b6 else lib.lrpx_conv_geom_grad)(C.byref(d), stream_ptr()))
    return out


def conv_geom_grad_b6(*args, **kw):
    """`conv_geom_grad` in the exact bf16-split arithmetic (wpacked from `conv_geom_pack_bf16x3`)"""
    return conv_geom_grad(*args, b6=True, **kw)


def resnet_relu_grad(g, act, map2img, out, n_maps, n_img, clamp):
    """out = (clamp ? max(g, 0) : g) * (act[img] > 0): ReLU backward at a block's output (include/lrpx.h)"""
    _count("resnet_relu_grad")
    check(_lib.load().lrpx_resnet_relu_grad(ptr(_dev(g)), ptr(_dev(act)), ptr(map2img), ptr(_dev(out)), n_maps, n_img, g.numel() // n_maps,
                                            1 if clamp else 0, stream_ptr()))


def resnet_maxpool_grad(x, g_out, map2img, g_in, n_maps, n_img, hw, ohw, c, win):
    """MaxPool2d backward on NHWC: each window's gradient to its first maximum (include/lrpx.h)"""
    _count("resnet_maxpool_grad")
    check(_lib.load().lrpx_resnet_maxpool_grad(ptr(_dev(x)), ptr(_dev(g_out)), ptr(map2img), ptr(_dev(g_in)), n_maps, n_img, hw[0], hw[1],
                                               ohw[0], ohw[1], c, *win, stream_ptr()))


def resnet_bn_act_coef(yz, w, b, act, q, relu):
    """yz (n, pix, 2c) = [conv output | Z of its rule] -> act = BN affine (+ ReLU), q = the conv's relevance coefficient (include/lrpx.h)"""
    c = w.shape[0]
    _count("resnet_bn_act_coef")
    check(_lib.load().lrpx_resnet_bn_act_coef(ptr(_dev(yz)), yz.shape[-1], ptr(_dev(w)), ptr(_dev(b)), ptr(_dev(act)), ptr(_dev(q)),
                                              yz.numel() // yz.shape[-1], c, 1 if relu else 0, stream_ptr()))


def resnet_coef_neg(yz, w, b, qn):
    """yz (n, pix, 2c) = [conv output | Z- of the general rule] -> qn, the second coefficient of `conv_geom_ab` (include/lrpx.h)"""
    _count("resnet_coef_neg")
    check(_lib.load().lrpx_resnet_coef_neg(ptr(_dev(yz)), yz.shape[-1], ptr(_dev(w)), ptr(_dev(b)), ptr(_dev(qn)),
                                           yz.numel() // yz.shape[-1], w.shape[0], stream_ptr()))


def resnet_add_relu_coef(x1, x2, out, c1, c2):
    _count("resnet_add_relu_coef")
    check(_lib.load().lrpx_resnet_add_relu_coef(ptr(_dev(x1)), ptr(_dev(x2)), ptr(_dev(out)), ptr(_dev(c1)), ptr(_dev(c2)), x1.numel(),
                                                stream_ptr()))


def resnet_maxpool_fwd(x, y, n, hw, ohw, c, win):
    _count("resnet_maxpool_fwd")
    check(_lib.load().lrpx_resnet_maxpool_fwd(ptr(_dev(x)), ptr(_dev(y)), n, hw[0], hw[1], ohw[0], ohw[1], c, *win, stream_ptr()))


def resnet_maxpool_rel(x, r_out, map2img, r_in, n_maps, n_img, hw, ohw, c, win):
    _count("resnet_maxpool_rel")
    check(_lib.load().lrpx_resnet_maxpool_rel(ptr(_dev(x)), ptr(_dev(r_out)), ptr(map2img), ptr(_dev(r_in)), n_maps, n_img, hw[0], hw[1],
                                              ohw[0], ohw[1], c, *win, stream_ptr()))


def resnet_add_split(r, c1, c2, map2img, r1, r2, n_maps, n_img):
    _count("resnet_add_split")
    check(_lib.load().lrpx_resnet_add_split(ptr(_dev(r)), ptr(_dev(c1)), ptr(_dev(c2)), ptr(map2img), ptr(_dev(r1)), ptr(_dev(r2)), n_maps,
                                            n_img, r.numel() // n_maps, stream_ptr()))


def resnet_stem_fold(r_split, out, n_maps, cin, half, ld, pix):
    _count("resnet_stem_fold")
    check(_lib.load().lrpx_resnet_stem_fold(ptr(_dev(r_split)), ptr(_dev(out)), n_maps, cin, half, ld, pix, stream_ptr()))


def _pair(v):
    return tuple(int(a) for a in v) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _conv_out(size, k, s, p):
    return (size + 2 * p - k) // s + 1


class ResNetPlan(object):
    """What `match_bottleneck_resnet` found.  `convs`: one dict per conv in forward order - name, module, bn, cin, cout, geom = (kh, kw,
    sh, sw, ph, pw), producer ('image' | 'maxpool(relu)' | 'relu') and nonneg = the producer is a ReLU or the pool of a ReLU (all but the
    stem: what licenses K = cin and W+ alone).  `blocks`: one dict per bottleneck block - name, conv1 / conv2 / conv3 / downsample (indices
    into `convs`, downsample None for an identity shortcut).  `pool` = (kh, kw, sh, sw, ph, pw) of the stem's MaxPool2d."""

    def __init__(self, convs, blocks, pool):
        self.convs, self.blocks, self.pool = convs, blocks, pool


def match_bottleneck_resnet(model):
    """Recognise a bottleneck ResNet by STRUCTURE (not by class): direct children Conv2d -> BatchNorm2d -> ReLU -> MaxPool2d (the stem,
    models/resnet.py:164-168), then nn.Sequential containers (`layer1..layer4` or one `layers`) of blocks with conv1 / bn1 / conv2 / bn2 /
    conv3 / bn3 / relu / add members and an optional downsample = Sequential(Conv2d, BatchNorm2d) (:93-140); an AdaptiveAvgPool2d / Linear
    head the forward never calls may follow (:176-177).  Returns a `ResNetPlan`; ValueError naming the reason otherwise.  The
    non-negativity of every conv input but the stem's follows from this structure - its producer is the ReLU member or the pool behind
    the stem's ReLU - never from data.  Host logic: no device."""
    import torch.nn as nn

    def fail(msg):
        raise ValueError("not a bottleneck ResNet the engine runs: " + msg)
    kids = list(model.named_children())
    stem_types = (nn.Conv2d, nn.BatchNorm2d, nn.ReLU, nn.MaxPool2d)
    if len(kids) < 5 or not all(isinstance(kids[i][1], t) for i, t in enumerate(stem_types)):
        fail("the stem must be Conv2d -> BatchNorm2d -> ReLU -> MaxPool2d followed by containers of blocks, got " +
             ", ".join(type(m).__name__ for _, m in kids[:5]))

    def conv_entry(name, conv, bn, producer):
        if not isinstance(conv, nn.Conv2d) or not isinstance(bn, nn.BatchNorm2d):
            fail("{}: a Conv2d followed by a BatchNorm2d, got {} / {}".format(name, type(conv).__name__, type(bn).__name__))
        if _pair(conv.dilation) != (1, 1):
            fail("{}: dilation {} is not supported".format(name, conv.dilation))
        if conv.groups != 1:
            fail("{}: groups={} is not supported".format(name, conv.groups))
        if conv.bias is not None:
            fail("{}: a conv with bias is not supported (the preset ignores it, the trace would not)".format(name))
        if isinstance(conv.padding, str) or conv.padding_mode != "zeros":
            fail("{}: padding {!r} / padding_mode {!r} is not supported".format(name, conv.padding, conv.padding_mode))
        if bn.training:
            fail("{}: its BatchNorm2d is in training mode (call .eval(): the rule uses the running statistics)".format(name))
        if bn.running_mean is None or bn.running_var is None or not bn.affine:
            fail("{}: its BatchNorm2d has no running statistics / affine parameters".format(name))
        if bn.num_features != conv.out_channels:
            fail("{}: BatchNorm2d({}) after {} output channels".format(name, bn.num_features, conv.out_channels))
        if conv.out_channels % 4:
            fail("{}: {} output channels - the engine reads channels in fours".format(name, conv.out_channels))
        geom = _pair(conv.kernel_size) + _pair(conv.stride) + _pair(conv.padding)
        return dict(name=name, module=conv, bn=bn, cin=conv.in_channels, cout=conv.out_channels, geom=geom, producer=producer,
                    nonneg=producer in ("relu", "maxpool(relu)"))

    pool = kids[3][1]
    if _pair(pool.dilation) != (1, 1) or pool.ceil_mode:
        fail("{}: MaxPool2d with dilation / ceil_mode is not supported".format(kids[3][0]))
    pk, ps, pp = _pair(pool.kernel_size), _pair(pool.stride if pool.stride is not None else pool.kernel_size), _pair(pool.padding)
    convs = [conv_entry(kids[0][0], kids[0][1], kids[1][1], "image")]
    blocks = []
    cin = convs[0]["cout"]
    producer = "maxpool(relu)"
    head = False
    for cname, cont in kids[4:]:
        if isinstance(cont, (nn.AdaptiveAvgPool2d, nn.Linear)):
            head = True
            continue
        if head or not isinstance(cont, nn.Sequential) or len(cont) == 0:
            fail("{}: expected a Sequential of bottleneck blocks (or the unused AdaptiveAvgPool2d / Linear head), got {}".format(
                cname, type(cont).__name__))
        for bname, blk in cont.named_children():
            name = "{}.{}".format(cname, bname)
            get = lambda a: getattr(blk, a, None)
            if not all(isinstance(get(a), nn.Module) for a in ("conv1", "bn1", "conv2", "bn2")):
                fail("{}: not a residual block (no conv1 / bn1 / conv2 / bn2 members)".format(name))
            if get("conv3") is None or get("bn3") is None:
                fail("{}: a BasicBlock (two convs, no conv3 / bn3) - only bottleneck blocks are supported; BasicBlock nets also build "
                     "their Add inside forward (models/resnet.py:87)".format(name))
            if not isinstance(get("relu"), nn.ReLU):
                fail("{}: no `relu` member of type nn.ReLU".format(name))
            if not isinstance(get("add"), nn.Module):
                fail("{}: no registered `add` module (models/resnet.py:118)".format(name))
            i0 = len(convs)
            convs.append(conv_entry(name + ".conv1", blk.conv1, blk.bn1, producer))
            convs.append(conv_entry(name + ".conv2", blk.conv2, blk.bn2, "relu"))
            convs.append(conv_entry(name + ".conv3", blk.conv3, blk.bn3, "relu"))
            down = None
            ds = get("downsample")
            if ds is not None:
                if not (isinstance(ds, nn.Sequential) and len(ds) == 2):
                    fail("{}.downsample: expected Sequential(Conv2d, BatchNorm2d)".format(name))
                down = len(convs)
                convs.append(conv_entry(name + ".downsample.0", ds[0], ds[1], producer))
            chain = [(convs[i0], cin), (convs[i0 + 1], convs[i0]["cout"]), (convs[i0 + 2], convs[i0 + 1]["cout"])]
            if down is not None:
                chain.append((convs[down], cin))
            for cv, want in chain:
                if cv["cin"] != want:
                    fail("{}: {} input channels where its producer has {}".format(cv["name"], cv["cin"], want))
            cout = convs[i0 + 2]["cout"]
            if down is not None and convs[down]["cout"] != cout:
                fail("{}: the shortcut has {} channels, the residual branch {}".format(name, convs[down]["cout"], cout))
            if down is None and (cin != cout or any(cv["geom"][2:4] != (1, 1) for cv in convs[i0:i0 + 3])):
                fail("{}: an identity shortcut needs equal channels and stride 1".format(name))
            blocks.append(dict(name=name, conv1=i0, conv2=i0 + 1, conv3=i0 + 2, downsample=down))
            cin, producer = cout, "relu"
    if not blocks:
        fail("no bottleneck blocks found")
    if 2 * convs[0]["cin"] > 8:
        fail("{}: {} image channels (at most 4)".format(convs[0]["name"], convs[0]["cin"]))
    return ResNetPlan(convs, blocks, pk + ps + pp)


def bottleneck_resnet_from_state(sd, prefix=""):
    """A bottleneck ResNet module from a checkpoint's tensors alone: the keys of models/resnet.py (ResNet + Bottleneck, :93-236) under
    `prefix` - conv1.weight, bn1.{weight, bias, running_mean, running_var}, layerN.M.conv1..3.weight, layerN.M.bn1..3.*,
    layerN.M.downsample.0.weight / .downsample.1.* - as torch tensors or numpy arrays.  Widths and block counts are read from the
    tensor shapes; what a state dict does not hold is that file's: the stem conv has stride 2 and padding (k - 1) / 2 (:164), the pool
    is MaxPool2d(3, 2, 1) (:168), a block's middle conv has padding (k - 1) / 2, and the first block of layer2 and later has stride 2
    on its middle conv and its shortcut (:111, :205 - the ResNet V1.5 placement).  The class's unused `fc.*` head (:177) and the
    BatchNorms' `num_batches_tracked` are ignored; any other key under the prefix, a missing tensor or a shape that does not fit
    raises ValueError naming the key.  The result is in eval mode, on the CPU, with an explicit `add` member per block:
    `match_bottleneck_resnet` accepts it, `.to(device)` makes it a `ResNetEncoder`'s module.  Host logic: no device."""
    import re
    import numpy as np
    import torch.nn as nn

    def fail(key, msg):
        raise ValueError("bottleneck_resnet_from_state: {!r}: {}".format(prefix + key, msg))
    own = {}
    for k, v in sd.items():
        if not k.startswith(prefix):
            continue
        k = k[len(prefix):]
        if k.startswith("fc.") or k.endswith("num_batches_tracked"):
            continue
        v = torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v
        own[k] = v.detach().to(device="cpu", dtype=torch.float32).clone()
    used = set()

    def take(key, shape=None, dim=None):
        if key not in own:
            fail(key, "missing")
        t = own[key]
        if dim is not None and t.dim() != dim:
            fail(key, "expected a {}-d tensor, got shape {}".format(dim, tuple(t.shape)))
        if shape is not None and tuple(t.shape) != tuple(shape):
            fail(key, "expected shape {}, got {}".format(tuple(shape), tuple(t.shape)))
        used.add(key)
        return t

    def conv(name, cin, stride, cout=None, k=None):
        w = take(name + ".weight", dim=4)
        if w.shape[1] != cin or (cout is not None and w.shape[0] != cout) or w.shape[2] != w.shape[3] or w.shape[2] % 2 == 0 or \
                (k is not None and w.shape[2] != k):
            fail(name + ".weight", "shape {} does not fit ({} input channels{}{}, a square odd kernel)".format(
                tuple(w.shape), cin, "" if cout is None else ", {} output channels".format(cout), "" if k is None else ", {0}x{0}".format(k)))
        m = nn.Conv2d(cin, w.shape[0], w.shape[2], stride=stride, padding=(w.shape[2] - 1) // 2, bias=False)
        m.weight.data = w
        return m

    def bn(name, c):
        m = nn.BatchNorm2d(c)
        m.weight.data, m.bias.data = take(name + ".weight", (c,)), take(name + ".bias", (c,))
        m.running_mean, m.running_var = take(name + ".running_mean", (c,)), take(name + ".running_var", (c,))
        return m

    class Add(nn.Module):                  # the explicit residual sum (models/resnet.py:32-37)
        def forward(self, x, y):
            return x + y

    class Bottleneck(nn.Module):
        def __init__(self, name, cin, stride):
            super().__init__()
            self.conv1 = conv(name + ".conv1", cin, 1, k=1)
            width = self.conv1.out_channels
            self.bn1 = bn(name + ".bn1", width)
            self.conv2 = conv(name + ".conv2", width, stride, cout=width)
            self.bn2 = bn(name + ".bn2", width)
            self.conv3 = conv(name + ".conv3", width, 1, k=1)
            cout = self.conv3.out_channels
            self.bn3 = bn(name + ".bn3", cout)
            self.relu = nn.ReLU(inplace=True)
            self.downsample = None
            if name + ".downsample.0.weight" in own:
                self.downsample = nn.Sequential(conv(name + ".downsample.0", cin, stride, cout=cout, k=1), bn(name + ".downsample.1", cout))
            elif stride != 1 or cin != cout:
                fail(name + ".downsample.0.weight", "missing (the block changes {} channels into {} with stride {})".format(cin, cout, stride))
            self.add = Add()

        def forward(self, x):
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
            identity = x if self.downsample is None else self.downsample(x)
            return self.relu(self.add(out, identity))

    class BottleneckResNet(nn.Module):
        def __init__(self):
            super().__init__()
            if "conv1.weight" not in own:
                fail("conv1.weight", "missing")
            self.conv1 = conv("conv1", own["conv1.weight"].shape[1] if own["conv1.weight"].dim() == 4 else 0, 2)
            self.bn1 = bn("bn1", self.conv1.out_channels)
            self.relu = nn.ReLU(inplace=True)
            self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
            counts = {}
            for k in own:
                m = re.match(r"layer(\d+)\.(\d+)\.", k)
                if m:
                    counts.setdefault(int(m.group(1)), set()).add(int(m.group(2)))
            if not counts:
                fail("layer1.0.conv1.weight", "missing (no layerN.M.* keys)")
            cin = self.conv1.out_channels
            self.layer_names = []
            for n in range(1, max(counts) + 1):
                if n not in counts or sorted(counts[n]) != list(range(len(counts[n]))):
                    fail("layer{}.{}.conv1.weight".format(n, 0 if n not in counts else min(set(range(len(counts[n]) + 1)) - counts[n])),
                         "missing (layers and blocks are numbered without gaps)")
                blocks = []
                for b in range(len(counts[n])):
                    blocks.append(Bottleneck("layer{}.{}".format(n, b), cin, 2 if (b == 0 and n > 1) else 1))
                    cin = blocks[-1].conv3.out_channels
                setattr(self, "layer{}".format(n), nn.Sequential(*blocks))
                self.layer_names.append("layer{}".format(n))
            self.feat_dim = cin

        def forward(self, x):
            x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
            for n in self.layer_names:
                x = getattr(self, n)(x)
            return x

    net = BottleneckResNet()
    for k in own:
        if k not in used:
            fail(k, "not a key of a bottleneck ResNet (conv1, bn1, layerN.M.conv1..3 / bn1..3 / downsample.0 / downsample.1)")
    return net.eval()


class ResNetEncoder:
    """The reference's bottleneck ResNet encoders (models/resnet.py resnet50 / resnet101, any `layers`) as a device-resident, batched LRP
    engine in the pattern of `Vgg16`: `forward` traces B images once - activations and, per conv, the relevance coefficient q that folds
    the BatchNorm rule and the division by Z+ (per Add, its two split coefficients) - and `relevance` turns n_maps relevance tensors at
    the feature map into image-sized maps, each on the trace of image map2img[m], as a chain of transposed convs (`lrpx_conv_geom_ex`,
    K = cout, W+ only) with NHWC tensors throughout.  The preset only: alpha 1, beta 0, ignore_bias, BatchNorm epsilon rule, ReLU
    identity, winner-take-all pool (lrp_wrapper.py:7-12,42-56).  DESIGN.md 5.8.
    conv_mode: the arithmetic of every contraction of the trace and of the maps - 0: fp32 MFMA (`lrpx_conv_geom_ex`); 1: the exact
    bf16 split, six plane products on the bf16 MFMA (`lrpx_conv_geom_ex_b6`).  The engine's own choice: it does not
    follow `lrpx_set_conv_mode`.  `replica()` shares packs and mode.
    `relevance_alpha_beta` runs the general alpha-beta rule on the same trace, in either mode.
    `gradient` / `guided_backprop` run the autograd chain and guided backprop on the same trace, in either mode."""

    CONV_MODES = (0, 1)

    def __init__(self, module, conv_mode=0):
        if isinstance(conv_mode, bool) or conv_mode not in self.CONV_MODES:
            raise ValueError("ResNetEncoder: conv_mode {!r}: this engine has modes 0 (fp32 MFMA) and 1 (exact bf16 split); the f16 "
                             "modes 2 / 3 are not built at these geometries".format(conv_mode))
        self.conv_mode = conv_mode
        self.b6 = conv_mode == 1
        pack = conv_geom_pack_bf16x3 if self.b6 else conv_geom_pack
        plan = match_bottleneck_resnet(module)
        tensors = list(module.parameters()) + list(module.buffers())
        if not tensors or any(t.device.type != "cuda" for t in tensors):
            raise ValueError("ResNetEncoder: the model must live on the GPU (no CPU path)")
        self.device = tensors[0].device
        self.plan = plan
        self.cin = plan.convs[0]["cin"]
        self.c2 = 8                                   # the split image [x+ | x- | 0..] (lrpx_nchw_to_nhwc_posneg)
        self.packs = []
        relu = {0} | {blk[k] for blk in plan.blocks for k in ("conv1", "conv2")}       # the convs whose BatchNorm a ReLU follows
        for i, cv in enumerate(plan.convs):
            wt = cv["module"].weight.detach().to(torch.float32)
            bn = cv["bn"]
            sd = torch.sqrt(bn.running_var.detach().float() + bn.eps)
            w = (bn.weight.detach().float() / sd).contiguous()                                       # lrp_modules.py:210
            b = (bn.bias.detach().float() - (bn.running_mean.detach().float() * bn.weight.detach().float()) / sd).contiguous()   # :211
            wpos = wt.clamp(min=0)
            if cv["nonneg"]:            # x >= 0: Z+ = conv(x, W+), K = cin;  columns [W | W+] share one gather of the input tile
                fwd = pack(torch.cat([wt, wpos], 0), _lib.GEOM_FWD)
                bwd = pack(wpos, _lib.GEOM_BWD)
                k_in = cv["cin"]
            else:                       # the stem on the split image: y = [x+ | x-] [W | W], Z = [x+ | x-] [W+ | W-]  (lrp_modules.py:81-84)
                pad = torch.zeros(wt.shape[0], self.c2 - 2 * self.cin, *wt.shape[2:], device=self.device)
                zrow = torch.cat([wpos, wt.clamp(max=0), pad], 1)
                fwd = pack(torch.cat([torch.cat([wt, wt, pad], 1), zrow], 0), _lib.GEOM_FWD)
                bwd = pack(zrow, _lib.GEOM_BWD)
                k_in = self.c2
            self.packs.append(dict(fwd=fwd, bwd=bwd, w=w, b=b, k_in=k_in, cout=cv["cout"], geom=cv["geom"], relu=i in relu))
        self._ab_packs = []                           # the general rule's packs, built at its first call; replicas share the list
        self._grad_packs = []                         # the gradient chain's raw-W transposed packs, likewise
        torch.cuda.current_stream().synchronize()
        self._reset()

    def _reset(self):
        self.trace, self.shape, self._ws, self.n_img = None, None, {}, 0
        self._serial, self._qn, self._qn_serial = 0, None, -1

    def replica(self):
        """Same packed weights, own trace / workspace buffers (for a second batch in flight on another stream)."""
        import copy
        r = copy.copy(self)
        r._reset()
        return r

    # ---- shapes ------------------------------------------------------------------------------------------------------------------------
    def _layout(self, H, W):
        """[(hw_in, hw_out)] per conv, the pool's (hw_in, hw_out) and the feature map's size for an H x W image; ValueError where a
        window does not fit or a block's two branches disagree"""
        convs, dims = self.plan.convs, [None] * len(self.plan.convs)

        def out_of(i, hw):
            kh, kw, sh, sw, ph, pw = convs[i]["geom"]
            if hw[0] + 2 * ph < kh or hw[1] + 2 * pw < kw:
                raise ValueError("ResNetEncoder: {}: the {}x{} kernel does not fit its {}x{} input".format(convs[i]["name"], kh, kw, *hw))
            dims[i] = (hw, (_conv_out(hw[0], kh, sh, ph), _conv_out(hw[1], kw, sw, pw)))
            return dims[i][1]
        hw = out_of(0, (H, W))
        kh, kw, sh, sw, ph, pw = self.plan.pool
        if hw[0] + 2 * ph < kh or hw[1] + 2 * pw < kw:
            raise ValueError("ResNetEncoder: the image is too small for the stem's pool")
        pool = (hw, (_conv_out(hw[0], kh, sh, ph), _conv_out(hw[1], kw, sw, pw)))
        hw = pool[1]
        for blk in self.plan.blocks:
            o = out_of(blk["conv3"], out_of(blk["conv2"], out_of(blk["conv1"], hw)))
            short = out_of(blk["downsample"], hw) if blk["downsample"] is not None else hw
            if short != o:
                raise ValueError("ResNetEncoder: {}: the residual branch gives {}x{}, the shortcut {}x{}".format(blk["name"], *o, *short))
            hw = o
        return dims, pool, hw

    def feature_shape(self, H, W):
        """(h, w, C) of the feature map of an H x W image (host arithmetic; ValueError where a window does not fit)"""
        return tuple(self._layout(H, W)[2]) + (self.packs[self.plan.blocks[-1]["conv3"]]["cout"],)

    def trace_bytes(self, B, H, W, alpha_beta=False):
        """bytes of the trace `forward` keeps for B images of H x W pixels (activations, q per conv, c1 / c2 per Add); alpha_beta: plus
        the second coefficient per conv that `relevance_alpha_beta` keeps beside it"""
        dims, pool, _ = self._layout(H, W)
        f = H * W * self.c2 + pool[1][0] * pool[1][1] * self.packs[0]["cout"]
        for i, pk in enumerate(self.packs):
            f += (3 if alpha_beta else 2) * dims[i][1][0] * dims[i][1][1] * pk["cout"]    # act + q (+ qn)
        for blk in self.plan.blocks:
            o = dims[blk["conv3"]][1]
            f += 3 * o[0] * o[1] * self.packs[blk["conv3"]]["cout"]                # the block's output, c1, c2
        return 4 * B * f

    # ---- trace ---------------------------------------------------------------------------------------------------------------------------
    def forward(self, img_nchw, layer_ms=None):
        """(B, cin, H, W) -> the feature map (B, h w, C) NHWC (a view into the trace).  Everything `relevance` needs from the images is
        computed here, once per image.  layer_ms: a dict - the call then adds each conv's milliseconds under its name (HIP events)."""
        img = _dev(img_nchw).detach().to(torch.float32).contiguous()
        if img.dim() != 4 or img.shape[1] != self.cin:
            raise ValueError("ResNetEncoder.forward: images must be (B, {}, H, W)".format(self.cin))
        B, _, H, W = img.shape
        dims, pool, feat_hw = self._layout(H, W)
        dev = self.device
        new = lambda pix, c: torch.empty(B, pix[0] * pix[1], c, dtype=torch.float32, device=dev)
        if self.shape != (B, H, W):
            t = {"xs": new((H, W), self.c2), "act": [], "q": [], "out": [], "c1": [], "c2": []}
            for i, pk in enumerate(self.packs):
                t["act"].append(new(dims[i][1], pk["cout"]))
                t["q"].append(new(dims[i][1], pk["cout"]))
            t["pool"] = new(pool[1], self.packs[0]["cout"])
            for blk in self.plan.blocks:
                for k in ("out", "c1", "c2"):
                    t[k].append(new(dims[blk["conv3"]][1], self.packs[blk["conv3"]]["cout"]))
            yz = max(2 * pk["cout"] * dims[i][1][0] * dims[i][1][1] for i, pk in enumerate(self.packs))
            t["yz"] = torch.empty(B * yz, dtype=torch.float32, device=dev)
            self.trace, self.shape, self._ws = t, (B, H, W), {}
            self.dims, self.pool_dims, self.feat_hw = dims, pool, feat_hw
        t = self.trace
        self.n_img = B
        self._serial += 1
        lib = _lib.load()
        check(lib.lrpx_nchw_to_nhwc_posneg(ptr(img), ptr(t["xs"]), B, self.cin, H * W, self.c2, stream_ptr()))

        def conv(i, x, relu):
            pk = self.packs[i]
            ev = _events(layer_ms)
            hw, ohw = dims[i]
            yz = t["yz"][: B * ohw[0] * ohw[1] * 2 * pk["cout"]].view(B, ohw[0] * ohw[1], 2 * pk["cout"])
            conv_geom_ex(x, pk["fwd"], _lib.GEOM_FWD, B, hw, ohw, pk["geom"], pk["k_in"], 2 * pk["cout"], out=yz, b6=self.b6)
            resnet_bn_act_coef(yz, pk["w"], pk["b"], t["act"][i], t["q"][i], relu)
            _events_done(ev, layer_ms, self.plan.convs[i]["name"])
            return t["act"][i]
        a = conv(0, t["xs"], True)
        resnet_maxpool_fwd(a, t["pool"], B, pool[0], pool[1], self.packs[0]["cout"], self.plan.pool)
        x = t["pool"]
        for bi, blk in enumerate(self.plan.blocks):
            y3 = conv(blk["conv3"], conv(blk["conv2"], conv(blk["conv1"], x, True), True), False)
            short = conv(blk["downsample"], x, False) if blk["downsample"] is not None else x
            resnet_add_relu_coef(y3, short, t["out"][bi], t["c1"][bi], t["c2"][bi])
            x = t["out"][bi]
        return x

    # ---- relevance ---------------------------------------------------------------------------------------------------------------------
    def _map_args(self, fn, feat, name, map2img, out):
        """The per-map arguments of the public pass `fn`, checked once, before anything is launched: -> (the tensor `name` at the feature
        map, contiguous; map2img validated on the host, or None; out, allocated if None; n_maps).  ValueError / LrpxError otherwise."""
        if self.trace is None:
            raise ValueError("ResNetEncoder.{}: no trace - call forward() first".format(fn))
        B = self.n_img
        r = _dev(feat)
        c_feat = self.packs[self.plan.blocks[-1]["conv3"]]["cout"]
        if r.dim() != 3 or tuple(r.shape[1:]) != (self.feat_hw[0] * self.feat_hw[1], c_feat) or r.dtype != torch.float32:
            raise ValueError("ResNetEncoder.{}: {} must be float32 (n_maps, {}, {}), got {}".format(
                fn, name, self.feat_hw[0] * self.feat_hw[1], c_feat, tuple(r.shape)))
        n_maps = r.shape[0]
        if n_maps == 0:
            raise ValueError("ResNetEncoder.{}: no maps".format(fn))
        if map2img is None:
            if n_maps != B:
                raise ValueError("ResNetEncoder.{}: without map2img there is one map per image of the trace ({} maps, {} images)"
                                 .format(fn, n_maps, B))
        else:
            map2img = check_map2img(map2img, n_maps, B)
        H, W = self.shape[1], self.shape[2]
        if out is None:
            out = torch.empty(n_maps, self.cin, H, W, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (n_maps, self.cin, H, W) or not out.is_contiguous():
            raise ValueError("ResNetEncoder.{}: out must be contiguous (n_maps, {}, {}, {})".format(fn, self.cin, H, W))
        return r.contiguous(), map2img, out, n_maps

    def _walk(self, r, map2img, out, n_maps, layer_ms, head, convT, pool, stem_c, tail):
        """One per-map pass down the trace, from `r` (n_maps, h w, C) at the feature map to `out`: per block, last first, the head, then
        conv3 -> ws a, conv2 -> ws b, the downsample (if any) -> ws a, conv1 with the shortcut's term as addend -> ws r[cur] (ping-pong);
        then the pool step -> ws a, the stem's conv -> ws b on `stem_c` channels, and the tail into `out`.  What a pass brings:
          head(bi, r, ws) -> (conv3's input, the shortcut's term) at block bi's output, in ws r1 / r2
          convT(i, inp, x, addend, o, n_oc): the transposed conv of conv i, o = f(inp, x) + addend on n_oc channels, x the trace's
            tensor at the conv's input
          pool: `resnet_maxpool_rel` or `resnet_maxpool_grad`;  tail(rs, out): the stem conv's result into the NCHW result
        layer_ms: as in `forward`, around every conv."""
        t, dims, blocks, B = self.trace, self.dims, self.plan.blocks, self.n_img
        ws = self._workspace(n_maps)

        def conv(i, inp, x, addend, dst, n_oc):
            hw = dims[i][0]
            o = dst[: n_maps * hw[0] * hw[1] * n_oc].view(n_maps, hw[0] * hw[1], n_oc)
            if layer_ms is None:
                convT(i, inp, x, addend, o, n_oc)
            else:
                ev = _events(layer_ms)
                convT(i, inp, x, addend, o, n_oc)
                _events_done(ev, layer_ms, self.plan.convs[i]["name"])
            return o
        cur = 0
        for bi in range(len(blocks) - 1, -1, -1):
            blk = blocks[bi]
            x = t["out"][bi - 1] if bi > 0 else t["pool"]
            x2, x1 = t["act"][blk["conv2"]], t["act"][blk["conv1"]]
            r1, r2 = head(bi, r, ws)
            ra = conv(blk["conv3"], r1, x2, None, ws["a"], x2.shape[2])
            rb = conv(blk["conv2"], ra, x1, None, ws["b"], x1.shape[2])
            if blk["downsample"] is not None:
                r2 = conv(blk["downsample"], r2, x, None, ws["a"], x.shape[2])
            r = conv(blk["conv1"], rb, x, r2, ws["r"][cur], x.shape[2])
            cur = 1 - cur
        a0 = t["act"][0]
        rp = ws["a"][: n_maps * a0[0].numel()].view(n_maps, *a0.shape[1:])
        pool(a0, r, map2img, rp, n_maps, B, self.pool_dims[0], self.pool_dims[1], self.packs[0]["cout"], self.plan.pool)
        tail(conv(0, rp, t["xs"], None, ws["b"], stem_c), out)
        return out

    def _walk_lrp(self, r, map2img, out, n_maps, layer_ms, convT):
        """`_walk` with the LRP rules around the convs: the Add split, the pool rule, the stem's split image and its fold"""
        t, B = self.trace, self.n_img

        def head(bi, r, ws):
            r1 = ws["r1"][: r.numel()].view(r.shape)
            r2 = ws["r2"][: r.numel()].view(r.shape)
            resnet_add_split(r, t["c1"][bi], t["c2"][bi], map2img, r1, r2, n_maps, B)
            return r1, r2
        pix = self.shape[1] * self.shape[2]
        return self._walk(r, map2img, out, n_maps, layer_ms, head, convT, resnet_maxpool_rel, self.c2,
                          lambda rs, o: resnet_stem_fold(rs, o, n_maps, self.cin, self.cin, self.c2, pix))

    def relevance(self, r_feat_nhwc, map2img=None, out=None, layer_ms=None):
        """compute_lrp (LRPtools/lrp_wrapper.py:63-87) for n_maps maps: (n_maps, h w, C) relevance at the feature map -> (n_maps, cin, H, W);
        map m runs on the trace of image map2img[m] (int32 on the device; None: n_maps == B, map m on image m).  No forward work: the
        pass is one Add split and three or four transposed convs per block, the pool gather, the stem's transposed conv and the fold.
        layer_ms: as in `forward`."""
        r, map2img, out, n_maps = self._map_args("relevance", r_feat_nhwc, "r_feat_nhwc", map2img, out)
        t, dims, packs, B, b6 = self.trace, self.dims, self.packs, self.n_img, self.b6

        def convT(i, r_out, x, addend, o, n_oc):
            pk = packs[i]
            hw, ohw = dims[i]
            conv_geom_ex(r_out, pk["bwd"], _lib.GEOM_BWD, n_maps, hw, ohw, pk["geom"], pk["cout"], n_oc, x=x, q=t["q"][i], addend=addend,
                         map2img=map2img, n_img=B, out=o, validate=False, b6=b6)
        return self._walk_lrp(r, map2img, out, n_maps, layer_ms, convT)

    # ---- the general alpha-beta rule -------------------------------------------------------------------------------
    def _ab_state(self):
        """per conv: `fwd`, the forward pack of the columns [W | W-] (the stem on the split image: Z- = x+ W- + x- W+, row block
        [W- | W+ | pad]) and `bwd`, the transposed pack of the stacked rows [W+ ; W-] (the stem: [W+ | W- | pad ; W- | W+ | pad]).
        Built once per engine from the model's weights, at the first alpha-beta call."""
        if not self._ab_packs:
            pack = conv_geom_pack_bf16x3 if self.b6 else conv_geom_pack
            for cv in self.plan.convs:
                wt = cv["module"].weight.detach().to(torch.float32)
                wpos, wneg = wt.clamp(min=0), wt.clamp(max=0)
                if cv["nonneg"]:
                    zneg, rows = wneg, torch.cat([wpos, wneg], 0)
                    y = wt
                else:
                    pad = torch.zeros(wt.shape[0], self.c2 - 2 * self.cin, *wt.shape[2:], device=self.device)
                    zneg = torch.cat([wneg, wpos, pad], 1)
                    rows = torch.cat([torch.cat([wpos, wneg, pad], 1), zneg], 0)
                    y = torch.cat([wt, wt, pad], 1)
                self._ab_packs.append(dict(fwd=pack(torch.cat([y, zneg], 0), _lib.GEOM_FWD), bwd=pack(rows, _lib.GEOM_BWD)))
            torch.cuda.current_stream().synchronize()
        return self._ab_packs

    def _ab_coef(self):
        """qn per conv = BatchNorm fraction / safe(Z-), per IMAGE, from the trace's stored inputs: one stacked forward contraction
        [y | Z-] and one streaming pass per conv at the first alpha-beta call after a `forward`, kept until the next one"""
        if self._qn_serial == self._serial:
            return self._qn
        ab, t, B = self._ab_state(), self.trace, self.n_img
        if self._qn is None or self._qn[0].shape != t["q"][0].shape:
            self._qn = [torch.empty_like(q) for q in t["q"]]
        inputs = {0: t["xs"]}
        for bi, blk in enumerate(self.plan.blocks):
            x = t["out"][bi - 1] if bi > 0 else t["pool"]
            inputs[blk["conv1"]], inputs[blk["conv2"]], inputs[blk["conv3"]] = x, t["act"][blk["conv1"]], t["act"][blk["conv2"]]
            if blk["downsample"] is not None:
                inputs[blk["downsample"]] = x
        for i, pk in enumerate(self.packs):
            hw, ohw = self.dims[i]
            yz = t["yz"][: B * ohw[0] * ohw[1] * 2 * pk["cout"]].view(B, ohw[0] * ohw[1], 2 * pk["cout"])
            conv_geom_ex(inputs[i], ab[i]["fwd"], _lib.GEOM_FWD, B, hw, ohw, pk["geom"], pk["k_in"], 2 * pk["cout"], out=yz, b6=self.b6)
            resnet_coef_neg(yz, pk["w"], pk["b"], self._qn[i])
        self._qn_serial = self._serial
        return self._qn

    def relevance_alpha_beta(self, r_feat_nhwc, map2img=None, alpha=2., beta=1., out=None, layer_ms=None):
        """`relevance` with the preset's Conv2d rule replaced by the general alpha-beta rule without bias, R = alpha lrp_backward(PosNetConv)
        - beta lrp_backward(NegNetConv) (LRPtools/lrp_modules.py:124-150): same arguments, same result shape, same map2img contract, in
        the engine's conv mode.  BatchNorm, ReLU, Add and MaxPool2d rules are those of `relevance`.  Per conv one transposed contraction
        over the stacked rows [W+ ; W-] with the operand (R qp) alpha | (R qn) (-beta) formed while the tile is gathered
        (`conv_geom_ab`); beta == 0 contracts over W+ alone.  alpha and beta are launch arguments: qp is the trace's q, qn is made per
        image at the first call after a `forward` (`_ab_coef`) and kept; another (alpha, beta) on the same trace does no forward
        work.  The dual packs come from the model's weights as they are at the first call.  alpha = 1, beta = 0 is `relevance`, bit
        for bit.  |R| grows by about (alpha + beta) per conv where beta != 0: a deep net can leave fp32's range."""
        alpha, beta = float(alpha), float(beta)
        if not (alpha == alpha and beta == beta and abs(alpha) != float("inf") and abs(beta) != float("inf")):
            raise ValueError("ResNetEncoder.relevance_alpha_beta: alpha and beta must be finite")
        r, map2img, out, n_maps = self._map_args("relevance_alpha_beta", r_feat_nhwc, "r_feat_nhwc", map2img, out)
        dual = beta != 0.
        qn = self._ab_coef() if dual else None
        ab = self._ab_packs
        t, dims, packs, B, b6 = self.trace, self.dims, self.packs, self.n_img, self.b6

        def convT(i, r_out, x, addend, o, n_oc):
            pk = packs[i]
            hw, ohw = dims[i]
            conv_geom_ab(r_out, ab[i]["bwd"] if dual else pk["bwd"], n_maps, hw, ohw, pk["geom"], pk["cout"], n_oc, x, t["q"][i],
                         q2=qn[i] if dual else None, scale=alpha, scale2=-beta if dual else 0., addend=addend, map2img=map2img, n_img=B,
                         out=o, validate=False, b6=b6)
        return self._walk_lrp(r, map2img, out, n_maps, layer_ms, convT)

    # ---- the gradient chain -----------------------------------------------------------------------------------------
    def _grad_state(self):
        """per conv: the transposed pack of the RAW weights W (K = cout; the stem onto its cin image channels) in the engine's mode.
        Built once per engine from the model's weights, at the first gradient call."""
        if not self._grad_packs:
            pack = conv_geom_pack_bf16x3 if self.b6 else conv_geom_pack
            for cv in self.plan.convs:
                self._grad_packs.append(pack(cv["module"].weight.detach().to(torch.float32), _lib.GEOM_BWD))
            torch.cuda.current_stream().synchronize()
        return self._grad_packs

    def gradient(self, d_feat_nhwc, map2img=None, out=None, layer_ms=None):
        """The autograd gradient of the image (ExplainGridTDGradient.explain_cnn, models/gridTDmodel.py:1510-1521) for n_maps maps:
        (n_maps, h w, C) gradient at the feature map -> (n_maps, cin, H, W); arguments and map2img contract of `relevance`.  ReLU:
        the trace's mask; BatchNorm (eval): its factor; conv: transposed conv with the raw weights; Add: both branches; MaxPool2d: the
        first maximum.  No forward work, no divisions; the trace is only read."""
        return self._grad_chain("gradient", d_feat_nhwc, map2img, out, None, layer_ms)

    def guided_backprop(self, d_feat_nhwc, map2img=None, out=None, relus="stem", layer_ms=None):
        """Guided backprop on the trace, arguments as `gradient`.  relus="stem": the reference's behaviour
        (ExplainiGridTDGuidedGradient.register_hooks, models/gridTDmodel.py:1677-1691, hooks the encoder's DIRECT children: on a ResNet
        the stem's ReLU alone) - the plain gradient with max(g, 0) at the stem ReLU's output.  relus="all": max(g, 0) at every ReLU
        output (stem, both inner ReLUs of each block, each block's ReLU behind the Add), canonical guided backprop."""
        if relus not in ("stem", "all"):
            raise ValueError("ResNetEncoder.guided_backprop: relus must be 'stem' or 'all', got {!r}".format(relus))
        return self._grad_chain("guided_backprop", d_feat_nhwc, map2img, out, relus, layer_ms)

    def _grad_chain(self, fn, d_feat_nhwc, map2img, out, relus, layer_ms):
        g, map2img, out, n_maps = self._map_args(fn, d_feat_nhwc, "d_feat_nhwc", map2img, out)
        gp = self._grad_state()
        t, dims, packs, B, b6 = self.trace, self.dims, self.packs, self.n_img, self.b6
        clamp_all, clamp_stem = relus == "all", relus is not None

        def head(bi, g, ws):
            g0 = ws["r1"][: g.numel()].view(g.shape)                   # the gradient at the Add's sum: both branches take it
            resnet_relu_grad(g, t["out"][bi], map2img, g0, n_maps, B, clamp_all)
            return g0, g0

        def convT(i, g_out, x, addend, o, n_oc):
            pk = packs[i]
            hw, ohw = dims[i]
            relu = pk["relu"]                                          # the ReLU behind conv i: its mask, and guided backprop's clamp
            conv_geom_grad(g_out, gp[i], n_maps, hw, ohw, pk["geom"], pk["cout"], n_oc, mask=t["act"][i] if relu else None,
                           scale=pk["w"], clamp=relu and (clamp_stem if i == 0 else clamp_all), addend=addend, map2img=map2img, n_img=B,
                           out=o, validate=False, b6=b6)
        pix = self.shape[1] * self.shape[2]
        return self._walk(g, map2img, out, n_maps, layer_ms, head, convT, resnet_maxpool_grad, self.cin,
                          lambda gi, o: check(_lib.load().lrpx_nhwc_to_nchw(ptr(gi), ptr(o), n_maps, self.cin, pix, self.cin, stream_ptr())))

    def _workspace(self, n_maps):
        """per-map scratch, sized once per (trace shape, n_maps): r1 / r2 of the Add split, two chain buffers, two block-input buffers"""
        ws = self._ws.get(n_maps)
        if ws is None:
            per_blk = max(o[0].numel() for o in self.trace["out"])
            per_in = max([self.trace["pool"][0].numel()] + [o[0].numel() for o in self.trace["out"]])
            per_any = max([self.trace["xs"][0].numel(), per_in] + [a[0].numel() for a in self.trace["act"]])
            new = lambda per: torch.empty(n_maps * per, dtype=torch.float32, device=self.device)
            ws = {"r1": new(per_blk), "r2": new(per_blk), "a": new(per_any), "b": new(per_any), "r": [new(per_in), new(per_in)]}
            self._ws = {n_maps: ws}
        return ws


def _events(layer_ms):
    if layer_ms is None:
        return None
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    return ev


def _events_done(ev, layer_ms, name):
    if ev is not None:
        ev[1].record()
        ev[1].synchronize()
        layer_ms[name] = layer_ms.get(name, 0.) + ev[0].elapsed_time(ev[1])
