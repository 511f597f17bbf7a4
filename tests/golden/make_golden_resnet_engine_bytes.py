#!/usr/bin/env python3
"""Output digests of the batched bottleneck-ResNet encoder engine (ops.ResNetEncoder: forward, relevance, relevance_alpha_beta, gradient,
guided_backprop, in both conv modes) and of the elementwise entries of csrc/resnet_engine.hip, recorded once from a build AND a Python
tree whose bytes are to be kept - tests/test_gpu_resnet_engine_bytes.py runs the same case functions on the tree at hand and requires
every sha256 to be the recorded one.  Writes tests/golden/resnet_engine_bytes.json: digests only, with the commit they were recorded from.

    python tests/golden/make_golden_resnet_engine_bytes.py --commit <hash of the checkout this runs in>

Needs a GPU; run it from a checkout of that commit (library and ops.py both), never from a tree whose bytes are in question.

Engine cases, per net and conv mode: `bottleneck_net` of make_golden_resnet.TINY (base 8, blocks [2, 1], 2 x 3 x 38 x 34: blocks with
and without a downsample; four maps on [0, 0, 1, 1], gradients on resnet_grad.npz's [1, 0]) and of make_golden_resnet_engine.ENGINE
(base 12, blocks [1, 2, 1], 2 x 3 x 45 x 51, map2img [1, 0, 1]: ragged tiles, unsorted maps), built from the seeds stored in
resnet_tiny.npz / resnet_engine.npz, inputs from those files and resnet_grad.npz.  Digested: the feature map, every trace tensor the
passes read, relevance with and without map2img, relevance_alpha_beta at three (alpha, beta), the qn list it leaves, gradient, and
guided_backprop with relus 'stem' and 'all'.

Elementwise cases, straight at the C entries, at the smallest shapes where they can go wrong (the two nets only have a 3x3 s2 p1 pool
and friendly values): the three pool entries on a 7 x 5 map of 5 channels under three windows, on inputs quantised so that ties inside
a window ("first maximum wins") and windows whose maximum is exactly 0 (the safe divisor) both occur; the two coefficient entries on
7 rows of 5 channels at ld = 2c and 2c + 3 with y w = 0 and b = 0, Z = 0 and ordinary values; add_split and relu_grad (clamp 0 / 1) on
35 floats per map with exact zeros and negatives in act.  The per-map entries run three maps on two images with map2img [1, 0, 1] and
two maps without map2img.  That each condition occurs is asserted here, on the CPU.

Every output buffer is pre-filled with one fixed bit pattern (a NaN): what a launch leaves unwritten shows in the digest.  Each case
also stores one digest of its inputs, so that a changed draw is told apart from a changed kernel."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden_resnet import TINY, bottleneck_net  # noqa: E402
from make_golden_resnet_engine import ENGINE  # noqa: E402

JSON = os.path.join(HERE, "resnet_engine_bytes.json")
FILL = 0x7FC12345                        # the NaN of make_golden_conv_geom_bytes.py
NETS = {"tiny": TINY, "engine": ENGINE}
MODES = (0, 1)
ALPHA_BETA = ((1., 0.), (2., 1.), (1.5, 0.5))
POOL_HW, POOL_C = (7, 5), 5
POOL_WINDOWS = {"k3s2p1": (3, 3, 2, 2, 1, 1), "k2s2p0": (2, 2, 2, 2, 0, 0), "k3x2s1x2p1x0": (3, 2, 1, 2, 1, 0)}   # (kh, kw, sh, sw, ph, pw)
COEF_ROWS, COEF_C = 7, 5
PER_MAP = 35
N_IMG, MAP2IMG = 2, [1, 0, 1]


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(torch.as_tensor(t).detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def filled(*shape):
    n = int(np.prod(shape))
    return torch.full((n,), FILL, dtype=torch.int32, device="cuda").view(torch.float32).view(*shape)


def _i32(v):
    return torch.tensor([int(a) for a in v], dtype=torch.int32, device="cuda")


# ---- the engine -----------------------------------------------------------------------------------------------------------------------
def engine_inputs(name):
    """the CPU arrays of one net: seed, images, relevance targets / gradients at the feature map (NCHW) and their map2img"""
    load = lambda f: np.load(os.path.join(HERE, f))
    grad = load("resnet_grad.npz")
    if name == "tiny":
        T = load("resnet_tiny.npz")
        t1, t2 = T["target1"], T["target2"]
        c = dict(seed=int(T["seed"]), x=T["x"], targets=np.stack([t1[0], t2[0], t1[1], t2[1]]), map2img=[0, 0, 1, 1])
    else:
        E = load("resnet_engine.npz")
        c = dict(seed=int(E["seed"]), x=E["x"], targets=E["targets"], map2img=[int(v) for v in E["map2img"]])
    c["d_feat"], c["grad_map2img"] = grad[name + "_d_feat"], [int(v) for v in grad[name + "_map2img"]]
    return c


def engine_case(name, mode, ops, _lib):
    """(digest of the inputs and the net's tensors, {case: sha256 of the output bytes}) of one net in one conv mode, in a fixed order"""
    from lrp_amd.LRPtools import lrp_modules
    c, cfg = engine_inputs(name), NETS[name]
    net = bottleneck_net(np.random.RandomState(c["seed"]), lrp_modules.resAdd, cfg["base"], cfg["blocks"])
    digest = sha(c["x"], c["targets"], np.asarray(c["map2img"], dtype=np.int32), c["d_feat"], np.asarray(c["grad_map2img"], dtype=np.int32),
                 *[v for _, v in sorted(net.state_dict().items())])
    eng = ops.ResNetEncoder(net.cuda(), conv_mode=mode)
    x = torch.from_numpy(c["x"]).cuda()
    B, shape = x.shape[0], tuple(x.shape[1:])
    r, m2i = ops.nchw_to_nhwc(torch.from_numpy(c["targets"]).cuda()), _i32(c["map2img"])
    g, gm2i = ops.nchw_to_nhwc(torch.from_numpy(c["d_feat"]).cuda()), _i32(c["grad_map2img"])
    res = {}
    res["forward"] = sha(eng.forward(x))
    t = eng.trace
    res["trace"] = sha(t["xs"], t["pool"], *(t["act"] + t["q"] + t["out"] + t["c1"] + t["c2"]))
    out = lambda n: filled(n, *shape)
    res["relevance"] = sha(eng.relevance(r, m2i, out=out(len(r))))
    res["relevance_nomap"] = sha(eng.relevance(r[:B].contiguous(), out=out(B)))
    for a, b in ALPHA_BETA:
        res["alpha_beta_%g_%g" % (a, b)] = sha(eng.relevance_alpha_beta(r, m2i, alpha=a, beta=b, out=out(len(r))))
    res["qn"] = sha(*eng._qn)
    res["gradient"] = sha(eng.gradient(g, gm2i, out=out(len(g))))
    res["gradient_nomap"] = sha(eng.gradient(g[:B].contiguous(), out=out(B)))
    for relus in ("stem", "all"):
        res["guided_" + relus] = sha(eng.guided_backprop(g, gm2i, out=out(len(g)), relus=relus))
    res["trace_after"] = sha(t["xs"], t["pool"], *(t["act"] + t["q"] + t["out"] + t["c1"] + t["c2"]))     # the passes only read it
    return digest, res


# ---- the elementwise entries ----------------------------------------------------------------------------------------------------------
def _map_sets():
    """(tag, n_maps, map2img or None): three maps on two images, and one map per image"""
    return (("m2i", len(MAP2IMG), _i32(MAP2IMG)), ("nomap", N_IMG, None))


def pool_inputs(win):
    """x (N_IMG, H W, c) >= 0 on a quarter grid, with a tie at a positive maximum and an all-zero window under `win`, and r_out"""
    kh, kw, sh, sw, ph, pw = win
    (h, w), c = POOL_HW, POOL_C
    oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    for seed in range(7100, 7200):
        g = torch.Generator().manual_seed(seed)
        x = (torch.round(4 * torch.randn(N_IMG, h * w, c, generator=g)) / 4).clamp(min=0)
        ties = zeros = 0
        xi = x.view(N_IMG, h, w, c)
        for i in range(oh):
            for j in range(ow):
                v = xi[:, max(i * sh - ph, 0): min(i * sh - ph + kh, h), max(j * sw - pw, 0): min(j * sw - pw + kw, w)].reshape(N_IMG, -1, c)
                mx = v.max(dim=1).values
                ties += int((((v == mx[:, None]).sum(dim=1) > 1) & (mx > 0)).sum())
                zeros += int((mx == 0).sum())
        if ties and zeros:
            r_out = torch.randn(len(MAP2IMG), oh * ow, c, generator=g)
            return dict(x=x, r_out=r_out, ohw=(oh, ow), ties=ties, zeros=zeros, digest=sha(x, r_out))
    raise AssertionError("no draw with a tie at a positive maximum and an all-zero window")


def pool_case(wname, ops, _lib):
    from lrp_amd._lib import check, ptr, stream_ptr
    win, lib = POOL_WINDOWS[wname], _lib.load()
    c = pool_inputs(win)
    assert c["ties"] > 0 and c["zeros"] > 0
    (h, w), (oh, ow), ch = POOL_HW, c["ohw"], POOL_C
    x, r_all = c["x"].cuda(), c["r_out"].cuda()
    res = {}
    y = filled(N_IMG, oh * ow, ch)
    check(lib.lrpx_resnet_maxpool_fwd(ptr(x), ptr(y), N_IMG, h, w, oh, ow, ch, *win, stream_ptr()))
    res["fwd"] = sha(y)
    for tag, n, m2i in _map_sets():
        r_out = r_all[:n].contiguous()
        for entry in ("rel", "grad"):
            o = filled(n, h * w, ch)
            check(getattr(lib, "lrpx_resnet_maxpool_" + entry)(ptr(x), ptr(r_out), ptr(m2i), ptr(o), n, N_IMG, h, w, oh, ow, ch, *win, stream_ptr()))
            res["%s_%s" % (entry, tag)] = sha(o)
    return c["digest"], res


def coef_inputs(ld):
    rows, c = COEF_ROWS, COEF_C
    g = torch.Generator().manual_seed(7300 + ld)
    yz, w, b = torch.randn(rows, ld, generator=g), torch.randn(c, generator=g), torch.randn(c, generator=g)
    b[1] = 0.
    yz[2, 1] = 0.              # y w = 0 and b = 0: the fraction's safe divisor
    yz[5, 1] = -0.
    w[3] = 0.                  # y w = 0 with b != 0: the fraction is 0
    yz[4, c + 2] = 0.          # Z = 0
    yz[2, c + 1] = 0.          # both at once
    yz[6, c + 4] = -0.
    y, z = yz[:, :c], yz[:, c: 2 * c]
    den = (y * w).abs() + b.abs()
    assert (den == 0).any() and (z == 0).any() and ((den != 0) & (z != 0)).any() and ((den == 0) & (z == 0)).any()
    return dict(yz=yz, w=w, b=b, digest=sha(yz, w, b))


def coef_case(ld, ops, _lib):
    from lrp_amd._lib import check, ptr, stream_ptr
    lib, (rows, c) = _lib.load(), (COEF_ROWS, COEF_C)
    d = coef_inputs(ld)
    yz, w, b = d["yz"].cuda(), d["w"].cuda(), d["b"].cuda()
    res = {}
    for relu in (0, 1):
        act, q = filled(rows, c), filled(rows, c)
        check(lib.lrpx_resnet_bn_act_coef(ptr(yz), ld, ptr(w), ptr(b), ptr(act), ptr(q), rows, c, relu, stream_ptr()))
        res["bn_act_coef_relu%d" % relu] = sha(act, q)
    qn = filled(rows, c)
    check(lib.lrpx_resnet_coef_neg(ptr(yz), ld, ptr(w), ptr(b), ptr(qn), rows, c, stream_ptr()))
    res["coef_neg"] = sha(qn)
    return d["digest"], res


def per_map_inputs():
    g = torch.Generator().manual_seed(7400)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = dict(r=rn(len(MAP2IMG), PER_MAP), c1=rn(N_IMG, PER_MAP), c2=rn(N_IMG, PER_MAP), act=torch.round(2 * rn(N_IMG, PER_MAP)) / 2)
    assert (d["act"] == 0).any() and (d["act"] < 0).any() and (d["act"] > 0).any() and (d["r"] < 0).any()
    d["digest"] = sha(d["r"], d["c1"], d["c2"], d["act"])
    return d


def per_map_case(ops, _lib):
    from lrp_amd._lib import check, ptr, stream_ptr
    lib, d = _lib.load(), per_map_inputs()
    r_all, c1, c2, act = (d[k].cuda() for k in ("r", "c1", "c2", "act"))
    res = {}
    for tag, n, m2i in _map_sets():
        r = r_all[:n].contiguous()
        r1, r2 = filled(n, PER_MAP), filled(n, PER_MAP)
        check(lib.lrpx_resnet_add_split(ptr(r), ptr(c1), ptr(c2), ptr(m2i), ptr(r1), ptr(r2), n, N_IMG, PER_MAP, stream_ptr()))
        res["add_split_" + tag] = sha(r1, r2)
        for clamp in (0, 1):
            o = filled(n, PER_MAP)
            check(lib.lrpx_resnet_relu_grad(ptr(r), ptr(act), ptr(m2i), ptr(o), n, N_IMG, PER_MAP, clamp, stream_ptr()))
            res["relu_grad_clamp%d_%s" % (clamp, tag)] = sha(o)
    return d["digest"], res


def _case(fn, *args):
    return lambda ops, _lib: fn(*args, ops, _lib)


# name -> f(ops, _lib) = (digest of the inputs, {case: digest of the output}); the test runs these very functions
CASES = {}
for _n in NETS:
    for _m in MODES:
        CASES["engine_%s_mode%d" % (_n, _m)] = _case(engine_case, _n, _m)
for _w in POOL_WINDOWS:
    CASES["pool_" + _w] = _case(pool_case, _w)
for _ld in (2 * COEF_C, 2 * COEF_C + 3):
    CASES["coef_ld%d" % _ld] = _case(coef_case, _ld)
CASES["per_map"] = per_map_case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit of the checkout (library and Python tree) this runs in")
    ap.add_argument("--out", default=JSON)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lrp_amd  # noqa: F401
    from lrp_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_resnet_engine_bytes: needs a GPU")
    g = {"recorded_from_commit": a.commit, "fill": "0x%08X" % FILL, "cases": {}}
    for name, fn in CASES.items():
        digest, res = fn(ops, _lib)
        torch.cuda.synchronize()
        g["cases"][name] = {"inputs": digest, "outputs": res}
    with open(a.out, "w") as f:
        json.dump(g, f, indent=0, sort_keys=True)
        f.write("\n")
    print(os.path.basename(a.out) + ":", os.path.getsize(a.out), "bytes;", len(CASES), "cases,",
          sum(len(c["outputs"]) for c in g["cases"].values()), "digests, library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
