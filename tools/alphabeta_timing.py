#!/usr/bin/env python3
"""What the general alpha-beta rule costs through the VGG16 encoder: `Vgg16.relevance_alpha_beta(alpha 2, beta 1)` beside
`Vgg16.relevance()` with the context's conv mode 0 (the same fp32 MFMA) on the same trace in the same process, the one-off
Z+ / Z- pass separately, and the milliseconds per layer.

    python tools/alphabeta_timing.py [--out profiles/alphabeta_timing.txt]       # 16 images x 20 maps (BASELINE config 2) and 1 x 20
    python tools/alphabeta_timing.py --images 16 --maps-per-image 20             # one configuration, in this process
    python tools/alphabeta_timing.py --conv-mode 1 [--out profiles/alphabeta_mode1_timing.txt]

--conv-mode 1: the context runs in conv mode 1 (the exact bf16 split, the process default) and the report sets three paths side by
side on the same trace in the same process - the preset `relevance()`, the mode-0 `relevance_alpha_beta` and the mode-1 chain
`relevance_alpha_beta(conv_mode=1)` - with the one-off coefficient pass and the new chain's milliseconds per layer.

Without --images every configuration runs in a child process of its own under a time limit, and the first failure ends the
run.  Times are HIP events around work on one stream, after a warm-up of every shape; nothing here is asserted."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(16, 20), (1, 20)]
STEP_LIMIT_S = 240
LAYERS = ["conv1_1", "conv1_2", "pool1", "conv2_1", "conv2_2", "pool2", "conv3_1", "conv3_2", "conv3_3", "pool3", "conv4_1", "conv4_2",
          "conv4_3", "pool4", "conv5_1", "conv5_2", "conv5_3"]


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def one_mode1(images, per_image, iters):
    """--conv-mode 1: preset, mode-0 alpha-beta and mode-1 alpha-beta on one trace"""
    import torch
    sys.path.insert(0, ROOT)
    import lrp_amd  # noqa: F401
    from lrp_amd import ops, weights
    if not torch.cuda.is_available():
        raise SystemExit("alphabeta_timing: no GPU - a time is measured on the device or not at all")
    sd = weights.make_gridtd_state(seed=0, vocab_size=64)
    names = [k for k in sd if k.startswith("img_encoder.encoder.") and k.endswith(".weight")]
    vgg = ops.Vgg16([torch.from_numpy(sd[k]).cuda() for k in names],
                    [torch.from_numpy(sd[k.replace(".weight", ".bias")]).cuda() for k in names])
    vgg.conv_mode = 1
    n_maps = images * per_image
    vgg.forward(torch.from_numpy(weights.make_images(0, images)).cuda())
    torch.manual_seed(0)
    r_feat = torch.randn(n_maps, 196, 512, device="cuda")
    m2i = (torch.arange(n_maps, device="cuda") // per_image).to(torch.int32)
    out = torch.empty(n_maps, 3, 224, 224, device="cuda")
    st = vgg._ab1_state()                                   # packs (once per context)

    def coef():
        st["serial"] = -1
        vgg._ab1_coef(st)
    paths = [("relevance() conv mode 1 (alpha1beta0)", lambda: vgg.relevance(r_feat, m2i, out=out)),
             ("relevance_alpha_beta(2, 1) conv_mode=0", lambda: vgg.relevance_alpha_beta(r_feat, m2i, 2., 1., out=out)),
             ("relevance_alpha_beta(2, 1) conv_mode=1", lambda: vgg.relevance_alpha_beta(r_feat, m2i, 2., 1., out=out, conv_mode=1)),
             ("relevance_alpha_beta(2, 0) conv_mode=1", lambda: vgg.relevance_alpha_beta(r_feat, m2i, 2., 0., out=out, conv_mode=1))]
    for _, fn in paths:                                     # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    t_c = timed(coef, iters)
    t = [timed(fn, iters) for _, fn in paths]
    lm = [0.0] * 17
    vgg.relevance_alpha_beta(r_feat, m2i, 2., 1., out=out, layer_ms=lm, conv_mode=1)
    print(f"== {images} image(s) x {per_image} maps = {n_maps} maps, {iters} iterations, {torch.cuda.get_device_name(0)}")
    for (name, _), ms in zip(paths, t):
        print(f"{name:<40}: {ms:9.2f} ms  {n_maps / ms * 1e3:9.1f} maps/s   {ms / t[1]:.2f}x the mode-0 alpha-beta path, "
              f"{ms / t[0]:.2f}x the mode-1 preset")
    print(f"one-off coefficient pass ({images} image(s))      : {t_c:9.2f} ms  {t_c / images:9.2f} ms per image")
    print("relevance_alpha_beta(2, 1) conv_mode=1 per layer, ms (one launch per conv, timed launch by launch; a pool is part of the conv below it)")
    for l in range(16, -1, -1):
        print(f"{LAYERS[l]:<8} {lm[l]:12.3f}")
    print(f"{'sum':<8} {sum(lm):12.3f}")


def one(images, per_image, iters):
    import ctypes as C
    import torch
    sys.path.insert(0, ROOT)
    import lrp_amd  # noqa: F401
    from lrp_amd import ops, weights
    if not torch.cuda.is_available():
        raise SystemExit("alphabeta_timing: no GPU - a time is measured on the device or not at all")
    sd = weights.make_gridtd_state(seed=0, vocab_size=64)
    names = [k for k in sd if k.startswith("img_encoder.encoder.") and k.endswith(".weight")]
    vgg = ops.Vgg16([torch.from_numpy(sd[k]).cuda() for k in names],
                    [torch.from_numpy(sd[k.replace(".weight", ".bias")]).cuda() for k in names])
    vgg.conv_mode = 0
    n_maps = images * per_image
    vgg.forward(torch.from_numpy(weights.make_images(0, images)).cuda())
    torch.manual_seed(0)
    r_feat = torch.randn(n_maps, 196, 512, device="cuda")
    m2i = (torch.arange(n_maps, device="cuda") // per_image).to(torch.int32)
    out = torch.empty(n_maps, 3, 224, 224, device="cuda")
    st = vgg._ab_state()                                    # packs (once per context)

    def zpn():
        st["serial"] = -1
        vgg._ab_zpn(st)
    zpn()
    vgg.relevance(r_feat, m2i, out=out)
    vgg.relevance_alpha_beta(r_feat, m2i, 2., 1., out=out)
    torch.cuda.synchronize()
    t_z = timed(zpn, iters)
    t_10 = timed(lambda: vgg.relevance(r_feat, m2i, out=out), iters)
    t_ab = timed(lambda: vgg.relevance_alpha_beta(r_feat, m2i, 2., 1., out=out), iters)
    lm10 = (C.c_float * 17)()
    vgg.relevance(r_feat, m2i, out=out, layer_ms=lm10)
    lmab = [0.0] * 17
    vgg.relevance_alpha_beta(r_feat, m2i, 2., 1., out=out, layer_ms=lmab)
    print(f"== {images} image(s) x {per_image} maps = {n_maps} maps, {iters} iterations, {torch.cuda.get_device_name(0)}")
    print(f"relevance() conv mode 0 (alpha1beta0)  : {t_10:9.2f} ms  {n_maps / t_10 * 1e3:9.1f} maps/s")
    print(f"relevance_alpha_beta(alpha2beta1)      : {t_ab:9.2f} ms  {n_maps / t_ab * 1e3:9.1f} maps/s   ratio {t_ab / t_10:.2f}x")
    print(f"one-off Z+ / Z- pass ({images} image(s))       : {t_z:9.2f} ms  {t_z / images:9.2f} ms per image")
    print("per layer, ms (relevance_alpha_beta: elementwise pass + conv, timed launch by launch; a pool is part of the conv below it)")
    print(f"{'layer':<8} {'alpha1beta0':>12} {'alpha2beta1':>12}")
    for l in range(16, -1, -1):
        print(f"{LAYERS[l]:<8} {lm10[l]:12.3f} {lmab[l]:12.3f}")
    print(f"{'sum':<8} {sum(lm10):12.3f} {sum(lmab):12.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=None)
    ap.add_argument("--maps-per-image", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--conv-mode", type=int, default=0, choices=(0, 1),
                    help="0: the mode-0 report; 1: preset, mode-0 and mode-1 alpha-beta paths on a mode-1 trace")
    a = ap.parse_args()
    if a.images is not None:
        return (one_mode1 if a.conv_mode == 1 else one)(a.images, a.maps_per_image, a.iters)
    report = []
    for images, per in CONFIGS:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--images", str(images), "--maps-per-image", str(per),
                            "--iters", str(a.iters), "--conv-mode", str(a.conv_mode)], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            raise SystemExit(f"alphabeta_timing: {images} x {per} failed with status {p.returncode}; nothing more is started")
        report.append(p.stdout)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/alphabeta_timing.py" + (" --conv-mode 1" if a.conv_mode == 1 else "") + "\n" + "\n".join(report))


if __name__ == "__main__":
    main()
