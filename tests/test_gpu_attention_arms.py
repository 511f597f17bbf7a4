"""The attention / Grad-CAM / chance arms of the experiments on the device: the seams (explainers/attention.py on the three models and their
drop-ins) and the reference's own run of the experiments on sharpened states (tests/golden/attention_arms.npz, written by
tests/golden/make_golden_attention.py - its docstring names every array).

Bounds.  A map formed by `expand_maps` from the alphas / cams the reference itself had is within the golden's per-row `bound` of the
reference's map (derived in tests/test_gpu_expand_maps.py); every correctness ratio is then within the golden's `sens` (the largest change
of that ratio under such a move, computed from the reference's map alone) + 1e-5, every statistic within `bound` + 1e-5.  Probabilities:
2e-4 of the largest score of the reference's teacher-forced calls, the bound of tests/test_gpu_ablation.py.  Ids, masks, captions,
positions: bit-exact, from the ENGINE's own alphas - the stored rows keep a gap of 1e-3 between the 20th and 21st patch sum.
The engine's alphas against the reference's: the decoder tests hold the attention logits to 1e-4 of their largest
(tests/test_gpu_decoder_fwd_alone.py); the unsharpened logits are w_h . tanh(.), at most ||w_h||_1, and sharpening multiplies logits and
errors by `factor`; a softmax value moves by at most twice the logit error, relatively: 2e-4 factor ||w_h||_1 (printed with the figure)."""
import os
import types

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _args():
    return types.SimpleNamespace(embed_dim=512, hidden_dim=512, encoder='vgg16', weight='', save_path='/tmp', dataset='synthetic',
                                 height=224, width=224, num_head=8)


def _bits(t):
    return t.contiguous().view(torch.int32)


_G = {}


def _golden():
    if not _G:
        with np.load(os.path.join(GOLDEN, "attention_arms.npz"), allow_pickle=False) as f:
            _G.update({k: f[k] for k in f.files})
    return _G


def _ref_map(a, normalize=True, p=14, upscale=16):
    from oracle import lrp_oracle as O
    e = O.pyramid_expand(torch.from_numpy(np.asarray(a, np.float32).reshape(p, p)), upscale).double().numpy()
    if not normalize:
        return e
    m = np.abs(e).max()
    return np.zeros(e.shape) if m == 0 else 1.0 * e / m


@pytest.mark.parametrize("model", ["gridtd", "aoa", "adaatt"])
def test_attention_maps_are_expand_maps_of_the_trace(model):
    """`attention_maps(engine, tr)` is `ops.expand_maps` of tr["alpha"] at the encoder's image size, row for row (all rows, and the valid
    rows of ragged `lens` in image-major order); it is the map of the drop-in's `.alphas[t]`, the array evaluation.py reads."""
    _need_gpu()
    from lrp_amd import ops, weights
    from lrp_amd.explainers import attention_maps, one_minus_beta
    V, B, T = 307, 2, 3
    wm = weights.make_word_map(V)
    images = torch.from_numpy(weights.make_images(3, B)).cuda()
    caps = torch.from_numpy(weights.make_captions(4, B, T, V)).cuda()
    if model == "gridtd":
        from lrp_amd.explainers.gridtd import ExplainGridTDAttention as Ex
        sd = weights.sharpen_attention(weights.make_gridtd_state(seed=2, vocab_size=V), 64)
    elif model == "aoa":
        from lrp_amd.explainers.aoa import ExplainAOAAttention as Ex
        sd = weights.sharpen_attention(weights.make_aoa_state(seed=2, vocab_size=V), 256)
    else:
        from lrp_amd.explainers.adaatt import ExplainAdaptiveAttention as Ex
        sd = weights.sharpen_attention(weights.make_adaatt_state(seed=2, vocab_size=V), 64)
    ex = Ex(_args(), wm, model=sd)
    eng = ex.engine
    enc = eng.encode(images)
    tr = eng.trace(enc, caps, predictions=False)
    alpha = tr["alpha"]
    flat = alpha.reshape((B * T,) + tuple(alpha.shape[2:])).contiguous()
    heads = [None] if model != "aoa" else [None, 5]
    for head in heads:
        for normalize in (True, False):
            got = attention_maps(eng, tr, head=head, normalize=normalize)
            assert got.shape == (B * T, 224, 224)
            assert torch.equal(_bits(got), _bits(ops.expand_maps(flat, 224, head=head, normalize=normalize)))
            ragged = attention_maps(eng, tr, lens=[3, 2], head=head, normalize=normalize)
            assert torch.equal(_bits(ragged), _bits(got[[0, 1, 2, 3, 4]]))
        # the drop-in: one image, its `.alphas[t]`
        ex.get_hidden_parameters(images[:1], caption_encode=caps[0].tolist())
        tr1 = eng.trace(eng.encode(images[:1]), caps[:1].contiguous(), predictions=False)
        own = attention_maps(eng, tr1, head=head)
        for t in range(T):
            a = ex.alphas[t][None].contiguous()
            assert torch.equal(_bits(ops.expand_maps(a, 224, head=head, normalize=True)[0]), _bits(own[t])), (model, head, t)
    peak = attention_maps(eng, tr).amax(dim=(1, 2))
    assert torch.equal(peak, torch.ones_like(peak))          # attention is positive: every normalised map peaks at 1
    if model == "aoa":
        with pytest.raises(ValueError):
            attention_maps(eng, tr, head=8)
        with pytest.raises(ValueError, match="sentinel"):
            one_minus_beta(tr)
    else:
        with pytest.raises(ValueError, match="single-head"):
            attention_maps(eng, tr, head=0)
        omb = one_minus_beta(tr, lens=[3, 2])
        assert torch.equal(omb, (1.0 - tr["beta"]).reshape(-1)[:5]) and ((omb >= 0) & (omb <= 1)).all()


def test_engines_without_an_encoder_are_refused():
    _need_gpu()
    from lrp_amd import weights
    from lrp_amd.explainers import AdaAttEngine, attention_maps, gradcam_maps
    from lrp_amd.explainers.gridtd import GridTDBUEngine
    bu = GridTDBUEngine(weights.make_gridtd_bu_state(seed=3, vocab_size=307))
    ada = AdaAttEngine(weights.make_adaatt_state(seed=3, vocab_size=307, feat_dim=192, num_pixels=16, encoder=None))
    for eng, P in ((bu, 36), (ada, 16)):
        with pytest.raises(ValueError, match="no encoder"):
            attention_maps(eng, dict(alpha=torch.zeros(1, 2, P, device="cuda")))
        with pytest.raises(ValueError, match="no encoder"):
            gradcam_maps(eng, torch.zeros(1, 2, P, device="cuda"))


def _box_layout(g, pre):
    """per-box pseudo rows: a word's first box alone, every later box behind an empty box (which scores 0 and takes the first place) -
    `bbox_correctness` then returns the score of every (box, threshold) call of the reference"""
    nbox, boxes = g[pre + "nbox"], g[pre + "boxes"]
    rows, bx, b2r, off = [], [], [], 0
    for r, n in enumerate(nbox):
        for k in range(n):
            if k:
                bx.append([0, 0, 0, 0]); b2r.append(len(rows))
            bx.append(boxes[off + k].tolist()); b2r.append(len(rows))
            rows.append(r)
        off += n
    box2row = np.repeat(np.arange(len(nbox)), nbox)
    return rows, bx, b2r, box2row


def _check_boxes(g, pre, maps, what):
    """maps (rows, 224, 224) normalised, formed from the reference's own alphas / cams"""
    from lrp_amd.explainers import bbox_correctness
    rows, bx, b2r, box2row = _box_layout(g, pre)
    table, sens, best = g[pre + "table"], g[pre + "sens"], g[pre + "best"]
    per_box = bbox_correctness(maps[rows], torch.tensor(bx), b2r).cpu().double().numpy()
    d = np.abs(per_box - table)
    print("%s: %d (box, threshold) ratios, largest deviation %.2e, largest of deviation - sens %.2e; sens: median %.1e, %d of %d at 1" % (
        what, d.size, d.max(), (d - sens).max(), np.median(sens), (sens >= 1).sum(), sens.size))
    assert (d <= sens + 1e-5).all(), (what, np.argwhere(d > sens + 1e-5)[:5].tolist())
    got = bbox_correctness(maps, torch.from_numpy(g[pre + "boxes"]), box2row).cpu().double().numpy()
    row_sens = np.stack([sens[box2row == r].max(axis=0) for r in range(len(best))])
    assert (np.abs(got - best) <= row_sens + 1e-5).all(), what
    # the clean definition: the first boxes are the reference's, a later box is scored on the whole map
    first = np.flatnonzero(np.r_[True, box2row[1:] != box2row[:-1]])
    clean = bbox_correctness(maps, torch.from_numpy(g[pre + "boxes"][first]), box2row[first], carry=False).cpu().double().numpy()
    assert (np.abs(clean - table[first]) <= sens[first] + 1e-5).all(), what
    both = bbox_correctness(maps, torch.from_numpy(g[pre + "boxes"]), box2row, carry=False).cpu().double().numpy()
    assert (both >= clean - 1e-6).all()


def _check_maps(maps, refs, bounds, what):
    worst = 0.0
    for m, ref, b in zip(maps, refs, bounds):
        d = float(np.abs(m.cpu().double().numpy() - ref).max())
        assert d <= b, (what, d, b)
        worst = max(worst, d / b if b > 0 else 0.0)          # (an all-zero map: bound 0, deviation 0)
    print("%s: %d maps, at worst %.2f of the bound" % (what, len(refs), worst))


def test_gridtd_arms_vs_the_references_own_experiments():
    _need_gpu()
    from lrp_amd import evaluation, ops, weights
    from lrp_amd.explainers import ablation, attention_maps, gradcam_maps, one_minus_beta, tpfp_statistics
    from lrp_amd.explainers.gridtd import ExplainGridTDAttention
    g = _golden()
    V, seed, factor = int(g["grid_V"]), int(g["grid_seed"]), float(g["grid_factor"])
    sd = weights.sharpen_attention(weights.make_gridtd_state(seed=seed, vocab_size=V), factor)
    wm = weights.make_word_map(V)
    wm['<end>'] = int(g["grid_end"])
    img = torch.from_numpy(weights.make_images(seed + 7, 1)).cuda()
    ex = ExplainGridTDAttention(_args(), wm, model=sd)
    ex.get_hidden_parameters(img)
    caption = [int(c) for c in ex.beam_caption_encode]
    assert caption == g["grid_caption"].tolist()
    eng, T = ex.engine, len(caption) - 1
    cap_dev = torch.tensor([caption], dtype=torch.int64, device="cuda")
    enc = eng.encode(img)
    tr = eng.trace(enc, cap_dev, predictions=True)
    # the engine's attention against the reference's
    a_ref = g["grid_alphas"].astype(np.float64)
    rel = float((np.abs(tr["alpha"][0].cpu().double().numpy() - a_ref) / a_ref.max(axis=1, keepdims=True)).max())
    db = float(np.abs(tr["beta"][0].cpu().double().numpy() - g["grid_betas"]).max())
    a_tol = 2e-4 * float(np.abs(sd["AdaAttention.w_h.weight"]).sum())          # (the sharpened w_h: factor ||w_h||_1)
    print("gridTD: alpha within %.2e of a row's largest, beta within %.2e (bound %.2e)" % (rel, db, a_tol))
    assert rel < a_tol and db < a_tol
    # (a) maps of the reference's own alphas
    ga = torch.from_numpy(g["grid_alphas"]).cuda()
    ts = g["grid_box_att_t"].tolist()
    norm = ops.expand_maps(ga[ts].contiguous(), 224, normalize=True)
    _check_maps(norm, [_ref_map(g["grid_alphas"][t]) for t in ts], g["grid_box_att_bound"], "gridTD attention maps")
    row = int(g["grid_map_row"])
    assert float(np.abs(norm[row].cpu().double().numpy() - g["grid_map_full"]).max()) <= g["grid_box_att_bound"][row] + 2.0 ** -24
    # (b) bbox: attention and Grad-CAM
    _check_boxes(g, "grid_box_att_", norm, "gridTD attention bbox")
    cams = torch.from_numpy(g["grid_box_cam_cams"]).cuda()
    cam_maps = gradcam_maps(eng, cams, normalize=True)
    _check_maps(cam_maps, [_ref_map(c) for c in g["grid_box_cam_cams"]], g["grid_box_cam_bound"], "gridTD Grad-CAM maps")
    _check_boxes(g, "grid_box_cam_", cam_maps, "gridTD Grad-CAM bbox")
    cap2 = torch.from_numpy(g["grid_box_cam_caption"])[None].cuda()
    own_cam, _ = eng.explain_batch_gradient(img, cap2, cam=True)
    assert own_cam.shape == (1, cap2.shape[1] - 1, 196)
    assert torch.equal(_bits(gradcam_maps(eng, own_cam)), _bits(ops.expand_maps(own_cam[0].contiguous(), 224)))
    dc = float((own_cam[0][g["grid_box_cam_t"].tolist()].cpu() - cams.cpu()).abs().max())
    print("gridTD: the engine's Grad-CAM maps against the reference's (both peak at 1): %.2e" % dc)
    # (c) tpfp: the raw attention map's row, 1 - beta
    ts = g["grid_tpfp_t"].tolist()
    raw = ops.expand_maps(ga[ts].contiguous(), 224)
    stats, q = tpfp_statistics(raw)
    stats, q = stats.cpu().double().numpy(), q.cpu().double().numpy()
    b = g["grid_tpfp_bound"]
    d = [np.abs(stats[:, 0] - g["grid_tpfp_att_mean"]), np.abs(stats[:, 3] - g["grid_tpfp_att_max"]), np.abs(q - g["grid_tpfp_att_quantile"]).max(axis=1)]
    print("gridTD tpfp: %d rows, mean %.2e, max %.2e, quantiles %.2e (bound %.2e + 1e-5)" % (len(ts), d[0].max(), d[1].max(), d[2].max(), b.max()))
    assert all((x <= b + 1e-5).all() for x in d)
    assert (stats[:, 1] == stats[:, 0]).all() and (stats[:, 2] >= stats[:, 0]).all()          # no negative pixel: mean |x| is the mean
    omb = one_minus_beta(tr)[ts].cpu().double().numpy()
    assert (np.abs(omb - g["grid_tpfp_one_minus_beta"]) < a_tol).all()
    # (d) image ablation, attention arm: the engine's own maps
    special = [wm[k] for k in ('<start>', '<end>', '<unk>', '<pad>')]
    kw = dict(start_id=wm['<start>'], end_id=wm['<end>'], special_ids=special, model_bias=ex.TF_MODEL_BIAS)
    tol = 2e-4 * float(g["grid_abl_absmax"])
    own = attention_maps(eng, tr)
    branches = set()
    for arm in ("att", "rnd"):
        pre = "grid_abl_%s_" % arm
        ts = g[pre + "t"].tolist()
        spatial = own[ts] if arm == "att" else torch.from_numpy(g["grid_abl_rnd_perm"].astype(np.float32)).view(-1, 224, 224).cuda()
        targets = [caption[t + 1] for t in ts]
        mask = evaluation.block_image(spatial)
        assert np.array_equal(mask[:, ::8, ::8].cpu().numpy().astype(np.uint8), g[pre + "mask"]), arm
        found, idx, prob, caps = ablation.image_ablation(eng, img, [0] * len(ts), spatial, targets, **kw)
        assert found.cpu().tolist() == g[pre + "found"].tolist() and idx.cpu().tolist() == g[pre + "new_idx"].tolist(), arm
        for i in range(len(ts)):
            assert caps[i] == g["grid_abl_%s_cap_%d" % (arm, i)].tolist(), (arm, i)
        f = g[pre + "found"]
        orig = ablation.word_prob(eng, tr["pred"], ts, targets, row2img=[0] * len(ts)).cpu().double().numpy()
        d0 = np.abs(orig - g[pre + "orig"]).max()
        assert np.isnan(prob.cpu().numpy()[~f]).all()
        d1 = np.abs(prob.cpu().double().numpy()[f] - (g[pre + "orig"] - g[pre + "diff"])[f]).max() if f.any() else 0.0
        print("gridTD image ablation, %s arm: %d rows (%d found), original score %.2e, new score %.2e (bound %.2e)" % (arm, len(ts), f.sum(), d0, d1, tol))
        assert d0 < tol and d1 < tol
        branches |= set(f.tolist())
    assert branches == {True, False}
    # (e) word ablation, random arm: the drawn positions
    ts, ids = g["grid_abl_wrd_t"].tolist(), torch.from_numpy(g["grid_abl_wrd_ids"])
    R = len(ts)
    captions = torch.tensor([caption] * R)
    short, lens = ablation.delete_tokens(eng, captions, ts, ids)
    for i in range(R):
        assert short[i, :lens[i]].cpu().tolist() == g["grid_abl_wrd_short_%d" % i].tolist(), i
    new = ablation.word_ablation(eng, enc, [0] * R, captions, ts, torch.zeros(R, T), model_bias=ex.TF_MODEL_BIAS, delete_ids=ids)
    d2 = np.abs(new.cpu().double().numpy() - (g["grid_abl_wrd_orig"] - g["grid_abl_wrd_diff"])).max()
    print("gridTD word ablation, random arm: %d rows, new score %.2e (bound %.2e)" % (R, d2, tol))
    assert d2 < tol


def test_aoa_arms_vs_the_references_own_experiments():
    _need_gpu()
    from lrp_amd import evaluation, ops, weights
    from lrp_amd.explainers import attention_maps
    from lrp_amd.explainers.aoa import ExplainAOAAttention
    g = _golden()
    V, seed, factor, head = int(g["aoa_V"]), int(g["aoa_seed"]), float(g["aoa_factor"]), int(g["aoa_head"])
    sd = weights.sharpen_attention(weights.make_aoa_state(seed=seed, vocab_size=V), factor)
    wm = weights.make_word_map(V)
    wm['<end>'] = int(g["aoa_end"])
    img = torch.from_numpy(weights.make_images(seed + 7, 1)).cuda()
    ex = ExplainAOAAttention(_args(), wm, model=sd)
    ex.get_hidden_parameters(img)
    caption = [int(c) for c in ex.beam_caption_encode]
    assert caption == g["aoa_caption"].tolist()
    eng = ex.engine
    tr = eng.trace(eng.encode(img), torch.tensor([caption], dtype=torch.int64, device="cuda"), predictions=False)
    a_ref = g["aoa_alphas"].astype(np.float64)
    rel = float((np.abs(tr["alpha"][0].cpu().double().numpy() - a_ref) / a_ref.max(axis=2, keepdims=True)).max())
    print("AoA: alpha within %.2e of a row's largest" % rel)
    # maps of the reference's own alphas: one head, and the mean over the heads
    ga = torch.from_numpy(g["aoa_alphas"]).cuda()
    ts, heads = g["aoa_box_att_t"].tolist(), g["aoa_box_att_head"].tolist()
    n = heads.index(-1)
    assert heads == [head] * n + [-1] * (len(heads) - n)
    norm = torch.cat([ops.expand_maps(ga[ts[:n]].contiguous(), 224, head=head, normalize=True),
                      ops.expand_maps(ga[ts[n:]].contiguous(), 224, normalize=True)])
    refs = [_ref_map(g["aoa_alphas"][t][h] if h >= 0 else np.mean(g["aoa_alphas"][t], axis=0)) for t, h in zip(ts, heads)]
    _check_maps(norm, refs, g["aoa_box_att_bound"], "AoA attention maps")
    row = int(g["aoa_map_row"])
    assert float(np.abs(norm[row].cpu().double().numpy() - g["aoa_map_full"]).max()) <= g["aoa_box_att_bound"][row] + 2.0 ** -24
    _check_boxes(g, "aoa_box_att_", norm, "AoA attention bbox")
    # masks from the engine's own alphas
    for h in (head, -1):
        sel = np.flatnonzero(g["aoa_mask_head"] == h)
        if len(sel) == 0:
            continue
        own = attention_maps(eng, tr, head=None if h < 0 else h)[g["aoa_mask_t"][sel].tolist()]
        mask = evaluation.block_image(own)
        assert np.array_equal(mask[:, ::8, ::8].cpu().numpy().astype(np.uint8), g["aoa_mask_mask"][sel]), h
