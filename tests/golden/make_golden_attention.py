#!/usr/bin/env python3
"""Golden vectors of the OTHER arms of the reference's experiments - the model's own attention, Grad-CAM and chance - run by the reference
itself (CPU, the harness shims of make_golden.py / make_golden_ablation.py) on seeded models whose attention was sharpened
(`weights.sharpen_attention`: gridTD x 64, AoA x 256; random-init attention is uniform to a few percent and its top-20 patches are decided
by rounding).  `skimage.transform.pyramid_expand` is served by `oracle.pyramid_expand` as in make_golden.py: scikit-image is not available,
that one function stays pinned to its restatement only.

gridTD (`ExplainGridTDAttention`, and `ExplainGridTDGradCam` on the same weights), one image, the reference's own beam-search caption under
a word map whose <end> is the first new word at position 10 or later of the natural caption (a short caption; words can disappear from
the re-captioned masked images):

  `EvaluationExperiments.ablation_experiment(do_attention=True)` (evaluation.py:82-311) with every caption word an object word: per word
      t >= 1 the attention arm (:198-233) and the random arm (:159-197) of the image ablation, per word t >= 6 the random arm of the word
      ablation (:265-287).  `random.sample` is wrapped to record what was drawn.
  `bbox_experiment(explanation_type='lrp', do_attention=True)` and `('GradCam')` (:345-448) on a synthetic `category_dict`: three caption
      words, with 2, 1 and 3 boxes - the in-place cut of `_calculate_overlaped_pixels` (:324-326) carries over to a word's later boxes.
      The gradient family captions with beam 3 (models/gridTDmodel.py:1325): the Grad-CAM run has a caption and categories of its own.
  `tpfp_experiment(do_attention=True)` (:450-573): two frequent words, one of them in the reference captions.

AoA (`ExplainAOAAttention`): `EvaluationExperimentsAOA.bbox_experiment_attention(head_idx)` (:720-771, one head) and the head-mean path
(`np.mean(attention, axis=0)`, :391-393) through `EvaluationExperiments.bbox_experiment(do_attention=True)`; the reference's `block_image`
on those maps gives the masks.

Writes tests/golden/attention_arms.npz - arrays only.  Per model prefix (`grid_`, `aoa_`): seed, V, end, factor, caption, alphas (T, P) or
(T, NH, P), betas (T,).  Per experiment a table of rows; a row is an (explained word t, category) match or an explained word:

  grid_abl_*: att_t, att_gap (20th against 21st patch sum of the reference's map, relative to the largest), att_mask (rows, 28, 28) uint8,
      att_sums (rows, 28, 28) float64, att_found, att_new_idx, att_orig, att_diff, att_cap_<i>; the same for rnd_ on at most two rows, with
      rnd_perm (rows, 50176) uint16 - the drawn permutation, its patch sums are integers below 2^24 and exact in fp32: every row with a
      non-zero gap is kept; wrd_t, wrd_ids (rows, 3), wrd_orig, wrd_diff, wrd_short_<i>; absmax (largest |score| of any teacher-forced call).
      Attention rows whose gap is below 1e-3 are not stored.
  <model>_box_<arm>_*: t (rows,), head (AoA: -1 is the mean), nbox (rows,), boxes (sum nbox, 4) pixel boxes, table (sum nbox, 10): the score
      of every (box, threshold) call in the reference's order, best (rows, 10): the running maximum the reference keeps, started at 0,
      sens (sum nbox, 10), bound (rows,): see below.  Arms: att (attention), cam (Grad-CAM, with cams (rows, 196) and caption: the
      gradient family's own beam-3 caption), lrp (table and best
      only: for the record).
  grid_tpfp_*: t, tp (bool), att_mean, att_max, att_quantile (rows, 100), one_minus_beta, bound (rows,); lrp_stats (rows, 4), lrp_quantile.
  <model>_map_full (H, W) float32 and _map_row: the reference's own normalised map of one attention row, whole; every other map is
      `_project_maxabs(oracle.pyramid_expand(.))` of the stored alphas / cams - asserted here to be the array the reference used, bit for bit.
  aoa_mask_*: t, head, gap, mask, sums of the AoA rows with a gap >= 1e-3.

bound (per row): what `lrpx_expand_maps` may deviate from the reference's map, tests/test_gpu_expand_maps.py: raw (2 p + 4) 2^-24 max|a|,
normalised 2 raw / max|E_ref| + 2^-24.  sens (per ratio): the largest change of that ratio when every pixel of the reference's map moves by
up to `bound` - pixels within `bound` of the effective threshold may enter or leave, all others move by `bound`:
(dI + dS) / (S - dS), capped at 1; computed from the reference's map alone.

    python tests/golden/make_golden_attention.py [--first-seed N]

Conditions on the draw, searched from --first-seed: at least 4 stored attention image-ablation rows on gridTD, both branches (word found,
word gone) among the stored attention and random rows, at least one word with two boxes among the bbox rows of each model.
Run where the reference is available only.

Printed by the run that wrote the committed file:
    grid seed 0: caption of 11 words; attention image rows 8 (found 8, gone 0), random image rows 2 (found 2, gone 0), random word rows 5;
        bbox rows 7 (4 with several boxes), Grad-CAM rows 8 (0 all-zero); tpfp rows 5 (TP 2)          [no word gone: next seed]
    grid seed 1: caption of 12 words; attention image rows 10 (found 4, gone 6), random image rows 2 (found 1, gone 1), random word rows 6;
        bbox rows 4 (2 with several boxes), Grad-CAM rows 3 (1 all-zero); tpfp rows 3 (TP 1)
    aoa seed 0: caption of 10 words; bbox rows 8 (head 5 and the mean; 6 with several boxes); mask rows 6
    attention_arms.npz: 736265 bytes"""
import argparse
import os
import random as _random
import sys
import tempfile
import types

import numpy as np
import torch

from make_golden import install_stubs, load_pkg, make_args, ref_vgg_patch, to_torch_sd
from make_golden_ablation import patch_gap, patch_sums

HERE = os.path.dirname(os.path.abspath(__file__))
GAP = 1e-3
U = 2.0 ** -24
THR = [0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]
# boxes in the coordinates of a 448 x 448 original, resize_ratio 0.5 (evaluation.py:420-424 truncates): 2, 1 and 3 boxes
BOXES = [[[41, 61, 241, 281], [199, 181, 421, 401]], [[101, 21, 349, 301]], [[9, 9, 151, 201], [251, 31, 439, 221], [121, 241, 331, 441]]]
RATIO = (0.5, 0.5)
DRAWS = []


class _Random(object):
    """the `random` module as evaluation.py sees it: `sample` records what it returns"""

    def __getattr__(self, name):
        return getattr(_random, name)

    @staticmethod
    def sample(population, k):
        out = _random.sample(population, k)
        DRAWS.append(list(out))
        return out


def div14_on():
    orig = torch.Tensor.__truediv__

    def div14(a, b):          # `top_words / vocab_size` is integer division in the PyTorch 1.4 the reference pins (make_golden.gen_beam)
        if torch.is_tensor(a) and not a.is_floating_point() and isinstance(b, int):
            return torch.div(a, b, rounding_mode="floor")
        return orig(a, b)
    torch.Tensor.__truediv__ = div14
    return orig


def expand_ref(a, p, upscale, normalize):
    """the reference's map of a (P,) array: pyramid_expand (the oracle's restatement, float64) and `_project_maxabs`"""
    from oracle import lrp_oracle as O
    e = O.pyramid_expand(torch.from_numpy(np.asarray(a).reshape(p, p)), upscale).double().numpy()
    raw_bound = (2 * p + 4) * U * float(np.abs(a).max())
    if not normalize:
        return e, raw_bound
    m = np.abs(e).max()
    if m == 0:
        return np.zeros(e.shape), 0.0
    return 1.0 * e / m, 2 * raw_bound / m + U


def ratio_sens(v, box, thr, b):
    """largest change of `_calculate_overlaped_pixels(box, v, thr)` when every pixel of v moves by up to b (module docstring)"""
    inside = np.zeros(v.shape, bool)
    inside[box[1]:box[3], box[0]:box[2]] = True
    above = v > thr
    border = np.abs(v - thr) <= b
    S = v[above].sum()
    moved = np.where(border, np.abs(v) + b, np.where(above, b, 0.0))
    dS, dI = moved.sum(), moved[inside].sum()
    if S - dS <= 0:
        return 1.0
    return float(min(1.0, (dI + dS) / (S - dS)))


class Groups(object):
    """Every `_project_maxabs` result of an experiment is a group: the (box, threshold, score) calls of `_calculate_overlaped_pixels`
    on that array, and a copy of the array as it was before the first call."""

    def __init__(self, ev):
        self.groups, self.by_id = [], {}
        real_p, real_c = ev._project_maxabs, ev._calculate_overlaped_pixels

        def project(x):
            out = real_p(x)
            g = dict(arr=out, clean=np.array(out, copy=True), calls=[])
            self.groups.append(g)
            self.by_id[id(out)] = g
            return out

        def overlap(bbox, relevance, threshold):
            score = real_c(bbox, relevance, threshold)
            self.by_id[id(relevance)]["calls"].append((tuple(int(b) for b in bbox), float(threshold), float(score)))
            return score
        ev._project_maxabs, ev._calculate_overlaped_pixels = project, overlap


def box_rows(groups, matches, want=None, bounds=None, extra=None):
    """groups (one per match, in order) -> the arrays of one arm.  want[i]: the clean map the group must hold, bit for bit."""
    assert len(groups) == len(matches), (len(groups), len(matches))
    out = dict(t=[], nbox=[], boxes=[], table=[], best=[], sens=[], bound=[])
    for i, (g, (t, _)) in enumerate(zip(groups, matches)):
        boxes = []
        for b, _, _ in g["calls"]:
            if b not in boxes:
                boxes.append(b)
        assert len(g["calls"]) == len(boxes) * len(THR)
        table = np.array([s for _, _, s in g["calls"]], np.float64).reshape(len(boxes), len(THR))
        assert [c[1] for c in g["calls"][:len(THR)]] == [float(x) for x in THR]
        best = np.maximum(table.max(axis=0), 0.0)
        out["t"].append(t)
        out["nbox"].append(len(boxes))
        out["boxes"] += [list(b) for b in boxes]
        out["table"].append(table)
        out["best"].append(best)
        if want is not None:
            assert np.array_equal(g["clean"], want[i]), "match %d: the reference's map is not the restated one" % i
            b = bounds[i]
            sens = np.zeros_like(table)
            for k, box in enumerate(boxes):
                for j, thr in enumerate(THR):
                    sens[k, j] = ratio_sens(g["clean"], box, thr if k == 0 else max(thr, THR[-1]), b)      # the carry
            out["sens"].append(sens)
            out["bound"].append(b)
    res = dict(t=np.array(out["t"], np.int64), nbox=np.array(out["nbox"], np.int64), boxes=np.array(out["boxes"], np.int64).reshape(-1, 4),
               table=np.concatenate(out["table"]) if out["table"] else np.zeros((0, 10)), best=np.stack(out["best"]) if out["best"] else np.zeros((0, 10)))
    if want is not None:
        res.update(sens=np.concatenate(out["sens"]), bound=np.array(out["bound"], np.float64))
    if extra:
        res.update(extra)
    return res


def category_dict(caption, wm, name):
    """three distinct caption words (t >= 1) as categories with 2, 1 and 3 boxes"""
    rev = {v: k for k, v in wm.items()}
    keys = []
    for c in caption[2:]:
        if rev[c] not in keys and not rev[c].startswith('<'):
            keys.append(rev[c])
    keys = keys[:3]
    cats = {k: i for i, k in enumerate(keys)}
    matches = [(t, rev[caption[t + 1]]) for t in range(len(caption) - 1) for k in keys if rev[caption[t + 1]] == k]
    return {name: dict(categories=cats, bbox=BOXES[:len(keys)], resize_ratio=RATIO)}, matches


def short_end(model, img, wm, beam, steps, at=10):
    """<end> := the first word at position >= `at` of the natural caption that does not occur before it"""
    _, sen = model.beam_search(torch.from_numpy(img.copy()), wm, beam_size=beam, max_cap_length=steps)
    sen = [int(w) for w in sen]
    for k in range(at, len(sen)):
        if sen[k] not in sen[:k]:
            return sen[k]
    return None


def quiet(ex, img):
    ex.preprocess_img = lambda path: torch.from_numpy(img.copy())
    ex.visualize_explanations = lambda *a, **k: None
    ex.save_linguistic_explanation = lambda *a, **k: None


def memo(fn):
    """the experiments explain the same image again and again: explain once (deterministic), hand out clones"""
    cache = {}

    def call(*a, **k):
        key = (a, tuple(sorted(k.items())))
        if key not in cache:
            cache[key] = fn(*a, **k)
        maps, rws = cache[key]
        return [m.detach().clone() for m in maps], [r.detach().clone() for r in rws]
    return call


def run_gridtd(weights, seed, factor=64.0, V=9586):
    import evaluation
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import models.gridTDmodel as gtd
    plt.show = lambda *a, **k: None
    evaluation.random = _Random()
    sd = weights.sharpen_attention(weights.make_gridtd_state(seed=seed, vocab_size=V), factor)
    wm = weights.make_word_map(V)
    img = weights.make_images(seed + 7, 1)
    model = gtd.GridTDModel(512, 512, V, 'vgg16')
    model.load_state_dict(to_torch_sd(sd))
    model.eval()
    name, data = "synthetic.jpg", dict(image_path="synthetic.jpg")
    g = {}
    orig_div = div14_on()
    try:
        with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
            end = short_end(model, img, wm, 2, 50)
        if end is None:
            return None
        wm['<end>'] = end
        rev = {v: k for k, v in wm.items()}
        with tempfile.TemporaryDirectory() as tmp:
            ex = gtd.ExplainGridTDAttention(make_args(tmp), wm, model=model)
            quiet(ex, img)
            ex.explain_caption = memo(ex.explain_caption)
            beams, forced, masks = [], [], []
            real_beam, real_tf = model.beam_search, ex.teacherforce_forward

            def beam(*a, **k):
                out = real_beam(*a, **k)
                beams.append([int(w) for w in out[1]])
                return out

            def tf(image, caption):
                pred = real_tf(image, caption)
                forced.append(([int(c) for c in caption], float(pred.detach().abs().max())))
                return pred
            model.beam_search, ex.teacherforce_forward = beam, tf
            ev = evaluation.EvaluationExperiments(ex)
            real_block = ev.block_image

            def block(rel):
                m = real_block(rel)
                masks.append((rel.detach().clone(), m.detach().clone()))
                return m
            ev.block_image = block
            ex.explain_caption(name)
            caption = [int(c) for c in ex.beam_caption_encode]
            T = len(caption) - 1
            alphas, betas = ex.alphas.detach().clone().numpy(), ex.betas.detach().clone().numpy()
            predictions = ex.predictions.detach().clone()
            evaluation.object_words_list = sorted({rev[c] for c in caption[1:]})
            evaluation.STOP_WORDS = []
            # ---- ablation: per t >= 1 three masks / captions in the order lrp, random, attention -------------------------------------------
            del beams[:], DRAWS[:]
            _random.seed(seed)
            ev.ablation_experiment(data, "lrp", tmp, do_attention=True)
            assert len(beams) == 3 * (T - 1) == len(masks), (len(beams), len(masks), T)
            perms = [d for d in DRAWS if len(d) == 224 * 224]
            ids = [d for d in DRAWS if len(d) == 3]
            assert len(perms) == T - 1 and len(ids) == max(0, T - 6)
            soft = lambda t: torch.softmax(predictions[t], dim=-1)[caption[t + 1]].item()
            g["abl_absmax"] = np.float64(max([m for _, m in forced] + [0.0]))
            for arm, off, found_l, gone_l in (("att", 2, ev.image_category_score_diff_att, ev.image_disappear_count_att),
                                              ("rnd", 1, ev.image_category_score_diff_random, ev.image_disappear_count_random)):
                found = {int(t): d for t, _, d in found_l}
                gone = {int(t) for t, _ in gone_l}
                assert sorted(list(found) + list(gone)) == list(range(1, T))
                rows = dict(t=[], gap=[], mask=[], sums=[], found=[], idx=[], orig=[], diff=[], perm=[])
                order = list(range(1, T))
                if arm == "rnd":          # at most two rows (a permutation is 100 KB): one of each branch where there is one
                    order = ([t for t in order if t in gone][:1] + [t for t in order if t in found][:2])[:2]
                for t in order:
                    rel, mask = masks[3 * (t - 1) + off]
                    new = beams[3 * (t - 1) + off]
                    gap = patch_gap(rel.double())
                    if arm == "att":
                        want, _ = expand_ref(alphas[t], 14, 16, True)
                        assert np.array_equal(rel.numpy(), want), "attention map of word %d is not the restated one" % t
                    else:
                        assert rel.flatten().tolist() == perms[t - 1]
                    if gap < (GAP if arm == "att" else 1e-12):
                        continue
                    w = caption[t + 1]
                    assert (t in found) == (w in new)
                    g["abl_%s_cap_%d" % (arm, len(rows["t"]))] = np.array(new, np.int64)
                    rows["t"].append(t); rows["gap"].append(gap)
                    rows["mask"].append(mask[::8, ::8].numpy().astype(np.uint8)); rows["sums"].append(patch_sums(rel.double()))
                    rows["found"].append(t in found); rows["idx"].append(new.index(w) if t in found else -1)
                    rows["orig"].append(soft(t)); rows["diff"].append(found.get(t, float("nan")))
                    if arm == "rnd":
                        rows["perm"].append(np.array(perms[t - 1], np.uint16))
                n = len(rows["t"])
                g.update({"abl_%s_t" % arm: np.array(rows["t"], np.int64), "abl_%s_gap" % arm: np.array(rows["gap"], np.float64),
                          "abl_%s_mask" % arm: np.stack(rows["mask"]) if n else np.zeros((0, 28, 28), np.uint8),
                          "abl_%s_sums" % arm: np.stack(rows["sums"]) if n else np.zeros((0, 28, 28)),
                          "abl_%s_found" % arm: np.array(rows["found"], np.bool_), "abl_%s_new_idx" % arm: np.array(rows["idx"], np.int64),
                          "abl_%s_orig" % arm: np.array(rows["orig"], np.float64), "abl_%s_diff" % arm: np.array(rows["diff"], np.float64)})
                if arm == "rnd":
                    g["abl_rnd_perm"] = np.stack(rows["perm"]) if n else np.zeros((0, 224 * 224), np.uint16)
            diffs = {int(t): v[0] for t, v in ev.category_scores_diff_random.items()}
            assert sorted(diffs) == list(range(6, T))
            shorts = [c for c, _ in forced]
            wt = list(range(6, T))
            for i, t in enumerate(wt):
                short = np.delete(np.array(caption[:t + 1]), ids[i]).tolist()
                assert short in shorts and all(1 <= d < t for d in ids[i])
                g["abl_wrd_short_%d" % i] = np.array(short, np.int64)
            g.update(abl_wrd_t=np.array(wt, np.int64), abl_wrd_ids=np.array(ids, np.int64).reshape(-1, 3),
                     abl_wrd_orig=np.array([soft(t) for t in wt], np.float64), abl_wrd_diff=np.array([diffs[t] for t in wt], np.float64))
            # ---- bbox, 'lrp' with attention: per match the attention group, then the LRP group ---------------------------------------------
            cat, matches = category_dict(caption, wm, name)
            ev = evaluation.EvaluationExperiments(ex)
            gr = Groups(ev)
            ev.bbox_experiment(cat, data, tmp, explanation_type='lrp', do_attention=True)
            maps = [expand_ref(alphas[t], 14, 16, True) for t, _ in matches]
            att = box_rows(gr.groups[0::2], matches, [m for m, _ in maps], [b for _, b in maps])
            lrp = box_rows(gr.groups[1::2], matches)
            g.update({"box_att_" + k: v for k, v in att.items()})
            g.update({"box_lrp_" + k: v for k, v in lrp.items() if k in ("t", "table", "best")})
            if matches:
                g["map_full"], g["map_row"] = maps[0][0].astype(np.float32), np.int64(0)          # (a row of box_att)
            # ---- tpfp: the first two categories are the frequent words, the first of them is in the reference captions ----------------------
            keys = list(cat[name]["categories"])
            ev = evaluation.EvaluationExperiments(ex)
            ref_caps = [[wm['<start>'], wm[keys[0]], wm['<end>']]] if keys else [[wm['<start>'], wm['<end>']]]
            ev.tpfp_experiment(dict(image_path=name, encoded_all_caps=ref_caps), "lrp", tmp, keys[:2], True)
            rows = dict(t=[], tp=[], mean=[], mx=[], q=[], omb=[], bound=[], ls=[], lq=[])
            it = {True: [iter(ev.TP_statistics), iter(ev.TP_statistics_att), iter(ev.TP_statistics_beta)],
                  False: [iter(ev.FP_statistics), iter(ev.FP_statistics_att), iter(ev.FP_statistics_beta)]}
            for t in range(T):
                w = rev[caption[t + 1]]
                if w not in keys[:2]:
                    continue
                tp = w == keys[0]
                st, sa, sb = [next(i) for i in it[tp]]
                assert st["word"] == sa["word"] == sb["word"] == w
                raw, b = expand_ref(alphas[t], 14, 16, False)
                assert float(sa["mean"]) == float(np.mean(raw)) and float(sa["max"]) == float(np.max(raw))
                rows["t"].append(t); rows["tp"].append(tp); rows["mean"].append(float(sa["mean"])); rows["mx"].append(float(sa["max"]))
                rows["q"].append([float(x) for x in sa["quantile"]]); rows["omb"].append(float(sb["1-beta"])); rows["bound"].append(b)
                rows["ls"].append([float(st[k]) for k in ("mean", "mean_abs", "mean_pos", "max")]); rows["lq"].append([float(x) for x in st["quantile"]])
            g.update(tpfp_t=np.array(rows["t"], np.int64), tpfp_tp=np.array(rows["tp"], np.bool_), tpfp_att_mean=np.array(rows["mean"]),
                     tpfp_att_max=np.array(rows["mx"]), tpfp_att_quantile=np.array(rows["q"]).reshape(-1, 100),
                     tpfp_one_minus_beta=np.array(rows["omb"]), tpfp_bound=np.array(rows["bound"]),
                     tpfp_lrp_stats=np.array(rows["ls"]).reshape(-1, 4), tpfp_lrp_quantile=np.array(rows["lq"]).reshape(-1, 100))
            # ---- bbox, 'GradCam' -----------------------------------------------------------------------------------------------------------
            real_load = torch.load
            torch.load = lambda *a, **k: {"state_dict": to_torch_sd(sd)}
            try:
                ex2 = gtd.ExplainGridTDGradCam(make_args(tmp), wm)
            finally:
                torch.load = real_load
            quiet(ex2, img)
            ex2.explain_caption = memo(ex2.explain_caption)
            cams_all, _ = ex2.explain_caption(name)
            caption2 = [int(c) for c in ex2.beam_caption_encode]          # the gradient family captions with beam 3 (:1325): a caption of its own
            cat, matches = category_dict(caption2, wm, name)          # ... and categories of its own: its first three distinct words
            ev = evaluation.EvaluationExperiments(ex2)
            gr = Groups(ev)
            ev.bbox_experiment(cat, data, tmp, explanation_type='GradCam', do_attention=False)
            cams = [cams_all[t].numpy().reshape(-1).astype(np.float32) for t, _ in matches]
            maps = [expand_ref(c, 14, 16, True) for c in cams]
            cam = box_rows(gr.groups, matches, [m for m, _ in maps], [b for _, b in maps],
                           extra=dict(cams=np.stack(cams) if cams else np.zeros((0, 196), np.float32), caption=np.array(caption2, np.int64)))
            g.update({"box_cam_" + k: v for k, v in cam.items()})
    finally:
        torch.Tensor.__truediv__ = orig_div
    g.update(seed=np.int64(seed), V=np.int64(V), end=np.int64(end), factor=np.float64(factor), caption=np.array(caption, np.int64),
             alphas=alphas.astype(np.float32), betas=betas.astype(np.float32))
    return g


def run_aoa(weights, seed, factor=256.0, V=11027, head=5):
    import evaluation
    import models.aoamodel as aoa
    sd = weights.sharpen_attention(weights.make_aoa_state(seed=seed, vocab_size=V), factor)
    wm = weights.make_word_map(V)
    img = weights.make_images(seed + 7, 1)
    model = aoa.AOAModel(512, 512, 8, V, 'vgg16')
    model.load_state_dict(to_torch_sd(sd))
    model.eval()
    name, data = "synthetic.jpg", dict(image_path="synthetic.jpg")
    g = {}
    orig_div = div14_on()
    try:
        with torch.no_grad():
            end = short_end(model, img, wm, 3, 20)
        if end is None:
            return None
        wm['<end>'] = end
        with tempfile.TemporaryDirectory() as tmp:
            ex = aoa.ExplainAOAAttention(make_args(tmp), wm, model=model)
            quiet(ex, img)
            # one head: the attention-only experiment (no relevance is computed)
            ev = evaluation.EvaluationExperimentsAOA(ex)
            gr = Groups(ev)
            ex.get_hidden_parameters(name)
            caption = [int(c) for c in ex.beam_caption_encode]
            cat, matches = category_dict(caption, wm, name)
            ev.bbox_experiment_attention(cat, data, tmp, head)
            alphas = ex.alphas.detach().clone().numpy()
            assert alphas.shape[1:] == (8, 196)
            maps = [expand_ref(alphas[t][head], 14, 16, True) for t, _ in matches]
            one = box_rows(gr.groups, matches, [m for m, _ in maps], [b for _, b in maps])
            # the mean over the heads: the base class's experiment on this explainer (its explain_caption takes the head to explain)
            real_explain = ex.explain_caption
            ex.explain_caption = memo(lambda path: real_explain(path, head))
            ev = evaluation.EvaluationExperiments(ex)
            gr = Groups(ev)
            ev.bbox_experiment(cat, data, tmp, explanation_type='lrp', do_attention=True)
            assert [int(c) for c in ex.beam_caption_encode] == caption
            means = [np.mean(alphas[t], axis=0) for t, _ in matches]
            maps2 = [expand_ref(a, 14, 16, True) for a in means]
            mean = box_rows(gr.groups[0::2], matches, [m for m, _ in maps2], [b for _, b in maps2])
            for k in one:
                g["box_att_" + k] = np.concatenate([one[k], mean[k]])
            g["box_att_head"] = np.array([head] * len(matches) + [-1] * len(matches), np.int64)
            if matches:
                g["map_full"], g["map_row"] = maps2[0][0].astype(np.float32), np.int64(len(matches))
            # the reference's block_image on these maps
            rows = dict(t=[], head=[], gap=[], mask=[], sums=[])
            for hd, ms in ((head, maps), (-1, maps2)):
                seen = set()
                for (t, _), (m, _) in zip(matches, ms):
                    rel = torch.from_numpy(m)
                    if t in seen or patch_gap(rel) < GAP:
                        continue
                    seen.add(t)
                    rows["t"].append(t); rows["head"].append(hd); rows["gap"].append(patch_gap(rel))
                    rows["mask"].append(ev.block_image(rel)[::8, ::8].numpy().astype(np.uint8)); rows["sums"].append(patch_sums(rel))
            n = len(rows["t"])
            g.update(mask_t=np.array(rows["t"], np.int64), mask_head=np.array(rows["head"], np.int64), mask_gap=np.array(rows["gap"]),
                     mask_mask=np.stack(rows["mask"]) if n else np.zeros((0, 28, 28), np.uint8),
                     mask_sums=np.stack(rows["sums"]) if n else np.zeros((0, 28, 28)))
    finally:
        torch.Tensor.__truediv__ = orig_div
    g.update(seed=np.int64(seed), V=np.int64(V), end=np.int64(end), factor=np.float64(factor), caption=np.array(caption, np.int64),
             alphas=alphas.astype(np.float32), head=np.int64(head))
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-seed", type=int, default=0)
    ap.add_argument("--tries", type=int, default=4)
    a = ap.parse_args()
    install_stubs()
    weights = load_pkg()
    ref_vgg_patch()
    from oracle import lrp_oracle as O
    expand = lambda x, upscale=2, multichannel=False, **kw: O.pyramid_expand(torch.from_numpy(np.asarray(x)), upscale).double().numpy()
    sys.modules["skimage.transform"].pyramid_expand = expand
    sys.modules["skimage"].transform = sys.modules["skimage.transform"]
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.show = lambda *a, **k: None
    out = {}
    for tag, run in (("grid", run_gridtd), ("aoa", run_aoa)):
        for seed in range(a.first_seed, a.first_seed + a.tries):
            g = run(weights, seed)
            if g is None:
                print("%s seed %d: no short caption" % (tag, seed), flush=True)
                continue
            two = int((g["box_att_nbox"] >= 2).sum())
            if tag == "grid":
                fa, fr = g["abl_att_found"], g["abl_rnd_found"]
                print("grid seed %d: caption of %d words; attention image rows %d (found %d, gone %d), random image rows %d (found %d, gone %d), "
                      "random word rows %d; bbox rows %d (%d with several boxes), Grad-CAM rows %d (%d all-zero); tpfp rows %d (TP %d)" % (
                          seed, len(g["caption"]) - 1, len(fa), fa.sum(), (~fa).sum(), len(fr), fr.sum(), (~fr).sum(), len(g["abl_wrd_t"]),
                          len(g["box_att_t"]), two, len(g["box_cam_t"]), int((np.abs(g["box_cam_cams"]).max(axis=1) == 0).sum()) if len(g["box_cam_t"]) else 0,
                          len(g["tpfp_t"]), g["tpfp_tp"].sum()), flush=True)
                both = set(fa.tolist()) | set(fr.tolist())
                ok = len(fa) >= 4 and both == {True, False} and two >= 1
            else:
                print("aoa seed %d: caption of %d words; bbox rows %d (head %d and the mean; %d with several boxes); mask rows %d" % (
                    seed, len(g["caption"]) - 1, len(g["box_att_t"]), int(g["head"]), two, len(g["mask_t"])), flush=True)
                ok = two >= 1 and len(g["mask_t"]) >= 4
            if ok:
                out.update({"%s_%s" % (tag, k): v for k, v in g.items()})
                break
        else:
            raise SystemExit("no %s seed met the conditions" % tag)
    path = os.path.join(HERE, "attention_arms.npz")
    np.savez_compressed(path, **out)
    print("attention_arms.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
