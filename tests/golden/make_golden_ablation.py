#!/usr/bin/env python3
"""Golden vectors of the reference's central quantitative experiment, `EvaluationExperiments.ablation_experiment(..., do_attention=False)`
(evaluation.py:82-311), run by the reference itself on the seeded gridTD model and `ExplainGridTDAttention` (CPU, the harness shims of
make_golden.py).  The image is captioned by the reference's own `beam_search` (beam 2 / 50 steps, models/gridTDmodel.py:935), explained
word by word, and then

  image ablation (:120-156): for every object word at t >= 1 the 20 most relevant 8 x 8 patches are masked, the masked image is captioned
      again (`beam_search`, beam 3 / 20 steps), and where the word is still there the prefix before it is teacher-forced;
  word ablation (:234-253): for every stop or object word at t >= 6 the three most relevant preceding words are deleted and the
      shortened caption is teacher-forced.

`evaluation.object_words_list` is set to EVERY word of the synthetic caption, `evaluation.STOP_WORDS` stays empty: every t >= 1 is an
image-ablation row and every t >= 6 a word-ablation row.  Rows whose selection rests on a gap below 1e-3 of the largest value - between the
20th and 21st patch sum, or between the 3rd and 4th word relevance - are not stored (the maps agree with the reference to the 1e-4 grade:
such a selection would test rounding).

Writes tests/golden/ablation.npz - arrays only:

  seed, V, cases (the prefixes below: "a" the synthetic word map, "b" the same with <end> := a word the model produces);
  per case <c>_: caption (incl. <start>), end (the <end> id), absmax (the largest |score| of any teacher-forced call: the scale of the
      tolerance);
  img_t, img_found, img_new_idx (-1: the word is gone), img_orig / img_diff (the original probability and original - new; NaN where the
      word is gone), img_mask (rows, 28, 28) uint8 (the mask at every 8th pixel: it is constant on a patch), img_gap (the measured gap /
      largest), img_patch_sums (rows, 28, 28) float64 (the reference map's sum over each patch), img_cap_<i>: the new caption (`sen_idx`) of row i;
  word_t, word_deleted (rows, 3: the dropped positions, most relevant first), word_orig, word_diff, word_gap, word_short_<i>: the
      shortened caption the reference teacher-forced.

    python tests/golden/make_golden_ablation.py [--first-seed N]

Conditions on the draw, searched from --first-seed: at least three word-ablation rows, at least one image-ablation row of each branch
(word found, word gone).  Random-init weights put the same few words into every caption, so no word disappears by itself: case "b"
re-runs the experiment under a word map whose <end> is a word that comes early in the masked images' captions and late in the explained one.  Run where the reference is available only."""
import argparse
import os
import tempfile

import numpy as np
import torch

from make_golden import install_stubs, load_pkg, make_args, ref_vgg_patch, to_torch_sd

HERE = os.path.dirname(os.path.abspath(__file__))
V = 9586
GAP = 1e-3


def patch_sums(spatial, patch=8):
    s = spatial.double().numpy()
    h, w = s.shape
    return s.reshape(h // patch, patch, w // patch, patch).sum(axis=(1, 3))


def patch_gap(spatial, k=20):
    sums = np.sort(patch_sums(spatial).ravel())[::-1]
    return float((sums[k - 1] - sums[k]) / np.abs(sums).max())


def word_gap(rw, k=3):
    v = np.sort(rw[1:].double().numpy())[::-1]
    if len(v) <= k:
        return 1.0
    return float((v[k - 1] - v[k]) / np.abs(v).max())


def run(weights, seed, end_id=None):
    import evaluation
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import models.gridTDmodel as gtd
    plt.show = lambda *a, **k: None
    sd = weights.make_gridtd_state(seed=seed, vocab_size=V)
    wm = weights.make_word_map(V)
    if end_id is not None:
        wm['<end>'] = int(end_id)          # <end> := a word the model produces, as make_golden.py's gen_beam does
    img = weights.make_images(seed + 7, 1)
    model = gtd.GridTDModel(512, 512, V, 'vgg16')
    model.load_state_dict(to_torch_sd(sd))
    orig_div = torch.Tensor.__truediv__

    def div14(a, b):          # `top_words / vocab_size` (:444) is integer division in the PyTorch 1.4 the reference pins
        if torch.is_tensor(a) and not a.is_floating_point() and isinstance(b, int):
            return torch.div(a, b, rounding_mode="floor")
        return orig_div(a, b)
    beams, forced = [], []
    with tempfile.TemporaryDirectory() as tmp:
        ex = gtd.ExplainGridTDAttention(make_args(tmp), wm, model=model)
        ex.preprocess_img = lambda path: torch.from_numpy(img.copy())
        ex.visualize_explanations = lambda *a, **k: None
        ex.save_linguistic_explanation = lambda *a, **k: None
        real_beam, real_tf = model.beam_search, ex.teacherforce_forward

        def beam(*a, **k):
            out = real_beam(*a, **k)
            beams.append([int(w) for w in out[1]])
            return out

        def tf(image, caption):
            pred = real_tf(image, caption)
            forced.append(([int(c) for c in caption], pred.detach().clone()))
            return pred
        model.beam_search, ex.teacherforce_forward = beam, tf
        ev = evaluation.EvaluationExperiments(ex)
        masks = []
        real_block = ev.block_image

        def block(rel):
            m = real_block(rel)
            masks.append((rel.detach().clone(), m.detach().clone()))
            return m
        ev.block_image = block
        torch.Tensor.__truediv__ = div14
        try:
            # first pass of the explainer alone: the caption decides the word lists
            ex.explain_caption("synthetic.jpg")
            caption = [int(c) for c in ex.beam_caption_encode]
            rev = {v: k for k, v in wm.items()}
            evaluation.object_words_list = sorted({rev[c] for c in caption[1:]})
            evaluation.STOP_WORDS = []
            del beams[:]
            ev.ablation_experiment(dict(image_path="synthetic.jpg"), "lrp", tmp, do_attention=False)
        finally:
            torch.Tensor.__truediv__ = orig_div
        predictions = ex.predictions.detach().clone()
    T = len(caption) - 1
    assert beams[0] == caption[1:], "the experiment's own caption differs from the first pass"
    new_caps = beams[1:]
    assert len(new_caps) == len(masks) == T - 1, (len(new_caps), len(masks), T)
    found = {int(t): d for t, _, d in ev.image_category_score_diff}
    gone = {int(t) for t, _ in ev.image_disappear_count}
    assert sorted(list(found) + list(gone)) == list(range(1, T))
    g = dict(caption=np.array(caption, np.int64), end=np.int64(wm['<end>']),
             absmax=np.float64(max([p.abs().max().item() for _, p in forced] + [0.0])))
    soft = lambda t: torch.softmax(predictions[t], dim=-1)[caption[t + 1]].item()
    rows = dict(t=[], found=[], idx=[], orig=[], diff=[], mask=[], gap=[], sums=[])
    for i, t in enumerate(range(1, T)):
        gap = patch_gap(masks[i][0])
        if gap < GAP:
            continue
        w = caption[t + 1]
        g["img_cap_%d" % len(rows["t"])] = np.array(new_caps[i], np.int64)
        rows["t"].append(t)
        rows["found"].append(t in found)
        rows["idx"].append(new_caps[i].index(w) if t in found else -1)
        rows["orig"].append(soft(t))
        rows["diff"].append(found.get(t, float("nan")))
        rows["mask"].append(masks[i][1][::8, ::8].numpy().astype(np.uint8))
        rows["gap"].append(gap)
        rows["sums"].append(patch_sums(masks[i][0]))
        assert (t in found) == (w in new_caps[i])
    g.update(img_t=np.array(rows["t"], np.int64), img_found=np.array(rows["found"], np.bool_), img_new_idx=np.array(rows["idx"], np.int64),
             img_orig=np.array(rows["orig"], np.float64), img_diff=np.array(rows["diff"], np.float64),
             img_mask=np.stack(rows["mask"]) if rows["mask"] else np.zeros((0, 28, 28), np.uint8), img_gap=np.array(rows["gap"], np.float64),
             img_patch_sums=np.stack(rows["sums"]) if rows["sums"] else np.zeros((0, 28, 28)))
    # word ablation: the teacher-forced calls on the UNMASKED image are the shortened captions, in the order of t
    diffs = {int(t): v[0] for t, v in ev.category_scores_diff.items()}
    assert sorted(diffs) == list(range(6, T)), (sorted(diffs), T)
    n_img_tf = sum(1 for t in range(1, T) if t in found)
    # the calls interleave per t (:120 before :234): pick the word-ablation ones by their length, t + 1 - 3 tokens on a caption prefix
    wt, wdel, worig, wdiff, wgap = [], [], [], [], []
    rel_words = RELEVANCE_WORDS[0]
    k = 0
    for t in range(1, T):
        k += 1 if t in found else 0
        if t < 6:
            continue
        short = forced[k][0]
        k += 1
        rw = rel_words[t]
        assert rw.shape[0] == t + 1 and len(short) == t + 1 - 3
        top = (torch.topk(rw[1:], k=3)[1] + 1).tolist()
        assert short == [c for p, c in enumerate(caption[:t + 1]) if p not in top]
        gap = word_gap(rw)
        if gap < GAP:
            continue
        g["word_short_%d" % len(wt)] = np.array(short, np.int64)
        g["word_rw_%d" % len(wt)] = rw.numpy().astype(np.float32)
        wt.append(t)
        wdel.append(top)
        worig.append(soft(t))
        wdiff.append(diffs[t])
        wgap.append(gap)
    assert k == len(forced) == n_img_tf + max(0, T - 6)
    g.update(word_t=np.array(wt, np.int64), word_deleted=np.array(wdel, np.int64).reshape(-1, 3), word_orig=np.array(worig, np.float64),
             word_diff=np.array(wdiff, np.float64), word_gap=np.array(wgap, np.float64))
    return g, new_caps


RELEVANCE_WORDS = [None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-seed", type=int, default=0)
    ap.add_argument("--tries", type=int, default=4)
    a = ap.parse_args()
    install_stubs()
    weights = load_pkg()
    ref_vgg_patch()
    import models.gridTDmodel as gtd
    real = gtd.ExplainGridTDAttention.explain_caption

    def keep(self, *args, **kw):          # the experiment reads `relevance_previous_words` from this call: keep what it saw
        maps, rws = real(self, *args, **kw)
        RELEVANCE_WORDS[0] = [r.detach().clone() for r in rws]
        return maps, rws
    gtd.ExplainGridTDAttention.explain_caption = keep
    for seed in range(a.first_seed, a.first_seed + a.tries):
        ga, new_caps = run(weights, seed)
        nf, ng, nw = int(ga["img_found"].sum()), int((~ga["img_found"]).sum()), len(ga["word_t"])
        print("seed %d: image rows found %d gone %d, word rows %d" % (seed, nf, ng, nw), flush=True)
        cases = {"a": ga}
        if ng == 0:
            # random weights put the same few words into every caption: no word disappears.  <end> := a word that comes early in the masked
            # images' captions (beam 3) and late in the explained one (beam 2): words before it in the explained caption are then gone
            cap, new = [int(c) for c in ga["caption"][1:]], new_caps[0]
            for e in sorted(set(new), key=new.index):
                po = cap.index(e) if e in cap else len(cap)
                if po >= 2 and any(w not in new[:new.index(e)] for w in cap[1:po]):
                    gb, _ = run(weights, seed, end_id=e)
                    print("   <end> := %d: image rows found %d gone %d, word rows %d" % (
                        e, int(gb["img_found"].sum()), int((~gb["img_found"]).sum()), len(gb["word_t"])), flush=True)
                    if int((~gb["img_found"]).sum()) >= 1:
                        cases["b"] = gb
                        break
        nf = sum(int(c["img_found"].sum()) for c in cases.values())
        ng = sum(int((~c["img_found"]).sum()) for c in cases.values())
        nw = sum(len(c["word_t"]) for c in cases.values())
        if nf >= 1 and ng >= 1 and nw >= 3:
            g = dict(seed=np.int64(seed), V=np.int64(V), cases=np.array(sorted(cases)))
            for tag, c in cases.items():
                g.update({"%s_%s" % (tag, k): v for k, v in c.items()})
            path = os.path.join(HERE, "ablation.npz")
            np.savez_compressed(path, **g)
            print("ablation.npz:", os.path.getsize(path), "bytes;", {k: getattr(v, "shape", v) for k, v in g.items() if not k[-1].isdigit()})
            return
    raise SystemExit("no seed gave both image-ablation branches and three word-ablation rows")


if __name__ == "__main__":
    main()
