"""tests/golden/ablation.npz (the reference's own ablation experiment, tests/golden/make_golden_ablation.py) is consistent with itself:
both image-ablation branches are there, the selections rest on the gaps the file records, and the two selection rules restated in numpy
on the stored inputs give the stored selections.  No GPU."""
import os

import numpy as np

from conftest import GOLDEN


def _golden():
    with np.load(os.path.join(GOLDEN, "ablation.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def test_both_branches_three_word_rows_and_the_recorded_gaps():
    g = _golden()
    cases = [str(c) for c in g["cases"]]
    found = np.concatenate([g[c + "_img_found"] for c in cases])
    assert found.any() and (~found).any()
    assert sum(len(g[c + "_word_t"]) for c in cases) >= 3
    assert os.path.getsize(os.path.join(GOLDEN, "ablation.npz")) < 2**20
    for c in cases:
        cap = g[c + "_caption"].tolist()
        for i, t in enumerate(g[c + "_img_t"].tolist()):
            sums = np.sort(g[c + "_img_patch_sums"][i].ravel())[::-1]
            gap = (sums[19] - sums[20]) / np.abs(sums).max()
            assert abs(gap - g[c + "_img_gap"][i]) < 1e-12 and gap >= 1e-3, (c, i)
            new, w = g["%s_img_cap_%d" % (c, i)].tolist(), cap[t + 1]
            assert bool(g[c + "_img_found"][i]) == (w in new)
            assert g[c + "_img_new_idx"][i] == (new.index(w) if w in new else -1)
            assert np.isnan(g[c + "_img_diff"][i]) == (w not in new)
        for i, t in enumerate(g[c + "_word_t"].tolist()):
            v = np.sort(g["%s_word_rw_%d" % (c, i)][1:].astype(np.float64))[::-1]
            gap = (v[2] - v[3]) / np.abs(v).max() if len(v) > 3 else 1.0
            assert abs(gap - g[c + "_word_gap"][i]) < 1e-12 and gap >= 1e-3, (c, i)


def test_numpy_restatement_of_the_two_selection_rules():
    """evaluation.py:70-76: zero the 20 patches of the largest sums; :242-247: drop 1 + topk(r_words[1:t + 1], 3)"""
    g = _golden()
    for c in [str(c) for c in g["cases"]]:
        cap = g[c + "_caption"]
        for i in range(len(g[c + "_img_t"])):
            sums = g[c + "_img_patch_sums"][i].ravel()
            mask = np.ones(sums.size, np.uint8)
            mask[np.argsort(-sums, kind="stable")[:20]] = 0
            assert np.array_equal(mask.reshape(28, 28), g[c + "_img_mask"][i]), (c, i)
        for i, t in enumerate(g[c + "_word_t"].tolist()):
            rw = g["%s_word_rw_%d" % (c, i)].astype(np.float64)
            assert rw.shape == (t + 1,)
            top = np.argsort(-rw[1:], kind="stable")[:3] + 1
            assert top.tolist() == g[c + "_word_deleted"][i].tolist(), (c, i)
            assert np.delete(cap[:t + 1], top).tolist() == g["%s_word_short_%d" % (c, i)].tolist(), (c, i)
