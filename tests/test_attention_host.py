"""Host logic of the attention / Grad-CAM / chance arms (no GPU): the reference's box loop restated in numpy, with and without the in-place
cut carrying over to a word's later boxes, against the tables the reference itself produced (tests/golden/attention_arms.npz, written
by tests/golden/make_golden_attention.py); the `np.delete` rule of the random word arm; `weights.sharpen_attention`; the argument checks
of `ops.expand_maps` and of the functions of explainers/attention.py."""
import os
import types

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN

THR = [0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "attention_arms.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _overlap(box, relevance, threshold):
    """`_calculate_overlaped_pixels` (evaluation.py:313-336), cutting `relevance` in place as the reference does"""
    inside = np.zeros(relevance.shape)
    inside[box[1]:box[3], box[0]:box[2]] = 1
    cut = relevance <= threshold
    if np.sum(cut > 0):
        relevance[cut] = 0
    total = np.sum(relevance)
    if total == 0:
        return 0
    ratio = 1.0 * np.sum(np.multiply(inside, relevance)) / total
    return 1. if ratio > 1 else ratio


def _box_loop(rel, boxes, carry):
    """evaluation.py:419-430 for one word: every (box, threshold) score; carry=False hands every box a map of its own"""
    work = rel.copy()
    table = np.zeros((len(boxes), len(THR)))
    for k, box in enumerate(boxes):
        if not carry:
            work = rel.copy()
        for j, thr in enumerate(THR):
            table[k, j] = _overlap(box, work, thr)
    return table


def _ref_map(a, p=14, upscale=16):
    from oracle import lrp_oracle as O
    e = O.pyramid_expand(torch.from_numpy(np.asarray(a, np.float32).reshape(p, p)), upscale).double().numpy()
    m = np.abs(e).max()
    return np.zeros(e.shape) if m == 0 else 1.0 * e / m


def _arm_maps(g, model, arm):
    """the (P,) array behind every row of an arm, from the stored alphas / cams"""
    t = g["%s_box_%s_t" % (model, arm)]
    if arm == "cam":
        return list(g["grid_box_cam_cams"])
    if model == "grid":
        return [g["grid_alphas"][i] for i in t]
    out = []
    for i, h in zip(t, g["aoa_box_att_head"]):
        a = g["aoa_alphas"][i]
        out.append(a[h] if h >= 0 else np.mean(a, axis=0))
    return out


@pytest.mark.parametrize("model,arm", [("grid", "att"), ("grid", "cam"), ("aoa", "att")])
def test_box_loop_restated_with_and_without_the_carry(golden, model, arm):
    """With the carry the restatement gives the reference's own (box, threshold) scores; without it a word's first box is unchanged and
    every later box differs exactly as `bbox_correctness` says: under the carry its score at every threshold is the clean score at the
    last one (the map was already cut there).  1e-9: the maps are rebuilt here from the stored alphas by the oracle's restatement of
    pyramid_expand (float64; the generator asserts them equal, bit for bit, to the arrays the reference used)."""
    g = golden
    pre = "%s_box_%s_" % (model, arm)
    nbox, table, best = g[pre + "nbox"], g[pre + "table"], g[pre + "best"]
    maps = _arm_maps(g, model, arm)
    assert len(maps) == len(nbox) and nbox.sum() == len(table) and (nbox >= 2).any()
    off = 0
    later = 0
    for r, a in enumerate(maps):
        rel = _ref_map(a)
        boxes = g[pre + "boxes"][off:off + nbox[r]].tolist()
        want = table[off:off + nbox[r]]
        with_carry, clean = _box_loop(rel, boxes, True), _box_loop(rel, boxes, False)
        assert np.abs(with_carry - want).max() < 1e-9, (model, arm, r)
        assert np.abs(np.maximum(want.max(axis=0), 0) - best[r]).max() == 0
        assert np.abs(clean[0] - want[0]).max() < 1e-9
        for k in range(1, nbox[r]):
            assert np.abs(want[k] - clean[k, -1]).max() < 1e-9, (model, arm, r, k)
            later += int(np.abs(clean[k] - want[k]).max() > 1e-6)
        off += nbox[r]
    if arm == "att":
        assert later >= 1, "no later box whose clean scores differ from the carried ones: the quirk is not exercised"
    if (model, arm) != ("grid", "cam"):
        full = _ref_map(maps[int(g[model + "_map_row"])])
        assert np.abs(full - g[model + "_map_full"]).max() <= 2.0 ** -24          # stored as fp32


def test_golden_meets_its_conditions(golden):
    g = golden
    assert len(g["grid_abl_att_t"]) >= 4 and (g["grid_abl_att_gap"] >= 1e-3).all() and (g["aoa_mask_gap"] >= 1e-3).all()
    assert set(g["grid_abl_att_found"].tolist()) | set(g["grid_abl_rnd_found"].tolist()) == {True, False}
    assert len(g["aoa_mask_t"]) >= 4 and set(g["aoa_box_att_head"].tolist()) == {-1, int(g["aoa_head"])}
    assert g["grid_abl_rnd_perm"].shape[1] == 224 * 224 and len(g["grid_abl_rnd_perm"]) <= 2
    for row in g["grid_abl_rnd_perm"]:
        assert sorted(row.tolist()) == list(range(224 * 224))
    assert all(v.dtype.kind in "biuf" or v.dtype.kind == "U" for v in g.values())
    # the masks are the 20 largest patch sums of the reference's own maps
    for pre in ("grid_abl_att_", "grid_abl_rnd_", "aoa_mask_"):
        for mask, sums in zip(g[pre + "mask"], g[pre + "sums"]):
            top = np.argsort(-sums.ravel(), kind="stable")[:20]
            assert sorted(np.flatnonzero(mask.ravel() == 0).tolist()) == sorted(top.tolist())


def test_random_word_arm_is_np_delete(golden):
    """`word_ablation(delete_ids=)` deletes as `np.delete(sub_caption, delete_id)` (evaluation.py:269): the golden's drawn positions give
    the shortened captions the reference teacher-forced; a position named twice counts once, negative positions count from the end, a
    position outside the prefix is numpy's IndexError"""
    from lrp_amd.explainers import ablation
    g = golden
    eng = types.SimpleNamespace(device=torch.device("cpu"))
    cap, ts, ids = g["grid_caption"], g["grid_abl_wrd_t"].tolist(), g["grid_abl_wrd_ids"]
    assert len(ts) >= 1
    short, lens = ablation.delete_tokens(eng, torch.tensor(np.stack([cap] * len(ts))), ts, ids)
    for i, t in enumerate(ts):
        want = np.delete(cap[:t + 1], ids[i]).tolist()
        assert want == g["grid_abl_wrd_short_%d" % i].tolist()
        assert short[i, :lens[i]].tolist() == want and not short[i, lens[i]:].any() and lens[i] == t + 1 - 3
    caps = torch.arange(10, 20)[None].repeat(4, 1)
    short, lens = ablation.delete_tokens(eng, caps, [5, 5, 7, 3], [[1, 1, 2], [-1, 0, 3], [7, 6, 5], [1, 2, 3]])
    for r, (t, d) in enumerate(((5, [1, 1, 2]), (5, [-1, 0, 3]), (7, [7, 6, 5]), (3, [1, 2, 3]))):
        assert short[r, :lens[r]].tolist() == np.delete(np.arange(10, 11 + t), d).tolist(), r
    with pytest.raises(IndexError):
        ablation.delete_tokens(eng, caps, [5, 5, 7, 3], [[1, 2, 6], [1, 2, 3], [1, 2, 3], [1, 2, 3]])
    with pytest.raises(IndexError):
        np.delete(np.arange(6), [1, 2, 6])
    with pytest.raises(ValueError):
        ablation.delete_tokens(eng, caps, [5, 5, 7, 3], [[1, 2, 3]])
    with pytest.raises(ValueError):
        ablation.delete_tokens(eng, caps, [5, 5, 10, 3], [[1, 2, 3]] * 4)


def test_sharpen_attention_keys_per_model():
    from lrp_amd import weights
    small = dict(vocab_size=50, embed_dim=8, hidden_dim=8)
    for make, keys in ((lambda: weights.make_gridtd_resnet_state(seed=1, feat_dim=16, num_pixels=9, **small), ["AdaAttention.w_h.weight"]),
                       (lambda: weights.make_adaatt_state(seed=1, feat_dim=16, num_pixels=9, encoder=None, **small), ["AdaAttention.w_h.weight"]),
                       (lambda: weights.make_aoa_state(seed=1, feat_dim=16, with_encoder=False, **small),
                        ["decoder_multihead_attention.q_proj.weight", "decoder_multihead_attention.q_proj.bias"])):
        sd = make()
        sharp = weights.sharpen_attention(sd, 64)
        assert list(sharp) == list(sd)
        for k in sd:
            if k in keys:
                assert sharp[k].dtype == np.float32 and np.array_equal(sharp[k], sd[k] * np.float32(64)) and sharp[k] is not sd[k]
            else:
                assert sharp[k] is sd[k]
        assert np.array_equal(weights.sharpen_attention(sd, 1)[keys[0]], sd[keys[0]])
    with pytest.raises(ValueError):
        weights.sharpen_attention({"fc.weight": np.zeros((2, 2), np.float32)}, 2)


def test_expand_maps_argument_checks():
    """refused by host logic, before the library is asked for anything: the reference would fail at `reshape` / `mask * image`"""
    from lrp_amd import ops
    for maps, hw, kw in ((torch.zeros(2, 195), 224, {}),                  # not a square grid
                         (torch.zeros(2, 8, 195), 224, {}),
                         (torch.zeros(2, 196), 225, {}),                  # not a multiple of the grid
                         (torch.zeros(2, 196), 0, {}),
                         (torch.zeros(196), 224, {}),                     # no rows
                         (torch.zeros(1, 2, 8, 196), 224, {}),
                         (torch.zeros(2, 196), 224, dict(head=0)),        # a head of single-head maps
                         (torch.zeros(2, 8, 196), 224, dict(head=8)),
                         (torch.zeros(2, 8, 196), 224, dict(head=-1))):
        with pytest.raises(ValueError, match="expand_maps"):
            ops.expand_maps(maps, hw, **kw)
    with pytest.raises(ValueError, match="device tensors"):               # there is no CPU path
        ops.expand_maps(torch.zeros(2, 196), 224)


def test_attention_functions_refuse_what_has_no_image_grid():
    from lrp_amd import explainers
    from lrp_amd.explainers import attention
    assert explainers.attention_maps is attention.attention_maps and explainers.gradcam_maps is attention.gradcam_maps
    assert explainers.one_minus_beta is attention.one_minus_beta
    regions = types.SimpleNamespace(cnn=None, resnet=False, device=torch.device("cpu"))
    tr = dict(alpha=torch.zeros(1, 2, 36), beta=torch.tensor([[0.25, 0.5]]))
    with pytest.raises(ValueError, match="no encoder"):
        attention.attention_maps(regions, tr)
    with pytest.raises(ValueError, match="no encoder"):
        attention.gradcam_maps(regions, torch.zeros(1, 2, 36))
    vgg = types.SimpleNamespace(cnn=object(), resnet=False, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="single-head"):
        attention.attention_maps(vgg, dict(alpha=torch.zeros(1, 2, 196)), head=0)
    with pytest.raises(ValueError, match="square"):
        attention.attention_maps(vgg, dict(alpha=torch.zeros(1, 2, 195)))
    with pytest.raises(ValueError, match="sentinel"):
        attention.one_minus_beta(dict(alpha=torch.zeros(1, 2, 8, 196)))
    assert attention.one_minus_beta(tr).tolist() == [0.75, 0.5]
    assert attention.one_minus_beta(dict(beta=torch.tensor([[0.25, 0.5], [0.125, 0.0]])), lens=[2, 1]).tolist() == [0.75, 0.5, 0.875]
    assert attention._image_grid(vgg, 196, "x") == (14, 224)
    assert attention._image_grid(types.SimpleNamespace(cnn=object(), resnet=True), 196, "x") == (14, 448)
