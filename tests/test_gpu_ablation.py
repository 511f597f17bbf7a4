"""The device work of the ablation experiment (lrp_amd/explainers/ablation.py): the two small kernels against numpy in float64, and
`image_ablation`'s chunking against itself."""
import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.parametrize("V", [37, 9586])
def test_softmax_pick_rows_vs_float64(V):
    """softmax(x[r])[ids[r]] for 5 rows (a padded row stride, the first and the last id, a row with one dominant score).  Bound: the
    exponent's argument x - max (|.| <= 40 here) carries half an ulp of 40, 2.4e-6, into exp's relative error, expf itself 2 ulp, the
    sum of V such terms no more than its terms: 1e-5 of the value."""
    _need_gpu()
    from lrp_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(V)
    rows, ld = 5, V + 3
    x = (rs.standard_normal((rows, ld)) * 4).astype(np.float32)
    x[3, V // 2] = 30.0
    ids = np.array([0, V - 1, V // 3, V // 2, 5], np.int64)
    xd, idd = torch.from_numpy(x).cuda(), torch.from_numpy(ids).cuda()
    out = torch.empty(rows, device="cuda")
    _lib.check(lib.lrpx_softmax_pick_rows(_lib.ptr(xd), ld, rows, V, _lib.ptr(idd), _lib.ptr(out), _lib.stream_ptr()))
    x64 = x[:, :V].astype(np.float64)
    e = np.exp(x64 - x64.max(1, keepdims=True))
    want = (e / e.sum(1, keepdims=True))[np.arange(rows), ids]
    rel = np.abs(out.cpu().numpy() - want) / want
    print("softmax_pick_rows V = %d: largest deviation %.2e of the value" % (V, rel.max()))
    assert rel.max() < 1e-5
    # an id outside the row is NaN, never a read outside it
    idd[2] = V
    _lib.check(lib.lrpx_softmax_pick_rows(_lib.ptr(xd), ld, rows, V, _lib.ptr(idd), _lib.ptr(out), _lib.stream_ptr()))
    assert torch.isnan(out[2]).item() and not torch.isnan(out[[0, 1, 3, 4]]).any().item()


def _delete_host(cap, rw, t, kdel):
    order = np.argsort(-rw[1:t + 1].astype(np.float64), kind="stable")[:kdel] + 1          # ties: the earlier word
    return np.delete(cap[:t + 1], order), order


def test_delete_topk_tokens_vs_numpy():
    """evaluation.py:242-247 on rows of different t in one launch: t = 3 (the smallest with three deletable words: <start> alone is
    left), t = 19, t = 70 (more positions than the wave has lanes), a tie at the third place (the earlier word goes), a tie between the
    first two, the largest relevance at <start> (never a candidate), and kdel = 1 .. 4.  Bit-exact: positions, captions, lengths."""
    _need_gpu()
    from lrp_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(3)
    ts = [3, 19, 70, 19, 7, 12, 6]
    R, W = len(ts), 75
    caps = rs.randint(4, 9000, size=(R, W)).astype(np.int64)
    rw = rs.standard_normal((R, W)).astype(np.float32)
    rw[3, [2, 5, 9, 14]] = [9.0, 8.0, 7.0, 7.0]              # third place: positions 9 and 14 tie, 9 goes
    rw[4, [3, 6]] = 5.0                                       # first place: 3 before 6
    rw[5, 0] = 50.0                                           # <start> carries the most: not a candidate
    rw[6, 1:7] = 1.0                                          # all equal: 1, 2, 3
    cd, rd, td = torch.from_numpy(caps).cuda(), torch.from_numpy(rw).cuda(), torch.tensor(ts, dtype=torch.int32, device="cuda")
    for kdel in (3, 1, 2, 4):
        out = torch.full((R, W), -7, dtype=torch.int64, device="cuda")
        lens = torch.zeros(R, dtype=torch.int32, device="cuda")
        gone = torch.zeros(R, kdel, dtype=torch.int32, device="cuda")
        _lib.check(lib.lrpx_delete_topk_tokens(_lib.ptr(cd), W, _lib.ptr(rd), W, _lib.ptr(td), R, kdel, _lib.ptr(out), W, _lib.ptr(lens),
                                               _lib.ptr(gone), _lib.stream_ptr()))
        out, lens, gone = out.cpu().numpy(), lens.cpu().numpy(), gone.cpu().numpy()
        for r, t in enumerate(ts):
            if t < kdel:
                continue
            want, order = _delete_host(caps[r], rw[r], t, kdel)
            assert lens[r] == t + 1 - kdel and gone[r].tolist() == order.tolist(), (kdel, r)
            assert out[r, :lens[r]].tolist() == want.tolist() and (out[r, lens[r]:] == -7).all(), (kdel, r)
        if kdel == 3:
            assert gone[3].tolist() == [2, 5, 9] and gone[4][:2].tolist() == [3, 6] and 0 not in gone[5] and gone[6].tolist() == [1, 2, 3]
            assert lens[0] == 1 and out[0, 0] == caps[0, 0]
    # fewer candidates than kdel: all of them go, the missing places read -1
    out = torch.zeros(R, W, dtype=torch.int64, device="cuda")
    lens = torch.zeros(R, dtype=torch.int32, device="cuda")
    gone = torch.zeros(R, 4, dtype=torch.int32, device="cuda")
    _lib.check(lib.lrpx_delete_topk_tokens(_lib.ptr(cd), W, _lib.ptr(rd), W, _lib.ptr(td), R, 4, _lib.ptr(out), W, _lib.ptr(lens), _lib.ptr(gone),
                                           _lib.stream_ptr()))
    assert lens.cpu()[0].item() == 1 and sorted(gone.cpu()[0].tolist()) == [-1, 1, 2, 3]
    assert lib.lrpx_delete_topk_tokens(_lib.ptr(cd), W, _lib.ptr(rd), W, _lib.ptr(td), R, 5, _lib.ptr(out), W, _lib.ptr(lens), _lib.ptr(gone),
                                       _lib.stream_ptr()) == _lib.EINVAL


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


def test_image_ablation_70_rows_equal_35_plus_35():
    """`image_ablation` works in chunks of 16 rows at beam 3 (48 rows a launch, 16 masked images an `encode`): 70 rows are 4 x 16 + 6, the
    same rows as two calls are 16 + 16 + 3 twice - rows meet other neighbours in chunks of other sizes.  Everything it returns is the same, bit for bit, and both branches
    (word found with a probability, word gone with NaN) are among the rows.  `word_prob` / `word_ablation` on the same engine: a row's
    number does not depend on the rows beside it either."""
    _need_gpu()
    from lrp_amd import weights
    from lrp_amd.explainers import ablation
    from lrp_amd.explainers.gridtd import GridTDEngine
    V, R = 503, 70
    wm = weights.make_word_map(V)
    eng = GridTDEngine(weights.make_gridtd_state(seed=5, vocab_size=V))
    images = torch.from_numpy(weights.make_images(70, 4)).cuda()
    row2img = torch.arange(R) % 4
    g = torch.Generator().manual_seed(9)
    spatial = torch.randn(R, 224, 224, generator=g).cuda()
    special = [wm[k] for k in ('<start>', '<end>', '<unk>', '<pad>')]
    kw = dict(start_id=wm['<start>'], end_id=wm['<end>'], special_ids=special)
    _, _, _, caps = ablation.image_ablation(eng, images, row2img, spatial, [0] * R, **kw)
    # even rows: a word of the row's new caption (found); odd rows: an id no caption holds (gone)
    absent = next(w for w in range(4, V) if all(w not in c for c in caps))
    targets = [caps[r][(r // 2) % len(caps[r])] if r % 2 == 0 else absent for r in range(R)]
    found, idx, prob, caps2 = ablation.image_ablation(eng, images, row2img, spatial, targets, **kw)
    assert caps2 == caps
    assert found.tolist() == [r % 2 == 0 for r in range(R)]
    assert all(caps[r].index(targets[r]) == idx[r].item() for r in range(0, R, 2)) and (idx[1::2] == -1).all()
    assert torch.isnan(prob[1::2]).all() and ((prob[0::2] > 0) & (prob[0::2] <= 1)).all()
    halves = [ablation.image_ablation(eng, images, row2img[a:b], spatial[a:b], targets[a:b], **kw) for a, b in ((0, 35), (35, 70))]
    assert torch.equal(torch.cat([h[0] for h in halves]), found) and torch.equal(torch.cat([h[1] for h in halves]), idx)
    assert _same(torch.cat([h[2] for h in halves]), prob)
    assert halves[0][3] + halves[1][3] == caps
    # the found rows against the drop-in's route, one row at a time: teacher-force the prefix on the masked image alone
    from lrp_amd import evaluation
    for r in (0, 20, 36, 68):
        masked = evaluation.block_image(spatial[r:r + 1])[:, None] * images[row2img[r]][None]
        enc = eng.encode(masked)
        cap = torch.tensor([[wm['<start>']] + caps[r][:idx[r].item()] + [0]], dtype=torch.int64, device="cuda")
        tr = eng.trace(enc, cap, model_bias=False, predictions=False)
        sc = eng.logits(tr["hc"].view(cap.shape[1] - 1, eng.H))[-1:]
        one = ablation.softmax_pick(eng, sc, torch.tensor([targets[r]]))
        assert one.item() == prob[r].item(), r
    # word ablation: 70 rows at once equal 35 + 35
    enc = eng.encode(images)
    T = 9
    captions = torch.from_numpy(weights.make_captions(31, R, T, V))
    t_rows = [6 + r % 3 for r in range(R)]
    r_words = torch.randn(R, T, generator=g)
    tr = eng.trace(enc, captions[:4].cuda(), model_bias=False, predictions=True)
    p0 = ablation.word_prob(eng, tr["pred"], t_rows, captions[torch.arange(R), torch.tensor(t_rows) + 1], row2img=row2img)
    assert ((p0 > 0) & (p0 <= 1)).all()
    full = ablation.word_ablation(eng, enc, row2img, captions, t_rows, r_words)
    parts = [ablation.word_ablation(eng, enc, row2img[a:b], captions[a:b], t_rows[a:b], r_words[a:b]) for a, b in ((0, 35), (35, 70))]
    assert torch.equal(torch.cat(parts), full) and ((full > 0) & (full <= 1)).all()


def _golden():
    import os
    from conftest import GOLDEN
    with np.load(os.path.join(GOLDEN, "ablation.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def test_ablation_vs_the_references_own_experiment():
    """tests/golden/ablation.npz: `EvaluationExperiments.ablation_experiment` run by the reference on the seeded gridTD model
    (tests/golden/make_golden_ablation.py), once per stored word map (case "b": <end> := a word the model produces, so that words
    disappear).  The drop-in explains the image (its own beam search, its own maps and r_words); `image_ablation` / `word_ablation`
    on those must give, bit for bit, the reference's masks, new captions, found / new_idx, deleted positions and shortened captions.
    Probabilities: tests/test_gpu_dropin.py holds `teacherforce_forward` to 1e-4 of the largest score; a softmax probability moves by at
    most twice the largest score error, so 2e-4 of the largest score the reference's teacher-forced calls produced (`absmax`).
    Measured on an MI355X: 2.9e-11 (original scores), 1.5e-11 (new scores of the image rows), 4.4e-11 (word rows) against a bound of
    4.6e-5 - the probabilities of this near-uniform model are ~1e-4, so the id-level comparisons carry the test."""
    _need_gpu()
    import types
    from lrp_amd import evaluation, weights
    from lrp_amd.explainers import ablation
    from lrp_amd.explainers.gridtd import ExplainGridTDAttention
    g = _golden()
    V, seed = int(g["V"]), int(g["seed"])
    sd = weights.make_gridtd_state(seed=seed, vocab_size=V)
    img = torch.from_numpy(weights.make_images(seed + 7, 1)).cuda()
    branches = set()
    for c in [str(c) for c in g["cases"]]:
        wm = weights.make_word_map(V)
        wm['<end>'] = int(g[c + "_end"])
        ex = ExplainGridTDAttention(types.SimpleNamespace(height=224, width=224), wm, model=sd)
        maps, rws = ex.explain_caption(img)
        caption = [int(w) for w in ex.beam_caption_encode]
        assert caption == g[c + "_caption"].tolist(), c
        eng, tol = ex.engine, 2e-4 * float(g[c + "_absmax"])
        special = [wm[k] for k in ('<start>', '<end>', '<unk>', '<pad>')]
        preds = ex.predictions[None]
        # image ablation
        ts = g[c + "_img_t"].tolist()
        if ts:
            targets = [caption[t + 1] for t in ts]
            spatial = evaluation.spatial_relevance(torch.cat([maps[t] for t in ts]))
            mask = evaluation.block_image(spatial)
            assert np.array_equal(mask[:, ::8, ::8].cpu().numpy().astype(np.uint8), g[c + "_img_mask"]), c
            found, idx, prob, caps = ablation.image_ablation(eng, img, [0] * len(ts), spatial, targets, wm['<start>'], wm['<end>'], special,
                                                             model_bias=ex.TF_MODEL_BIAS)
            assert found.cpu().numpy().tolist() == g[c + "_img_found"].tolist() and idx.cpu().tolist() == g[c + "_img_new_idx"].tolist(), c
            for i in range(len(ts)):
                assert caps[i] == g["%s_img_cap_%d" % (c, i)].tolist(), (c, i)
            orig = ablation.word_prob(eng, preds, ts, targets, row2img=[0] * len(ts)).cpu().double().numpy()
            d0 = np.abs(orig - g[c + "_img_orig"]).max()
            f = g[c + "_img_found"]
            assert np.isnan(prob.cpu().numpy()[~f]).all()
            d1 = np.abs(prob.cpu().double().numpy()[f] - (g[c + "_img_orig"] - g[c + "_img_diff"])[f]).max() if f.any() else 0.0
            print("case %s image ablation: %d rows (%d found), original score %.2e, new score %.2e (bound %.2e)" % (c, len(ts), f.sum(), d0, d1, tol))
            assert d0 < tol and d1 < tol, (c, d0, d1, tol)
            branches |= set(f.tolist())
        # word ablation
        ts = g[c + "_word_t"].tolist()
        if ts:
            R, T = len(ts), len(caption) - 1
            r_words = torch.zeros(R, T)
            for i, t in enumerate(ts):
                r_words[i, :t + 1] = rws[t].cpu()
            captions = torch.tensor([caption] * R)
            short, lens, deleted = ablation.delete_topk_tokens(eng, captions, ts, r_words)
            assert deleted.cpu().tolist() == g[c + "_word_deleted"].tolist(), c
            for i in range(R):
                assert short[i, :lens[i]].cpu().tolist() == g["%s_word_short_%d" % (c, i)].tolist(), (c, i)
            new = ablation.word_ablation(eng, eng.encode(img), [0] * R, captions, ts, r_words, model_bias=ex.TF_MODEL_BIAS).cpu().double().numpy()
            d2 = np.abs(new - (g[c + "_word_orig"] - g[c + "_word_diff"])).max()
            print("case %s word ablation: %d rows, new score %.2e (bound %.2e)" % (c, R, d2, tol))
            assert d2 < tol, (c, d2, tol)
    assert branches == {True, False}
