"""The bottom-up gridTD model explained (`GridTDBUEngine`, explainers/gridtd.py) against tests/golden/gridtd_bu.npz: the
reference's `GridTDModelBU` trace, its `ExplainGridTDAttention` decoder relevance on a stub that shares the model's decoder, and the
tail - the mean of the PROJECTED regions under the projector rule - from three uses of the reference's own `lrp_linear_eps`
(tests/golden/make_golden_gridtd_bu.py).  P = 36, C = 2048, V = 9586.  The new kernel entry `lrpx_gridtd_rel_pix_rows_avg` is also held
alone: byte for byte against `lrpx_gridtd_rel_pix_rows` where its added term vanishes, and against fp64 where only that term is left.
Every deviation is printed before it is asserted."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

PAIRS = dict(h1t="h1", c1t="c1", h2t="h2", c2t="c2", g1t="g1", g2t="g2", i1t_act="i1", f1t_act="f1", i2t_act="i2", f2t_act="f2", st="s",
             context="ctx", context_hat="ctx_hat", alphas="alpha", betas="beta")
P, CH, H = 36, 2048, 512


def _features(g, which):
    from lrp_amd import weights
    nonzero = g[which + "_nonzero"].tolist()
    f = weights.make_bu_features(int(g["feat_seed"]) + (which == "long"), len(nonzero), P, CH)
    for b, n in enumerate(nonzero):
        f[b, n:] = 0
    return torch.from_numpy(f)


@pytest.fixture(scope="module")
def fx():
    """the fixture, the engine on its state, and ONE explained `pair` batch shared by the tests (clones: never overwritten)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import weights
    from lrp_amd.explainers.gridtd import GridTDBUEngine
    with np.load(os.path.join(GOLDEN, "gridtd_bu.npz"), allow_pickle=False) as f:
        g = {k: f[k] for k in f.files}
    V = int(g["V"])
    eng = GridTDBUEngine(weights.make_gridtd_bu_state(seed=int(g["seed"]), vocab_size=V))
    feats, caps = _features(g, "pair"), torch.from_numpy(g["pair_caption"])
    r_feat, r_words, pred, tr, enc = eng.explain_batch(feats, caps, return_features=True, predictions=True)
    torch.cuda.synchronize()
    return types.SimpleNamespace(g=g, V=V, eng=eng, feats=feats, caps=caps, wm=weights.make_word_map(V), r_feat=r_feat.clone(),
                                 r_words=r_words.clone(), pred=pred.clone(), tr={k: v.clone() for k, v in tr.items() if torch.is_tensor(v)},
                                 want_feat=g["pair_r_feat"].transpose(0, 3, 1, 2))          # (B, T, P, C): the fixture stores the word last


@pytest.fixture(scope="module")
def small():
    """a V = 503 engine for the tests that compare the engine with itself"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd import weights
    from lrp_amd.explainers.gridtd import GridTDBUEngine
    return GridTDBUEngine(weights.make_gridtd_bu_state(seed=5, vocab_size=503))


def _small_inputs(k, B=2, T=3):
    from lrp_amd import weights
    return (torch.from_numpy(weights.make_bu_features(10 + k, B)).cuda(), torch.from_numpy(weights.make_captions(20 + k, B, T, 503)).cuda())


def _check_rows(what, r_feat, r_words, want_feat, want_words, rows):
    """SURVEY §8(d)'s bounds (tests/test_gpu_gridtd.py): r_feat within 1e-4 of each map's maximum, r_words within 1e-5 of the fp32
    reference, zero behind word t"""
    for (b, t, w) in rows:
        e = rel_err(r_feat[b, t].cpu(), want_feat[w])
        d = np.abs(r_words[b, t, :t + 1].cpu().numpy() - want_words[w][:t + 1]).max()
        print("%s image %d word %d: r_feat %.2e of the map's maximum, r_words %.2e" % (what, b, t, e, d))
        assert e < 1e-4, (what, b, t, e)
        assert d < 1e-5, (what, b, t, d)
        assert torch.count_nonzero(r_words[b, t, t + 1:]) == 0


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------
def _stab(z):
    zt = z + 0.01 * torch.sign(z)
    return torch.where(zt == 0, torch.full_like(zt, 0.01), zt)


@pytest.mark.parametrize("T, lens, rowlist", [(3, None, False), (3, [2, 0], True), (3, [2, 0], False), (26, None, False), (26, [26, 5], True)],
                         ids=["T3", "T3_lens_rows", "T3_lens", "T26", "T26_lens_rows"])
def test_pixel_rule_with_the_mean_term_alone(small, T, lens, rowlist):
    """P = 36, H = 512, B = 2: rows of at most 24 words take the register branch, words 24 and 25 of T = 26 the loop branch; the grid
    has two pixel chunks (28 + 8).  Outputs pre-filled with NaN."""
    from lrp_amd import _lib
    from lrp_amd._lib import GridRelState, check, ptr, stream_ptr
    lib, eng, B, dev = _lib.load(), small, 2, "cuda"
    gen = torch.Generator(device="cpu").manual_seed(100 + T)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    rows = B * T
    tr = eng._alloc_trace(B, T)
    tr["alpha"].copy_(torch.softmax(rnd(B, T, P), -1))
    proj_pre = rnd(B, P, H)
    Vp = torch.relu(proj_pre)
    avg = Vp.mean(1).contiguous()
    avg[:, 5] = 0                                        # z~(0) = eps
    r_avg, wacc = rnd(rows, H), rnd(rows, T, H)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
    active = [(b * T + t) for b in range(B) for t in range(T) if lens is None or t < lens[b]]
    rl = torch.tensor(active, dtype=torch.int32, device=dev) if rowlist else None
    n = len(active) if rowlist else rows
    keep = {k: torch.zeros(rows, w, device=dev) for k, w in (("r_h2n", H), ("r_c2", H), ("r_c1", H), ("r_ch0", H), ("r_h2p", H), ("r_glob", H),
                                                              ("A", H), ("rx", 4 * H), ("r_words", T))}

    def run(entry, wacc_, r_avg_):
        rs = GridRelState()
        rs.lens = ptr(lens_t)
        for k, v in keep.items():
            setattr(rs, k, ptr(v))
        rs.wacc = ptr(wacc_)
        out = torch.full((n, P, H), float("nan"), device=dev)
        args = (C.byref(tr["_c"]), C.byref(rs), ptr(Vp), ptr(proj_pre))
        if entry == "avg":
            check(lib.lrpx_gridtd_rel_pix_rows_avg(*args, ptr(r_avg_), ptr(avg), ptr(out), ptr(rl), n, stream_ptr()))
        else:
            check(lib.lrpx_gridtd_rel_pix_rows(*args, ptr(out), ptr(rl), n, stream_ptr()))
        torch.cuda.synchronize()
        return out

    # r_avg = 0: the entry without the term, byte for byte
    assert torch.equal(run("avg", wacc, torch.zeros_like(r_avg)), run("plain", wacc, None))
    # wacc = 0: the term alone, against fp64
    got = run("avg", torch.zeros_like(wacc), r_avg).double()
    row_of = active if rowlist else list(range(rows))
    img = torch.tensor([r // T for r in row_of], device=dev)
    ra = r_avg.double()[torch.tensor(row_of, device=dev)]                                    # (n, H)
    want = Vp.double()[img] * (ra / (P * _stab(avg.double())[img]))[:, None, :] / _stab(proj_pre.double())[img]
    live = torch.tensor([r in active for r in row_of], device=dev)
    want[~live] = 0                                                                              # inactive rows are zeros
    err = ((got - want).abs() / want.abs().clamp_min(1e-300))[want != 0].max().item()
    print("T %d lens %s rows %s: the mean term alone, largest element-wise deviation from fp64 %.2e" % (T, lens, rowlist, err))
    assert not torch.isnan(got).any() and torch.equal(got == 0, want == 0)
    assert err < 2e-6
    assert torch.count_nonzero(got[~live]) == 0
    # both terms: the sum of the two runs' brackets (a property of the formula, to fp32 rounding of a map's maximum)
    both, plain = run("avg", wacc, r_avg).double(), run("plain", wacc, None).double()
    assert rel_err(both, plain + got) < 1e-6


# ---- 2. - 4. against the reference -------------------------------------------------------------------------------------------------
def test_trace_vs_reference(fx):
    g = fx.g
    assert fx.eng.cnn is None and fx.eng.vgg is None and fx.eng.resnet is False and (fx.eng.P, fx.eng.C, fx.eng.H) == (P, CH, H)
    errs = {ref: rel_err(fx.tr[mine].cpu(), g["pair_tr_" + ref]) for ref, mine in PAIRS.items()}
    errs["predictions"] = rel_err(fx.pred.cpu()[:, :, ::97], g["pair_tr_predictions"])
    print("trace deviations (of the maximum): %s" % ", ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < 1e-4, (k, e)


def test_relevance_pair_vs_reference(fx):
    g = fx.g
    assert fx.r_feat.shape == (2, 3, P, CH) and fx.r_words.shape == (2, 3, 3)
    rows = [(b, t, (b, t)) for b in range(2) for t in range(3)]
    _check_rows("pair", fx.r_feat, fx.r_words, fx.want_feat, g["pair_r_words"], rows)
    assert torch.count_nonzero(fx.r_feat[1, :, int(g["pair_nonzero"][1]):]) == 0          # padded regions: exact zeros
    assert torch.count_nonzero(fx.r_feat[1, :, :int(g["pair_nonzero"][1])].abs().sum(-1) == 0) == 0


def test_relevance_long_caption_vs_reference(fx):
    """T = 26: word 23 is a row of the register branch of the pixel kernel, words 24 and 25 of its loop branch"""
    g = fx.g
    r_feat, r_words = fx.eng.explain_batch(_features(g, "long"), torch.from_numpy(g["long_caption"]))
    torch.cuda.synchronize()
    assert r_feat.shape == (1, 26, P, CH)
    want = g["long_r_feat"].transpose(2, 0, 1)
    _check_rows("long", r_feat, r_words, want, g["long_r_words"], [(0, int(t), i) for i, t in enumerate(g["long_words"])])
    assert torch.count_nonzero(r_feat[0, :, int(g["long_nonzero"][0]):]) == 0


# ---- 5. - 7. the engine against itself -----------------------------------------------------------------------------------------------
def test_unequal_caption_lengths(fx):
    g = fx.g
    r_feat, r_words, pred = fx.eng.explain_batch(fx.feats, fx.caps, lens=[3, 2], predictions=True)
    torch.cuda.synchronize()
    _check_rows("lens [3, 2]", r_feat, r_words, fx.want_feat, g["pair_r_words"], [(0, 0, (0, 0)), (0, 1, (0, 1)), (0, 2, (0, 2)), (1, 0, (1, 0)), (1, 1, (1, 1))])
    assert torch.count_nonzero(r_feat[1, 2]) == 0 and torch.count_nonzero(r_words[1, 2]) == 0
    assert pred.shape == (2, 3, fx.V)
    r_feat, r_words = fx.eng.explain_batch(fx.feats, fx.caps, lens=[0, 0])
    torch.cuda.synchronize()
    assert r_feat.shape == (2, 3, P, CH) and torch.count_nonzero(r_feat) == 0 and torch.count_nonzero(r_words) == 0


def test_batch_independence(fx):
    from lrp_amd import weights
    feats = torch.cat([fx.feats, torch.from_numpy(weights.make_bu_features(77, 1))])
    caps = torch.cat([fx.caps, torch.from_numpy(weights.make_captions(78, 1, 3, fx.V))])
    three = [t.clone() for t in fx.eng.explain_batch(feats, caps)]
    one = fx.eng.explain_batch(feats[:1], caps[:1])
    torch.cuda.synchronize()
    assert torch.equal(one[0][0], three[0][0]) and torch.equal(one[1][0], three[1][0])
    assert torch.equal(three[0][:2], fx.r_feat) and torch.equal(three[1][:2], fx.r_words)


def _same(got, want, what):
    torch.cuda.synchronize()
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert not torch.isnan(a).any(), (what, i)
        assert torch.equal(a, b), "%s, output %d: %d of %d elements differ, largest difference %.3g" % (
            what, i, int((a != b).sum()), a.numel(), float((a.double() - b.double()).abs().max()))


def _clones(out):
    return tuple(t.clone() for t in out)


def test_stream_and_replica_match_serial(small):
    batches = [_small_inputs(k) + (([3, 2],) if k == 1 else ()) for k in range(3)]
    rep = small.replica()
    assert rep.cnn is None and rep.sd is small.sd and rep._idx_cache is not small._idx_cache
    serial = [_clones((rep if i % 2 else small).explain_batch(b[0], b[1], lens=b[2] if len(b) > 2 else None)) for i, b in enumerate(batches)]
    got = [_clones(o) for o in small.explain_stream(batches, depth=2)]
    assert len(got) == 3 and len(small._replicas) == 2
    for k in range(3):
        _same(got[k], serial[k], "batch %d" % k)


@pytest.mark.parametrize("entry", ["explain_batch_graph", "explain_batch_replay"])
def test_static_steps_are_bit_identical_to_the_eager_step(small, entry):
    """call 0 captures / records, calls 1 and 2 replay on new features and captions (tests/test_gpu_graph_replay.py's pattern)"""
    outs = []
    for k in range(3):
        feats, caps = _small_inputs(5 + k)
        got = _clones(getattr(small, entry)(feats, caps, predictions=True))
        assert len(got) == 3          # r_feat, r_words, predictions
        _same(got, small.explain_batch(feats, caps, predictions=True), "%s, call %d" % (entry, k))
        outs.append(got)
    assert not torch.equal(outs[0][0], outs[1][0])          # (the inputs really differed)
    assert len(small._graphs if entry.endswith("graph") else small._recordings) == 1


# ---- 8. the model's own decoding loops ---------------------------------------------------------------------------------------------------
def test_decode_loops_vs_reference(fx):
    from lrp_amd.explainers.beam import caption_from_sequence
    g, eng, wm = fx.g, fx.eng, fx.wm
    start, end, skip = wm['<start>'], wm['<end>'], g["decode_skip"].tolist()
    enc = eng.encode(fx.feats)
    toks = eng.greedy(enc, g["decode_greedy"].shape[1], start, end)
    assert toks.cpu().tolist() == g["decode_greedy"].tolist()
    seq = eng.beam_search(eng.encode(fx.feats[:1]), int(g["decode_beam_size"]), int(g["decode_beam_steps"]), start, end)
    assert caption_from_sequence(seq, wm)[1:] == g["decode_beam"].tolist()
    seq, lps = eng.sample_lrp(enc, int(g["decode_sample_len"]), start, end, skip)
    d = np.abs(lps.cpu().numpy() - g["decode_sample_logprobs"]).max()
    print("sample_lrp log-probabilities: largest deviation %.2e" % d)
    assert seq.cpu().tolist() == g["decode_sample_seq"].tolist()
    assert d < 1e-5
    preds, wpreds, L = eng.forwardlrp_context(enc, torch.from_numpy(g["decode_fl_caption"]), g["decode_fl_lengths"].tolist(), skip)
    preds, wpreds = preds.cpu(), wpreds.cpu()
    e, ew = rel_err(preds[:, :, ::97], g["decode_fl_pred_sub"]), rel_err(wpreds[:, :, ::97], g["decode_fl_wpred_sub"])
    print("forwardlrp_context: predictions %.2e, re-weighted %.2e of the maximum" % (e, ew))
    assert L == int(g["decode_fl_L"]) and tuple(preds.shape) == (2, L, fx.V)
    assert preds.argmax(-1).tolist() == g["decode_fl_pred_argmax"].tolist() and wpreds.argmax(-1).tolist() == g["decode_fl_wpred_argmax"].tolist()
    assert e < 1e-4 and ew < 1e-4


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_fire_before_any_launch(small, monkeypatch):
    from lrp_amd import _lib
    feats, caps = _small_inputs(0)
    enc, tr = small.encode(feats), None

    def boom(*a, **k):
        raise AssertionError("a library call before the refusal")
    monkeypatch.setattr(_lib, "load", boom)
    for call in (lambda: small.guided_gradient(enc, tr), lambda: small.explain_batch_guided(feats, caps),
                 lambda: small.explain_batch_gradient(feats, caps)):
        with pytest.raises(NotImplementedError, match="no gradient explainer is defined for the bottom-up model"):
            call()
    images = torch.zeros(2, 3, 224, 224)
    for bad in (images, feats[:, :35], feats[:, :, :2047], torch.zeros(2, 196, 512)):
        for entry in (small.encode, lambda f: small.explain_batch(f, caps), lambda f: small.explain_batch_graph(f, caps),
                      lambda f: small.explain_batch_replay(f, caps)):
            with pytest.raises(ValueError, match="GridTDBUEngine"):
                entry(bad)
