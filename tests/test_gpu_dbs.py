"""The batched on-device diverse beam search: `lrpx_dbs_step_batch` alone against the list-level restatement of the reference's loop
(tests/dbs_restate.py, models/gridTDmodel.py:337-392) on recorded and drawn scores, `explainers.beam.diverse_beam_search_batch` against
the reference's own output (tests/golden/dbs.npz), and what the search promises without a golden: group 0 is the beam search, without a
penalty every group is, and an image's result does not depend on what else is in the batch."""
import ctypes as C
import os
import sys

import pytest
import torch

import lrp_amd  # noqa: F401
from lrp_amd.explainers import diverse_beam_search_batch, diverse_captions_batch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbs_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

START = 1
LIMIT = 1024          # LRPX_BEAM_MAX_STEPS (include/lrpx.h)
M = 8                 # the drawn table has one row of scores per (image, step, previous word % M)
STATE_W = 70          # width of the two stand-in state tensors: no multiple of the wave


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _table(seed, N, T, V):
    """drawn scores; the words below 2 M get a bonus after an input word of their residue class, so that a group tends to choose words
    which are the other groups' inputs one step on - the penalty then decides selections"""
    g = torch.Generator().manual_seed(seed)
    L = torch.randn(N, T, M, V, generator=g) * 2.0
    for m in range(M):
        L[:, :, m, m] += 3.0
        L[:, :, m, m + M] += 3.0
    return L


def _bufs(N, k, V, T, end, diversity, dev="cuda", n_state=2, start=START):
    from lrp_amd import _lib
    G, rows = k, N * k * k
    b = dict(toks=torch.full((rows, T + 1), start, dtype=torch.int64, device=dev),
             seqs=torch.full((rows, T + 1), start, dtype=torch.int64, device=dev),
             best=torch.zeros(N * G, T + 1, dtype=torch.int64, device=dev), cum=torch.zeros(rows, device=dev),
             best_score=torch.zeros(N * G, device=dev), n_live=torch.full((N * G,), k, dtype=torch.int32, device=dev),
             seq_len=torch.ones(N * G, dtype=torch.int32, device=dev), best_len=torch.zeros(N * G, dtype=torch.int32, device=dev),
             live=torch.full((1,), N, dtype=torch.int32, device=dev))
    state = [torch.zeros(rows, T + 1, STATE_W, device=dev) for _ in range(n_state)]
    st = _lib.DbsBatch()
    st.N, st.k, st.G, st.V, st.T, st.start_id, st.diversity = N, k, G, V, T, start, diversity
    if torch.is_tensor(end):
        st.end_id, st.end_ids = -1, _lib.ptr(end)
    else:
        st.end_id, st.end_ids = int(end), None
    st.toks, st.tok_ld, st.seqs, st.seq_ld, st.best, st.best_ld = _lib.ptr(b["toks"]), T + 1, _lib.ptr(b["seqs"]), T + 1, _lib.ptr(b["best"]), T + 1
    st.cum, st.best_score, st.n_live, st.seq_len = _lib.ptr(b["cum"]), _lib.ptr(b["best_score"]), _lib.ptr(b["n_live"]), _lib.ptr(b["seq_len"])
    st.best_len, st.live_images = _lib.ptr(b["best_len"]), _lib.ptr(b["live"])
    st.n_state = len(state)
    for j, s in enumerate(state):
        st.state[j] = _lib.ptr(s)
    st.state_w, st.state_ld = STATE_W, (T + 1) * STATE_W
    return st, b, state


def _device_search(score_rows, N, k, V, T, ends, diversity, start=START, n_state=2):
    """the loop a caller runs, without a model: `score_rows(t, toks)` -> the (rows, V) scores of step t on the device - no host read
    before the end.  Before every launch the `n_state` stand-in state tensors get, at time t + 1, a value that names the row's sequence.
    After it, `ok` collects: [a live row of a group that selected holds its NEW parent's name (the state was gathered like the tokens),
    a live row of a group that was passed over holds what it held at time t and feeds the same word again (the carry), a group without
    live beams is untouched, rows that are not live feed <start>]."""
    from lrp_amd import _lib
    lib, dev = _lib.load(), "cuda"
    rows = N * k * k
    end = ends if isinstance(ends, int) else torch.tensor(ends, dtype=torch.int32, device=dev)
    st, b, state = _bufs(N, k, V, T, end, diversity, start=start, n_state=n_state)
    toks, seqs, n_live, seq_len = b["toks"], b["seqs"], b["n_live"], b["seq_len"]
    grp = torch.arange(rows, device=dev) // k
    slot = (torch.arange(rows, device=dev) % k).to(torch.int32)
    pos = torch.arange(T + 1, device=dev)
    pos_w = (pos % 13 + 1).double()
    col = torch.arange(STATE_W, device=dev).float()
    ok = torch.ones(4, dtype=torch.bool, device=dev)

    def name(length):     # a number < 2^24 (exact in fp32) that differs between a group's sequences of `length` tokens
        return ((seqs.double() * pos_w * (pos[None, :] < length[:, None])).sum(1) % 9973).float()
    for t in range(T):
        x = score_rows(t, toks).contiguous()
        sl0, nl0 = seq_len.clone()[grp].long(), n_live.clone()[grp]
        ident = name(sl0)
        for j, s in enumerate(state):
            s[:, t + 1] = ident[:, None] * (j + 1) + col[None, :]
        before = [v.clone() for v in (toks, seqs, b["cum"])]
        _lib.check(lib.lrpx_dbs_step_batch(C.byref(st), _lib.ptr(x), V, t, _lib.stream_ptr()))
        sl1, nl1 = seq_len[grp].long(), n_live[grp]
        selected, live_row = sl1 > sl0, slot < nl1
        passed = (nl0 > 0) & ~selected
        want = name(sl0)               # the first sl0 tokens of a row are now its parent's: so must its state be
        for j, s in enumerate(state):
            good = (s[:, t + 1] == want[:, None] * (j + 1) + col[None, :]).all(1)
            ok[0] &= (good | ~(selected & live_row)).all()
            ok[1] &= ((s[:, t + 1] == s[:, t]).all(1) | ~passed).all()
        ok[1] &= ((toks[:, t + 1] == toks[:, t]) | ~passed).all()
        for was, now in zip(before, (toks, seqs, b["cum"])):
            same = (was == now).reshape(rows, -1).all(1)
            ok[2] &= (same | (nl0 > 0)).all()
        ok[3] &= ((toks[:, t + 1] == start) | live_row).all()
    out = torch.empty(N * k, T + 2, dtype=torch.int64, device=dev)
    _lib.check(lib.lrpx_dbs_result_batch(C.byref(st), _lib.ptr(out), T + 2, _lib.stream_ptr()))
    host = out.cpu()
    got = [[host[i * k + g, 1:1 + int(host[i * k + g, 0])].tolist() for g in range(k)] for i in range(N)]
    return got, ok.cpu().tolist(), n_live.cpu().view(N, k).tolist(), int(b["live"].item())


def _table_search(L, k, T, ends, diversity, n_state=2):
    N, V = L.shape[0], L.shape[3]
    Ld = L.cuda()
    img = torch.arange(N * k * k, device="cuda") // (k * k)
    return _device_search(lambda t, toks: Ld[img, t, toks[:, t] % M], N, k, V, T, ends, diversity, n_state=n_state)


def _table_restate(L, i, k, T, end, diversity, log=None):
    return R.diverse_beam_search(lambda t, g, seqs: torch.stack([L[i, t, s[-1] % M] for s in seqs]), L.shape[3], k, T, START, end, diversity, log)


ALL_OK = [True, True, True, True]


@pytest.mark.parametrize("V", [37, 9586])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_step_kernel_vs_restatement_on_drawn_tables(V, k):
    """N = 4 images with an <end> id each, 14 steps, diversity 0.5: image 0 with a likely <end> (groups complete some beams, finish and
    pass the later groups over), image 1 with <end> as the best first word, image 2 never completing (every group returns group 0's live
    sequence 0, 15 tokens), image 3 with <end> the best word everywhere from step 3 (every group finishes, one per step)"""
    _need_gpu()
    N, T = 4, 14
    L = _table(200 + k, N, T, V)
    ends = [5, 7, 11, 13]
    L[0, 2:, :, ends[0]] += 4.0
    L[1, 0, START % M, ends[1]] = 40.0
    L[2, :, :, ends[2]] = -60.0
    L[3, :3, :, ends[3]] = -60.0
    L[3, 3:, :, ends[3]] = 60.0
    got, ok, n_live, live = _table_search(L, k, T, ends, 0.5)
    logs = [dict() for _ in range(N)]
    want = [_table_restate(L, i, k, T, ends[i], 0.5, logs[i]) for i in range(N)]
    assert got == want
    assert ok == ALL_OK
    assert got[2] == [got[2][0]] * k and len(got[2][0]) == T + 1 and n_live[2] == [k] * k
    assert n_live[3] == [0] * k and all(s[-1] == ends[3] for s in got[3])
    assert live == sum(1 for n in n_live if any(n))
    if k > 1:
        assert logs[3]["passed_over"]
    if k > 1 and V == 37:       # (among 9586 words no group chooses another's input word)
        assert any(lg["penalised_pick"] for lg in logs)


@pytest.mark.parametrize("n_state", [0, 1, 4])
def test_step_kernel_with_every_count_of_state_tensors(n_state, k=3):
    """no state tensor, one, and the four of gridTD (h1, c1, h2, c2; the cases above run two, as AoA and the adaptive-attention model
    do): two images whose groups are gathered, finish and are passed over - the gather and the carry are checked on every tensor"""
    _need_gpu()
    N, T, V = 2, 10, 37
    L = _table(400, N, T, V)
    ends = [5, 13]
    L[0, 2:, :, ends[0]] += 4.0
    L[1, :3, :, ends[1]] = -60.0
    L[1, 3:, :, ends[1]] = 60.0
    got, ok, n_live, _ = _table_search(L, k, T, ends, 0.5, n_state=n_state)
    logs = [dict(), dict()]
    assert got == [_table_restate(L, i, k, T, ends[i], 0.5, logs[i]) for i in range(N)]
    assert ok == ALL_OK and n_live[1] == [0] * k and logs[1]["passed_over"]


@pytest.mark.parametrize("k", [2, 3, 4])
def test_penalty_decides_selections(k):
    """the same tables with and without the penalty give different results on the device, each equal to its restatement; <end> cannot be
    chosen before step 4 and is likely from there on, so the groups complete sequences of their own (a group that completes nothing
    returns group 0's)"""
    _need_gpu()
    N, T, V, end = 3, 10, 37, 36
    L = _table(300 + k, N, T, V)
    L[:, :4, :, end] = -60.0
    L[:, 4:, :, end] += 3.0
    with_p, ok1, _, _ = _table_search(L, k, T, end, 1.5)
    without, ok0, _, _ = _table_search(L, k, T, end, 0.0)
    assert with_p == [_table_restate(L, i, k, T, end, 1.5) for i in range(N)]
    assert without == [_table_restate(L, i, k, T, end, 0.0) for i in range(N)]
    assert ok1 == ALL_OK and ok0 == ALL_OK
    assert with_p != without


@pytest.mark.parametrize("T", [1, LIMIT])
def test_step_kernel_lengths(T):
    """max_cap_length 1, and the documented limit (include/lrpx.h: LRPX_BEAM_MAX_STEPS) with two images: image 0 never completes, image
    1's group 0 completes at the last step - both ends of the sequence storage are written"""
    _need_gpu()
    N, k, V, end = (2 if T == LIMIT else 1), 2, 37, 9
    L = _table(7 + T, N, T, V)
    L[0, :, :, end] = -60.0
    if T == LIMIT:
        L[1, :T - 1, :, end] = -60.0
        L[1, T - 1, :, end] = 60.0
    got, ok, n_live, _ = _table_search(L, k, T, end, 0.5)
    assert got == [_table_restate(L, i, k, T, end, 0.5) for i in range(N)]
    assert ok == ALL_OK
    assert len(got[0][0]) == min(T + 1, 20)
    if T == LIMIT:
        assert len(got[1][0]) == T + 1 and got[1][0][-1] == end and n_live[1] == [0, k]


def test_every_group_finishes_as_soon_as_it_can():
    """<end> is every row's best word from step 2 on, by far.  Two groups cannot finish in ONE step: the first that does ends the step
    (the `break`).  So group 0 finishes at step 2, group 1 at step 3, group 2 at step 4 - each with the sequence it had when it was
    passed over, so all three return four tokens.  With max_cap_length 4, group 2 never selects again: it falls back to group 0's row 0 -
    candidate 0 of group 0's last step, <end> included, which is also what group 0 returns."""
    _need_gpu()
    k, V, end = 3, 37, 4
    L = _table(11, 1, 8, V)
    L[:, :2, :, end] = -60.0
    L[:, 2:, :, end] = 60.0
    got, ok, n_live, live = _table_search(L, k, 8, end, 0.5)
    assert got == [_table_restate(L, 0, k, 8, end, 0.5)] and ok == ALL_OK
    assert [len(s) for s in got[0]] == [4, 4, 4] and n_live == [[0, 0, 0]] and live == 0
    log = {}
    got4, ok4, n_live4, live4 = _table_search(L[:, :4], k, 4, end, 0.5)
    assert got4 == [_table_restate(L[:, :4], 0, k, 4, end, 0.5, log)] and ok4 == ALL_OK
    assert log["fallback_after_g0_done"] and n_live4 == [[0, 0, k]] and live4 == 1
    assert got4[0][2] == got4[0][0] and got4[0][2][-1] == end and len(got4[0][2]) == 4


def test_exact_ties():
    """Exact ties, decided as the reference's loop decides them.  Step 0: words a < b with the same score - a first.  Their rows of step
    1 are identical and so are their cumulative scores: every candidate of row 0 ties with the same word of row 1, the lower FLAT index
    wins.  Image 0: that best word is <end> - two complete sequences with exactly equal scores in one step, the first is kept, in every
    group (the penalised column is <start>, which no row chooses).  Image 1: it is an ordinary word w."""
    _need_gpu()
    k, T, V, end = 2, 4, 37, 6
    a, b, w = 10, 19, 23                   # a % M = 2, b % M = 3
    L = _table(21, 2, T, V)
    L[:, :, :, end] = -60.0
    for i in range(2):
        L[i, 0, START % M, a] = L[i, 0, START % M, b] = 30.0
        L[i, 1, b % M] = L[i, 1, a % M]
        L[i, 2, b % M] = L[i, 2, a % M]
    L[0, 1:3, a % M, end] = L[0, 1:3, b % M, end] = 50.0
    L[1, 1:3, a % M, w] = L[1, 1:3, b % M, w] = 50.0
    got, ok, _, _ = _table_search(L, k, T, end, 0.5)
    assert got == [_table_restate(L, i, k, T, end, 0.5) for i in range(2)] and ok == ALL_OK
    assert got[0] == [[START, a, end]] * 2
    assert got[1][0][:3] == [START, a, w]


def test_refusals_give_an_error_code_and_launch_nothing():
    """G != k, k = 5, V = 0, N = 0, max_cap_length above the limit, a null pointer, a host pointer: LRPX_EINVAL, and the state on the
    device is as it was; `diverse_beam_search_batch` raises ValueError on a bad beam size or a bad `end_id` before it encodes anything"""
    _need_gpu()
    from lrp_amd import _lib
    lib = _lib.load()
    N, k, V, T = 2, 2, 37, 5
    x = torch.randn(N * 25, V, device="cuda")
    xh = torch.randn(N * 25, V)
    for what in ("G", "k", "V", "N", "T", "null", "host"):
        st, b, state = _bufs(N, 5 if what == "k" else k, V, LIMIT + 1 if what == "T" else T, 3, 0.5)
        keep = {n: v.clone() for n, v in b.items()}
        if what == "G":
            st.G = 3
        elif what == "V":
            st.V = 0
        elif what == "N":
            st.N = 0
        elif what == "null":
            st.seq_len = None
        px = C.c_void_p(xh.data_ptr()) if what == "host" else _lib.ptr(x)
        assert lib.lrpx_dbs_step_batch(C.byref(st), px, V, 0, _lib.stream_ptr()) == _lib.EINVAL, what
        assert "dbs_step_batch" in lib.lrpx_last_error_string().decode()
        if what != "host":
            out = torch.empty(N * 5, LIMIT + 3, dtype=torch.int64, device="cuda")
            assert lib.lrpx_dbs_result_batch(C.byref(st), _lib.ptr(out), LIMIT + 3, _lib.stream_ptr()) == _lib.EINVAL, what
        torch.cuda.synchronize()
        for n, v in b.items():
            assert torch.equal(v, keep[n]), (what, n)
    enc = {"B": 2}
    for bad in (0, 5):
        with pytest.raises(ValueError):
            diverse_beam_search_batch(None, enc, bad, 5, 1, 2)
    eng = type("E", (), {"device": "cuda"})()
    with pytest.raises(ValueError):
        diverse_beam_search_batch(eng, enc, 2, 5, 1, [2, 3, 4])


# ---- the engines ------------------------------------------------------------------------------------------------------------------------
def _engine(kind):
    from lrp_amd import weights
    V = 503
    if kind == "grid":
        from lrp_amd.explainers.gridtd import GridTDEngine
        eng = GridTDEngine(weights.make_gridtd_state(seed=5, vocab_size=V))
        return eng, lambda n: eng.encode(torch.from_numpy(weights.make_images(60, n)).cuda())
    if kind == "aoa":
        from lrp_amd.explainers.aoa import AOAEngine
        eng = AOAEngine(weights.make_aoa_state(seed=5, vocab_size=V))
        return eng, lambda n: eng.encode(images=torch.from_numpy(weights.make_images(61, n)).cuda())
    if kind == "bu":
        from lrp_amd.explainers.gridtd import GridTDBUEngine
        eng = GridTDBUEngine(weights.make_gridtd_bu_state(seed=5, vocab_size=V))
        return eng, lambda n: eng.encode(torch.from_numpy(weights.make_bu_features(62, n)).cuda())
    from lrp_amd.explainers.adaatt import AdaAttEngine
    eng = AdaAttEngine(weights.make_adaatt_state(seed=5, vocab_size=V, feat_dim=192, num_pixels=12, encoder=None))
    return eng, lambda n: eng.encode(features=torch.from_numpy(weights.make_bu_features(63, n, 12, 192)).cuda())


def _pick(enc, idx):
    e = {k: (v[idx].contiguous() if torch.is_tensor(v) else v) for k, v in enc.items()}
    e["B"] = len(idx)
    return e


T_ENG, START_ENG = 16, 1


@pytest.fixture(scope="module", params=["grid", "aoa", "bu", "ada"])
def searched(request):
    """per engine: 17 seeded images encoded ONCE, an <end> id per image, and what every case below compares with, computed once:
    `beam_search_batch` at beam 1, 2 and 3, and the diverse search on each image ALONE at beam 2 (all 17) and beam 3 (the first 8)"""
    _need_gpu()
    from lrp_amd.explainers import beam_search_batch
    eng, encode = _engine(request.param)
    enc = encode(17)
    # an <end> id per image, taken from the words the image's own free run produces (random weights never produce a fixed id): position
    # 2 .. 4 of that run, and every third image keeps an id no word has - the images of one batch finish at different steps
    free = beam_search_batch(eng, enc, 2, T_ENG, START_ENG, -1)
    ends = [-1 if i % 3 == 0 else free[i][2 + i % 3] for i in range(17)]
    plain = {k: beam_search_batch(eng, _pick(enc, range(n)), k, T_ENG, START_ENG, ends[:n]) for k, n in ((1, 17), (2, 17), (3, 8))}
    alone = {k: [diverse_beam_search_batch(eng, _pick(enc, [i]), k, T_ENG, START_ENG, ends[i])[0] for i in range(n)] for k, n in ((2, 17), (3, 8))}
    return eng, enc, ends, plain, alone


@pytest.mark.parametrize("beam,n", [(2, 16), (2, 17), (3, 7), (3, 8)])
def test_a_result_does_not_depend_on_the_batch(searched, beam, n):
    """`diverse_beam_search_batch` on n images equals the same call on each alone, group for group, token for token: 16 / 17 images at
    beam 2 and 7 / 8 at beam 3 (64 and 63 rows in one launch; one image more is a second chunk), and the same with the count of live
    images polled at every step"""
    eng, enc, ends, _, alone = searched
    got = diverse_beam_search_batch(eng, _pick(enc, range(n)), beam, T_ENG, START_ENG, ends[:n])
    assert got == alone[beam][:n]
    assert len({len(g[0]) for g in got}) > 1, "the images of this batch were meant to finish at different steps"
    assert diverse_beam_search_batch(eng, _pick(enc, range(n)), beam, T_ENG, START_ENG, ends[:n], poll=1) == got


@pytest.mark.parametrize("beam", [2, 3])
def test_group_0_is_the_beam_search(searched, beam):
    """group 0 is never penalised and never passed over: it is `beam_search_batch` on that image"""
    _, _, _, plain, alone = searched
    assert [g[0] for g in alone[beam]] == plain[beam][:len(alone[beam])]


def test_without_a_penalty_every_group_is_the_beam_search(searched):
    """diversity_prob = 0: the groups are copies of one beam search, a later one behind by a step for every group that finished before
    it (the `break`).  A copy that is behind returns the same sequence unless max_cap_length cuts it short, i.e. unless group 0's last
    beam completes in the last G - 1 steps; the fixture's <end> words come early in a 16-step run."""
    eng, enc, ends, plain, _ = searched
    got = diverse_beam_search_batch(eng, _pick(enc, range(8)), 3, T_ENG, START_ENG, ends[:8], diversity_prob=0.0)
    assert got == [[s] * 3 for s in plain[3]]


def test_beam_size_1_is_the_greedy_beam(searched):
    eng, enc, ends, plain, _ = searched
    got = diverse_beam_search_batch(eng, enc, 1, T_ENG, START_ENG, ends)
    assert got == [[s] for s in plain[1]]


def test_diverse_captions_drop_the_special_tokens_and_bad_endings(searched):
    """`[<start>] + sen_idx` per group (:391-392), and `remove_bad_endings` (:284-302) at id level: with the last word of the first
    caption declared a bad ending, trailing occurrences go from every caption; one that would be left empty is kept as it was"""
    from lrp_amd.explainers.beam import caption_from_sequence
    eng, enc, _, _, _ = searched
    wm = {'<pad>': 0, '<start>': START_ENG, '<end>': 502, '<unk>': 501}
    one = _pick(enc, [0])
    seqs = diverse_beam_search_batch(eng, one, 2, T_ENG, START_ENG, wm['<end>'])
    caps = diverse_captions_batch(eng, one, wm, 2, T_ENG)
    assert caps == [[caption_from_sequence(s, wm) for s in seqs[0]]]
    assert all(c[0] == START_ENG and not set(c[1:]) & {0, START_ENG, 501, 502} for c in caps[0]) and len(caps[0][0]) > 1
    bad = caps[0][0][-1]

    def trimmed(c):
        words = list(c[1:])
        while words and words[-1] == bad:
            words.pop()
        return c[:1] + words if words else c
    assert diverse_captions_batch(eng, one, wm, 2, T_ENG, bad_ending_ids=[bad]) == [[trimmed(c) for c in caps[0]]]
    assert diverse_captions_batch(eng, one, wm, 2, T_ENG, bad_ending_ids=[]) == caps


# ---- the reference's own runs (tests/golden/dbs.npz) ---------------------------------------------------------------------------------------
def _golden(small=None):
    from test_dbs_host import golden_cases
    return golden_cases(small)


def test_step_kernel_on_the_recorded_scores_of_the_golden_runs():
    """the V = 37 cases carry the scores of every `predict_next_word` call of the reference's run; the restatement's replay tells which
    (step, group) a call belonged to, the kernel gets them as the rows of that group (the rows of a group that did not select hold
    zeros, which it must not read) and has to arrive at the reference's `sen_idx`, group for group"""
    _need_gpu()
    from test_dbs_host import replay, sen_idx
    for c in _golden(small=True):
        k, V, T = c["beam"], c["V"], c["steps"]
        where = []
        orig = R.diverse_beam_search

        def spy(step, *a, **kw):
            return orig(lambda t, g, seqs: (where.append((t, g)), step(t, g, seqs))[1], *a, **kw)
        R.diverse_beam_search = spy
        try:
            _, wm = replay(c)
        finally:
            R.diverse_beam_search = orig
        X = torch.zeros(T, k * k, V)
        for (t, g), lg, n in zip(where, c["logits"], c["rows"]):
            X[t, g * k:g * k + int(n)] = torch.from_numpy(lg[:int(n)].copy())
        Xd = X.cuda()
        got, ok, _, _ = _device_search(lambda t, toks: Xd[t], 1, k, V, T, c["end"], c["div"], start=wm['<start>'])
        assert [sen_idx(s, wm) for s in got[0]] == c["sen"], (c["model"], c["end"], c["steps"])
        assert ok == ALL_OK


def _golden_engine(model, V, fc_scale, seed):
    from lrp_amd import weights
    img = lambda: torch.from_numpy(weights.make_images(seed + 7, 1))
    if model == "grid":
        from lrp_amd.explainers.gridtd import GridTDEngine
        eng = GridTDEngine(weights.scale_fc(weights.make_gridtd_state(seed=seed, vocab_size=V), fc_scale))
        return eng, eng.encode(img().cuda())
    if model == "bu":
        from lrp_amd.explainers.gridtd import GridTDBUEngine
        eng = GridTDBUEngine(weights.scale_fc(weights.make_gridtd_bu_state(seed=seed, vocab_size=V), fc_scale))
        return eng, eng.encode(torch.from_numpy(weights.make_bu_features(seed + 7, 1)).cuda())
    if model == "aoa":
        from lrp_amd.explainers.aoa import AOAEngine
        eng = AOAEngine(weights.scale_fc(weights.make_aoa_state(seed=seed, vocab_size=V), fc_scale))
        return eng, eng.encode(images=img().cuda())
    from lrp_amd.explainers.adaatt import AdaAttEngine
    eng = AdaAttEngine(weights.scale_fc(weights.make_adaatt_state(seed=seed, vocab_size=V), fc_scale))
    return eng, eng.encode(img())


@pytest.mark.parametrize("model,V", [("grid", 9586), ("bu", 9586), ("aoa", 11027), ("ada", 9586), ("grid", 37), ("bu", 37), ("aoa", 37), ("ada", 37)])
def test_engines_against_the_golden_runs(model, V):
    """`diverse_beam_search_batch` against the reference's `diverse_beam_search`, token for token: the cases of one seeded state that
    share beam size, length and diversity run as ONE batch - the same image with an <end> id per row - at their diversity and at 0"""
    _need_gpu()
    from test_dbs_host import sen_idx
    cases = [c for c in _golden() if c["model"] == model and c["V"] == V]
    assert cases
    for seed, fc_scale in sorted({(c["seed"], c["fc_scale"]) for c in cases}):
        eng, enc1 = _golden_engine(model, V, fc_scale, seed)
        mine = [c for c in cases if (c["seed"], c["fc_scale"]) == (seed, fc_scale)]
        for key in sorted({(c["beam"], c["steps"], c["div"]) for c in mine}):
            same = [c for c in mine if (c["beam"], c["steps"], c["div"]) == key]
            n = len(same)
            enc = {k: (v.expand(n, *v.shape[1:]).contiguous() if torch.is_tensor(v) else v) for k, v in enc1.items()}
            enc["B"] = n
            ends = [c["end"] for c in same]
            for div, want in ((key[2], "sen"), (0.0, "sen0")):
                got = diverse_beam_search_batch(eng, enc, key[0], key[1], same[0]["start"], ends, diversity_prob=div)
                for c, groups in zip(same, got):
                    assert [sen_idx(s, c["wm"]) for s in groups] == c[want], (model, V, seed, key, c["end"], want)
