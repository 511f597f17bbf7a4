"""The batched on-device beam search: `lrpx_beam_step_batch` alone against the host restatement of the reference's loop
(`oracle.lrp_oracle.beam_search`, models/gridTDmodel.py:400-478), `explainers.beam.beam_search_batch` against the reference's own captions
(tests/golden/beam.npz, adaatt.npz), and the property the engines promise: an image's sequence does not depend on what else is in the
batch and equals `beam_search` on that image, token for token."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN
from oracle import lrp_oracle as O

pytestmark = pytest.mark.gpu

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

START = 1
LIMIT = 1024          # LRPX_BEAM_MAX_STEPS (include/lrpx.h)
M = 8                 # the logits table has one row per (image, step, previous word % M)
STATE_W = 70          # width of the two stand-in state tensors: no multiple of the wave


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _table(seed, N, T, V):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, T, M, V, generator=g) * 4.0


def _state(N, k, V, T, toks, best, cum, best_score, n_live, best_len, live, end, state):
    from lrp_amd import _lib
    st = _lib.BeamBatch()
    st.N, st.k, st.V, st.T, st.start_id = N, k, V, T, START
    if torch.is_tensor(end):
        st.end_id, st.end_ids = -1, _lib.ptr(end)
    else:
        st.end_id, st.end_ids = int(end), None
    st.toks, st.tok_ld, st.best, st.best_ld = _lib.ptr(toks), toks.shape[1], _lib.ptr(best), best.shape[1]
    st.cum, st.best_score, st.n_live, st.best_len, st.live_images = (_lib.ptr(cum), _lib.ptr(best_score), _lib.ptr(n_live),
                                                                     _lib.ptr(best_len), _lib.ptr(live))
    st.n_state = len(state)
    for j, s in enumerate(state):
        st.state[j] = _lib.ptr(s)
    if state:
        st.state_w, st.state_ld = state[0].shape[2], state[0].shape[1] * state[0].shape[2]
    return st


def _device_search(L, k, T, ends):
    """the loop a caller runs, without a model: the scores of a row are L[image, t, previous word % M], gathered on the device - no host
    read before the end.  The two stand-in state tensors get, before every selection, a value that names the row's sequence; after it
    the value at a live row must name the row's NEW parent sequence (the state was gathered like the tokens).  Returns (sequences,
    `ok`: [state follows the tokens, rows of finished images untouched, rows that are not live hold <start>], n_live, live count)."""
    from lrp_amd import _lib
    lib, dev = _lib.load(), "cuda"
    N, V = L.shape[0], L.shape[3]
    rows = N * k
    Ld = L.to(dev)
    toks = torch.full((rows, T + 1), START, dtype=torch.int64, device=dev)
    best = torch.zeros(N, T + 1, dtype=torch.int64, device=dev)
    cum, best_score = torch.zeros(rows, device=dev), torch.zeros(N, device=dev)
    n_live = torch.full((N,), k, dtype=torch.int32, device=dev)
    best_len = torch.zeros(N, dtype=torch.int32, device=dev)
    live = torch.full((1,), N, dtype=torch.int32, device=dev)
    end = ends if isinstance(ends, int) else torch.tensor(ends, dtype=torch.int32, device=dev)
    state = [torch.zeros(rows, T + 1, STATE_W, device=dev) for _ in range(2)]
    st = _state(N, k, V, T, toks, best, cum, best_score, n_live, best_len, live, end, state)
    img = torch.arange(rows, device=dev) // k
    slot = (torch.arange(rows, device=dev) % k).to(torch.int32)
    pos_w = (torch.arange(T + 1, device=dev) % 13 + 1).double()
    col = torch.arange(STATE_W, device=dev).float()
    ok = torch.ones(3, dtype=torch.bool, device=dev)

    def name(t):          # a number < 2^24 (exact in fp32) that differs between an image's sequences of t + 1 tokens
        return ((toks[:, :t + 1].double() * pos_w[:t + 1]).sum(1) % 9973).float()
    for t in range(T):
        x = Ld[img, t, toks[:, t] % M].contiguous()
        ident = name(t)
        for j, s in enumerate(state):
            s[:, t + 1] = ident[:, None] * (j + 1) + col[None, :]
        before = [toks.clone(), cum.clone(), best.clone()] + [s.clone() for s in state]
        dead = (n_live == 0)
        _lib.check(lib.lrpx_beam_step_batch(C.byref(st), _lib.ptr(x), V, t, _lib.stream_ptr()))
        dead_row = dead[img]
        for b, a in zip(before, [toks, cum, best] + state):
            d = dead if a.shape[0] == N else dead_row
            same = (a == b).reshape(a.shape[0], -1).all(1)
            ok[1] &= (same | ~d).all()
        live_row = slot < n_live[img]
        want = name(t)                # the tokens were gathered by `src`; so must the state have been
        for j, s in enumerate(state):
            good = (s[:, t + 1] == want[:, None] * (j + 1) + col[None, :]).all(1)
            ok[0] &= (good | ~live_row).all()
        ok[2] &= ((toks[:, t + 1] == START) | live_row).all()
    out = torch.empty(N, T + 2, dtype=torch.int64, device=dev)
    _lib.check(lib.lrpx_beam_result_batch(C.byref(st), T, _lib.ptr(out), T + 2, _lib.stream_ptr()))
    host = out.cpu()
    return [host[i, 1:1 + int(host[i, 0])].tolist() for i in range(N)], ok.cpu().tolist(), n_live.cpu().tolist(), int(live.item())


def _oracle(L, i, k, T, end):
    return O.beam_search(lambda seqs: torch.stack([L[i, len(s) - 1, s[-1] % M] for s in seqs]), L.shape[3], k, T, START, end)


def _stable(L, i, k, T, end):
    """the same loop with the selection spelt out - descending score, ascending flat index - for the cases that rest on exact ties
    (a library top-k promises no order among equal values)"""
    V = L.shape[3]
    seqs, cum, complete, n_live = [[START] for _ in range(k)], torch.zeros(k), [], k
    for t in range(T):
        sc = cum[:n_live, None] + torch.log_softmax(torch.stack([L[i, t, s[-1] % M] for s in seqs]), dim=-1)
        flat = (sc[0] if t == 0 else sc.reshape(-1)).tolist()
        top = sorted(range(len(flat)), key=lambda f: (-flat[f], f))[:k if t == 0 else n_live]
        seqs = [seqs[f // V] + [f % V] for f in top]
        inc = [j for j, f in enumerate(top) if f % V != end]
        complete += [(flat[f], seqs[j]) for j, f in enumerate(top) if f % V == end]
        n_live = len(inc)
        if n_live == 0:
            break
        seqs, cum = [seqs[j] for j in inc], torch.tensor([flat[top[j]] for j in inc])
    if complete:
        best = complete[0]
        for c in complete[1:]:
            if c[0] > best[0]:
                best = c
        return best[1]
    return seqs[0][:20]


@pytest.mark.parametrize("V", [37, 9586])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_step_kernel_vs_host_restatement(V, k):
    """N = 3 images with an <end> id each, 20 steps: image 0 free, image 1 with <end> as the best first word (the empty caption for k = 1,
    else the first complete sequence, which no later one beats), image 2 never completing (cut at 20 tokens)"""
    _need_gpu()
    N, T = 3, 20
    L = _table(100 + k, N, T, V)
    ends = [5, 7, 11]
    L[1, 0, START % M, ends[1]] = 40.0
    L[2, :, :, ends[2]] = -60.0
    got, ok, n_live, live = _device_search(L, k, T, ends)
    want = [_oracle(L, i, k, T, ends[i]) for i in range(N)]
    assert got == want
    assert ok == [True, True, True]
    assert got[1] == [START, ends[1]] and len(got[2]) == 20 and n_live[2] == k
    assert live == sum(1 for n in n_live if n > 0)


@pytest.mark.parametrize("T", [1, 5, LIMIT])
def test_step_kernel_lengths(T):
    """max_cap_length 1 and 5 (one image) and the documented limit (include/lrpx.h: LRPX_BEAM_MAX_STEPS; two images): at the limit image 0
    never completes and image 1 does at the last step, so both ends of the sequence storage are written"""
    _need_gpu()
    N, k, V = (2 if T == LIMIT else 1), 2, 37
    L = _table(7 + T, N, T, V)
    end = 9
    L[0, :, :, end] = -60.0
    if T == LIMIT:
        L[1, :T - 1, :, end] = -60.0
        L[1, T - 1, :, end] = 60.0
    got, ok, n_live, _ = _device_search(L, k, T, end)
    assert got == [_oracle(L, i, k, T, end) for i in range(N)]
    assert ok == [True, True, True]
    assert len(got[0]) == min(T + 1, 20)
    if T == LIMIT:
        assert len(got[1]) == T + 1 and got[1][-1] == end and n_live == [k, 0]


def test_step_kernel_32_images():
    _need_gpu()
    N, k, T, V = 32, 2, 5, 37
    L = _table(3, N, T, V)
    ends = [(3 * i) % V for i in range(N)]
    got, ok, _, _ = _device_search(L, k, T, ends)
    assert got == [_oracle(L, i, k, T, ends[i]) for i in range(N)]
    assert ok == [True, True, True]


def test_all_beams_complete_at_step_2_next_to_an_image_that_never_does():
    """image 0: every live row's best word at step 2 is <end> - all beams complete there, the image is a no-op for the 22 steps that follow
    (its rows of tokens, scores, state and its kept sequence are compared before / after every later launch); image 1 runs to the end"""
    _need_gpu()
    k, T, V, end = 3, 25, 37, 4
    L = _table(11, 2, T, V)
    L[:, :2, :, end] = -60.0
    L[0, 2, :, end] = 60.0
    L[1, :, :, end] = -60.0
    got, ok, n_live, live = _device_search(L, k, T, end)
    assert got == [_oracle(L, i, k, T, end) for i in range(2)]
    assert len(got[0]) == 4 and got[0][-1] == end and len(got[1]) == 20
    assert ok == [True, True, True] and n_live == [0, k] and live == 1


def test_exact_ties():
    """Exact ties, decided as the reference's loop decides them.  Step 0: words a < b with the same score - a first (lower index in the
    row).  Their rows of step 1 are identical and so are their cumulative scores: every candidate of row 0 ties with the same word of
    row 1, the lower FLAT index (row 0) wins.  Image 0: that best word is <end> - two complete sequences with exactly equal scores in
    one step, the first ([<start>, a, <end>]) is kept.  Image 1: it is an ordinary word w - the two best are (row 0, w), (row 1, w)."""
    _need_gpu()
    k, T, V, end = 2, 4, 37, 6
    a, b, w = 10, 19, 23                   # a % M = 2, b % M = 3
    L = _table(21, 2, T, V)
    L[:, :, :, end] = -60.0
    for i in range(2):
        L[i, 0, START % M, a] = L[i, 0, START % M, b] = 30.0
        L[i, 1, b % M] = L[i, 1, a % M]
    L[0, 1, a % M, end] = L[0, 1, b % M, end] = 50.0
    L[1, 1, a % M, w] = L[1, 1, b % M, w] = 50.0
    got, ok, _, _ = _device_search(L, k, T, end)
    want = [_stable(L, i, k, T, end) for i in range(2)]
    assert got == want and ok == [True, True, True]
    assert got[0] == [START, a, end]
    assert got[1][:3] == [START, a, w]


def test_refusals_give_an_error_code_and_launch_nothing():
    """k = 5, max_cap_length above the limit, a host pointer: LRPX_EINVAL, and the state on the device is as it was"""
    _need_gpu()
    from lrp_amd import _lib
    lib, dev = _lib.load(), "cuda"
    N, k, V, T = 2, 2, 37, 5

    def fresh(T):
        toks = torch.full((N * 5, T + 1), START, dtype=torch.int64, device=dev)
        return dict(toks=toks, best=torch.zeros(N, T + 1, dtype=torch.int64, device=dev), cum=torch.zeros(N * 5, device=dev),
                    best_score=torch.zeros(N, device=dev), n_live=torch.full((N,), k, dtype=torch.int32, device=dev),
                    best_len=torch.zeros(N, dtype=torch.int32, device=dev), live=torch.full((1,), N, dtype=torch.int32, device=dev))
    x = torch.randn(N * 5, V, device=dev)
    for what, kk, TT, xp in (("k = 5", 5, T, None), ("max_cap_length", k, LIMIT + 1, None), ("host pointer", k, T, "host")):
        b = fresh(TT)
        keep = {n: v.clone() for n, v in b.items()}
        st = _state(N, kk, V, TT, b["toks"], b["best"], b["cum"], b["best_score"], b["n_live"], b["best_len"], b["live"], 3, [])
        xh = torch.randn(N * 5, V)
        px = C.c_void_p(xh.data_ptr()) if xp else _lib.ptr(x)
        rc = lib.lrpx_beam_step_batch(C.byref(st), px, V, 0, _lib.stream_ptr())
        assert rc == _lib.EINVAL, what
        msg = lib.lrpx_last_error_string().decode()
        assert "beam_step_batch" in msg, msg
        torch.cuda.synchronize()
        for n, v in b.items():
            assert torch.equal(v, keep[n]), (what, n)
    with pytest.raises(ValueError):
        _lib.check(_lib.EINVAL)


# ---- the engines ------------------------------------------------------------------------------------------------------------------------
def _golden_batch(eng, enc1, g, tag, cases):
    from lrp_amd.explainers.beam import beam_search_batch, caption_from_sequence
    n = len(cases)
    enc = {k: (v.expand(n, *v.shape[1:]).contiguous() if torch.is_tensor(v) else v) for k, v in enc1.items()}
    enc["B"] = n
    start = cases[0][1]['<start>']
    seqs = beam_search_batch(eng, enc, int(g[f"{tag}_beam"]), int(g[f"{tag}_steps"]), start, [wm['<end>'] for _, wm in cases])
    for (key, wm), seq in zip(cases, seqs):
        assert caption_from_sequence(seq, wm)[1:] == g[f"{tag}_{key}"].tolist(), (tag, key)
    return seqs


def test_grid_goldens_as_one_batch():
    """the four `grid_*` captions of tests/golden/beam.npz - the natural run (cut at 20), an <end> that is reached, <end> as first word, a
    dropped <unk> - as ONE batch of four rows-pairs with an <end> id each: images finish at different steps.  Token ids bit-exact."""
    _need_gpu()
    from lrp_amd import weights
    from lrp_amd.explainers.gridtd import GridTDEngine
    from test_oracle_golden import _beam_cases
    g = np.load(os.path.join(GOLDEN, "beam.npz"))
    V, cases = _beam_cases(g, "grid")
    eng = GridTDEngine(weights.make_gridtd_state(seed=int(g["seed"]), vocab_size=V))
    enc = eng.encode(torch.from_numpy(weights.make_images(int(g["seed"]) + 7, 1)).cuda())
    seqs = _golden_batch(eng, enc, g, "grid", cases)
    assert len({len(s) for s in seqs}) > 1
    wm = cases[1][1]
    from lrp_amd.explainers.beam import caption_batch
    assert caption_batch(eng, enc, wm, int(g["grid_beam"]), int(g["grid_steps"])) == [[wm['<start>']] + g["grid_sen_end"].tolist()]


def test_aoa_goldens_as_one_batch():
    _need_gpu()
    from lrp_amd import weights
    from lrp_amd.explainers.aoa import AOAEngine
    from test_oracle_golden import _beam_cases
    g = np.load(os.path.join(GOLDEN, "beam.npz"))
    V, cases = _beam_cases(g, "aoa")
    eng = AOAEngine(weights.make_aoa_state(seed=int(g["seed"]), vocab_size=V))
    enc = eng.encode(images=torch.from_numpy(weights.make_images(int(g["seed"]) + 7, 1)).cuda())
    _golden_batch(eng, enc, g, "aoa", cases)


def test_adaatt_golden():
    _need_gpu()
    from lrp_amd import weights
    from lrp_amd.explainers.adaatt import AdaAttEngine
    from lrp_amd.explainers.beam import beam_search_batch, caption_from_sequence
    with np.load(os.path.join(GOLDEN, "adaatt.npz"), allow_pickle=False) as f:
        g = {k: f[k] for k in f.files}
    V = int(g["V"])
    wm = weights.make_word_map(V)
    eng = AdaAttEngine(weights.make_adaatt_state(seed=int(g["seed"]), vocab_size=V))
    enc = eng.encode(torch.from_numpy(weights.make_images(int(g["seed"]), 1)))
    seq, = beam_search_batch(eng, enc, int(g["decode_beam_size"]), int(g["decode_beam_steps"]), wm['<start>'], wm['<end>'])
    assert caption_from_sequence(seq, wm)[1:] == g["decode_beam"].tolist()


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


def _one(enc, i):
    e = {k: (v[i:i + 1].contiguous() if torch.is_tensor(v) else v) for k, v in enc.items()}
    e["B"] = 1
    return e


@pytest.fixture(scope="module", params=["grid", "aoa", "bu", "ada"])
def searched(request):
    """per engine: 33 seeded images encoded ONCE, and `beam_search` on each of them alone at beam 2 (all 33) and beam 3 (the first 22) -
    the reference every case below compares with, computed once"""
    _need_gpu()
    eng, encode = _engine(request.param)
    enc = encode(33)
    T, start = 12, 1
    # an <end> id per image, taken from the words the image's own free run produces (random weights never produce a fixed id): position
    # 2 .. 6 of that run, and every third image keeps an id no word has - the images of one batch finish at different steps
    free = [eng.beam_search(_one(enc, i), 2, T, start, -1) for i in range(33)]
    ends = [-1 if i % 3 == 0 else free[i][2 + i % 5] for i in range(33)]
    alone = {2: [eng.beam_search(_one(enc, i), 2, T, start, ends[i]) for i in range(33)],
             3: [eng.beam_search(_one(enc, i), 3, T, start, ends[i]) for i in range(22)]}
    return eng, enc, T, start, ends, alone


def _first(enc, n):
    e = {k: (v[:n] if torch.is_tensor(v) else v) for k, v in enc.items()}
    e["B"] = n
    return e


@pytest.mark.parametrize("beam,n", [(2, 5), (2, 32), (2, 33), (3, 21), (3, 22)])
def test_a_sequence_does_not_depend_on_the_batch(searched, beam, n):
    """`beam_search_batch` on n images equals `beam_search` on each alone, token for token: 5 images, 32 / 33 at beam 2 and 21 / 22 at
    beam 3 (64 and 63 rows in one launch; one image more is a second chunk), and the same with the live count polled at every step"""
    from lrp_amd.explainers.beam import beam_search_batch
    eng, enc, T, start, ends, alone = searched
    got = beam_search_batch(eng, _first(enc, n), beam, T, start, ends[:n])
    assert got == alone[beam][:n]
    assert len({len(s) for s in got}) > 1, "the images of this batch were meant to finish at different steps"
    assert beam_search_batch(eng, _first(enc, n), beam, T, start, ends[:n], poll=1) == got
