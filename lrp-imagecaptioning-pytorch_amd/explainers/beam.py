"""Host bookkeeping of the reference's beam search (`GridTDModel.beam_search`, models/gridTDmodel.py:400-478;
`AOAModel.beam_search`, models/aoamodel.py, the same algorithm) around device steps: the explainers caption the image
with it (`get_hidden_parameters`, models/gridTDmodel.py:935: beam 2, 50 steps; models/aoamodel.py:992: beam 3, 20 steps)
before they explain, so a drop-in without `caption_encode=` has to decode the same caption.

The model step, the logits and the top-k (`lrpx_beam_topk`: log-softmax + cumulative score + k best over the live beams)
run on the device; what happens here is what the reference does in Python lists too (sequence bookkeeping, `<end>`
detection - one small device->host read per step, as the reference's `enumerate(next_word_idx)`)."""
import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr


def run_beam_search(step, logits, reorder, vocab, beam_size, max_cap_length, start_id, end_id, device):
    """step(t, prev_words): model step t for all `beam_size` rows (prev_words: int64 device tensor, live rows first);
    logits(t) -> (beam_size, vocab) scores of step t; reorder(t, src): state row j of time t+1 <- row src[j].
    Returns the chosen sequence incl. <start> (and <end> if it was produced), as the reference's `seq`."""
    lib = _lib.load()
    assert 1 <= beam_size <= 4, "lrpx_beam_topk keeps at most 4 candidates"
    seqs = [[start_id] for _ in range(beam_size)]
    cum = torch.zeros(beam_size, dtype=torch.float32, device=device)
    prev = torch.full((beam_size,), start_id, dtype=torch.int64, device=device)
    # indices (4 x int64) and scores (4 x float32) of a step in ONE 48-byte buffer: one device -> host read per step instead of two
    buf = torch.zeros(6, dtype=torch.int64, device=device)
    idx, val = buf[:4], buf[4:].view(torch.float32)
    complete, complete_scores = [], []
    n_live = beam_size
    for t in range(max_cap_length):
        step(t, prev)
        lg = logits(t)
        rows, k = (1, beam_size) if t == 0 else (n_live, n_live)          # :440-443
        check(lib.lrpx_beam_topk(ptr(lg), lg.shape[1], rows, vocab, ptr(cum), k, ptr(idx), ptr(val), stream_ptr()))
        host = buf.cpu()
        top, sc = host[:k].tolist(), host[4:].view(torch.float32)[:k].tolist()
        beam_idx = [w // vocab for w in top]                               # :444 (floor division: PyTorch 1.4 `/` on int64)
        nxt = [w % vocab for w in top]
        seqs = [seqs[b] + [w] for b, w in zip(beam_idx, nxt)]              # :447
        inc = [i for i, w in enumerate(nxt) if w != end_id]                # :448
        for i in sorted(set(range(len(nxt))) - set(inc)):                  # :449-453
            complete.append(seqs[i])
            complete_scores.append(sc[i])
        n_live = n_live - (len(nxt) - len(inc))
        if n_live == 0:
            break
        seqs = [seqs[i] for i in inc]                                      # :458
        reorder(t, [beam_idx[i] for i in inc])                             # :460-465
        cum[:n_live] = torch.tensor([sc[i] for i in inc], dtype=torch.float32, device=device)
        prev[:n_live] = torch.tensor([nxt[i] for i in inc], dtype=torch.int64, device=device)
    if complete:
        return complete[complete_scores.index(max(complete_scores))]       # :469-470
    return seqs[0][:20]                                                    # :472 (the cut at 20 tokens is the reference's)


BEAM_ROWS = 64      # rows per launch of a batched beam search: up to here `lrpx_linear_small` stays on the kernel `beam_search` runs


def beam_search_batch(engine, enc, beam_size, max_cap_length, start_id, end_id, poll=None):
    """`engine.beam_search` for every image of `enc` at once, on any caption engine (explainers/engine_base.py: its hooks `_decode_trace`,
    `_decode_step`, `logits`, `_BEAM_STATE`): a list of enc["B"] token lists, each what `beam_search` returns for that image alone, token
    for token.  Image i owns `beam_size` rows of the decoder trace; selection, sequence bookkeeping and the re-order of the LSTM state
    are one launch per step (`lrpx_beam_step_batch`), and nothing is read back before the end.  More than `BEAM_ROWS` rows are split
    into chunks of whole images (above 64 rows the skinny linear sums in another order).  `end_id`: one id, or one per image.  `poll`:
    every `poll` steps the device's count of images with live beams is read, and the loop stops when it is 0; the result does not
    depend on it.  A function, not an engine method: the engines' public surface is the recorded one (tests/test_explainer_api_host.py).
    Not one of the static-buffer drivers (no HIP graph, no recording)."""
    N, nb, T = int(enc["B"]), int(beam_size), int(max_cap_length)
    if not 1 <= nb <= 4:
        raise ValueError("beam_search_batch: beam_size {} (lrpx_beam_step_batch keeps 1..4 beams)".format(nb))
    ends = _end_ids("beam_search_batch", end_id, N, engine.device)
    per = max(1, BEAM_ROWS // nb)
    out = []
    for i0 in range(0, N, per):
        i1 = min(N, i0 + per)
        sub = {k: (v[i0:i1] if torch.is_tensor(v) else v) for k, v in enc.items()}
        sub["B"] = i1 - i0
        out += _beam_chunk(engine, sub, nb, T, int(start_id), end_id if ends is None else ends[i0:i1].contiguous(), poll)
    return out


def _beam_chunk(engine, enc, nb, T, start_id, end_id, poll):
    lib, dev, n = _lib.load(), engine.device, enc["B"]
    rows = n * nb
    encb = {k: (v.repeat_interleave(nb, 0).contiguous() if torch.is_tensor(v) else v) for k, v in enc.items()}
    encb["B"] = rows
    tr = engine._decode_trace(encb, rows, T)
    toks = torch.full((rows, T + 1), start_id, dtype=torch.int64, device=dev)      # rows that are not live feed a valid id to the embedding
    best = torch.zeros(n, T + 1, dtype=torch.int64, device=dev)
    cum, best_score = torch.zeros(rows, device=dev), torch.zeros(n, device=dev)
    n_live = torch.full((n,), nb, dtype=torch.int32, device=dev)
    best_len = torch.zeros(n, dtype=torch.int32, device=dev)
    live = torch.full((1,), n, dtype=torch.int32, device=dev)
    st = _lib.BeamBatch()
    st.N, st.k, st.V, st.T, st.start_id = n, nb, engine.V, T, start_id
    if torch.is_tensor(end_id):
        st.end_id, st.end_ids = -1, ptr(end_id)
    else:
        st.end_id, st.end_ids = int(end_id), None
    st.toks, st.tok_ld, st.best, st.best_ld = ptr(toks), T + 1, ptr(best), T + 1
    st.cum, st.best_score, st.n_live, st.best_len, st.live_images = ptr(cum), ptr(best_score), ptr(n_live), ptr(best_len), ptr(live)
    state = [tr[k] for k in engine._BEAM_STATE]
    st.n_state = len(state)
    for j, s in enumerate(state):
        assert s.shape[0] == rows and s.shape[1] == T + 1 and s.shape[2:] == state[0].shape[2:]
        st.state[j] = ptr(s)
    if state:
        st.state_w = int(state[0][0, 0].numel())
        st.state_ld = (T + 1) * st.state_w
    steps = 0
    for t in range(T):
        engine._decode_step(tr, encb, t, toks)
        lg = engine.logits(tr["hc"][:, t].contiguous())
        check(lib.lrpx_beam_step_batch(_lib.C.byref(st), ptr(lg), lg.shape[1], t, stream_ptr()))
        steps = t + 1
        if poll and steps % int(poll) == 0 and steps < T and int(live.item()) == 0:
            break
    res = torch.empty(n, T + 2, dtype=torch.int64, device=dev)
    check(lib.lrpx_beam_result_batch(_lib.C.byref(st), steps, ptr(res), T + 2, stream_ptr()))
    host = res.cpu()                                   # the one device -> host read of the search
    return [host[i, 1:1 + int(host[i, 0])].tolist() for i in range(n)]


def _end_ids(who, end_id, N, device):
    import numpy as np
    if isinstance(end_id, (int, np.integer)):
        return None
    ends = torch.as_tensor(end_id).to(device, torch.int32).contiguous()
    if ends.shape != (N,):
        raise ValueError("{}: end_id must be one id or one per image ({}), got shape {}".format(who, N, tuple(ends.shape)))
    return ends


def diverse_beam_search_batch(engine, enc, beam_size, max_cap_length, start_id, end_id, diversity_prob=0.5, poll=None):
    """The reference's `diverse_beam_search` (models/gridTDmodel.py:304-398, and the same loop in the other four model classes) for every
    image of `enc` at once, on any caption engine (the hooks of `beam_search_batch`): a list of enc["B"] lists of G = `beam_size` token
    lists - the reference's `seq` of each group, incl. <start> (and <end> where the group completed a sequence).  The reference takes one
    image and walks its groups in Python; here image i owns G * beam_size rows of the decoder trace, the groups of every image select in
    ONE launch per step (`lrpx_dbs_step_batch`, include/lrpx.h: the penalty of `diversity_prob` on the input words of groups 0 and 1,
    the `break` that passes the later groups over, the fallback to group 0's first sequence), and nothing is read back before the end.
    Chunks are whole images of at most `BEAM_ROWS` rows: 16 images at beam 2, 7 at beam 3, 4 at beam 4.  `end_id`: one id, or one per
    image.  `poll`: as in `beam_search_batch`; the result does not depend on it."""
    N, nb, T = int(enc["B"]), int(beam_size), int(max_cap_length)
    if not 1 <= nb <= 4:
        raise ValueError("diverse_beam_search_batch: beam_size {} (lrpx_dbs_step_batch keeps 1..4 groups of as many beams)".format(nb))
    ends = _end_ids("diverse_beam_search_batch", end_id, N, engine.device)
    per = max(1, BEAM_ROWS // (nb * nb))
    out = []
    for i0 in range(0, N, per):
        i1 = min(N, i0 + per)
        sub = {k: (v[i0:i1] if torch.is_tensor(v) else v) for k, v in enc.items()}
        sub["B"] = i1 - i0
        out += _dbs_chunk(engine, sub, nb, T, int(start_id), end_id if ends is None else ends[i0:i1].contiguous(), float(diversity_prob), poll)
    return out


def _dbs_chunk(engine, enc, nb, T, start_id, end_id, diversity, poll):
    lib, dev, n = _lib.load(), engine.device, enc["B"]
    groups, rows = n * nb, n * nb * nb
    encb = {k: (v.repeat_interleave(nb * nb, 0).contiguous() if torch.is_tensor(v) else v) for k, v in enc.items()}
    encb["B"] = rows
    tr = engine._decode_trace(encb, rows, T)
    toks = torch.full((rows, T + 1), start_id, dtype=torch.int64, device=dev)      # the decoder's inputs; rows that are not live feed <start>
    seqs = torch.full((rows, T + 1), start_id, dtype=torch.int64, device=dev)      # the sequences: a group that was passed over is shorter
    best = torch.zeros(groups, T + 1, dtype=torch.int64, device=dev)
    cum, best_score = torch.zeros(rows, device=dev), torch.zeros(groups, device=dev)
    n_live = torch.full((groups,), nb, dtype=torch.int32, device=dev)
    seq_len = torch.ones(groups, dtype=torch.int32, device=dev)
    best_len = torch.zeros(groups, dtype=torch.int32, device=dev)
    live = torch.full((1,), n, dtype=torch.int32, device=dev)
    st = _lib.DbsBatch()
    st.N, st.k, st.G, st.V, st.T, st.start_id, st.diversity = n, nb, nb, engine.V, T, start_id, diversity
    if torch.is_tensor(end_id):
        st.end_id, st.end_ids = -1, ptr(end_id)
    else:
        st.end_id, st.end_ids = int(end_id), None
    st.toks, st.tok_ld, st.seqs, st.seq_ld, st.best, st.best_ld = ptr(toks), T + 1, ptr(seqs), T + 1, ptr(best), T + 1
    st.cum, st.best_score, st.n_live, st.seq_len = ptr(cum), ptr(best_score), ptr(n_live), ptr(seq_len)
    st.best_len, st.live_images = ptr(best_len), ptr(live)
    state = [tr[k] for k in engine._BEAM_STATE]
    st.n_state = len(state)
    for j, s in enumerate(state):
        assert s.shape[0] == rows and s.shape[1] == T + 1 and s.shape[2:] == state[0].shape[2:]
        st.state[j] = ptr(s)
    if state:
        st.state_w = int(state[0][0, 0].numel())
        st.state_ld = (T + 1) * st.state_w
    for t in range(T):
        engine._decode_step(tr, encb, t, toks)
        lg = engine.logits(tr["hc"][:, t].contiguous())
        check(lib.lrpx_dbs_step_batch(_lib.C.byref(st), ptr(lg), lg.shape[1], t, stream_ptr()))
        if poll and (t + 1) % int(poll) == 0 and t + 1 < T and int(live.item()) == 0:
            break
    res = torch.empty(groups, T + 2, dtype=torch.int64, device=dev)
    check(lib.lrpx_dbs_result_batch(_lib.C.byref(st), ptr(res), T + 2, stream_ptr()))
    host = res.cpu()                                   # the one device -> host read of the search
    return [[host[i * nb + g, 1:1 + int(host[i * nb + g, 0])].tolist() for g in range(nb)] for i in range(n)]


def diverse_captions_batch(engine, enc, word_map, beam_size, max_cap_length, diversity_prob=0.5, bad_ending_ids=None):
    """the G captions per image `diverse_beam_search` returns, as ids: `[<start>] + sen_idx` per group (:391-392), with
    `remove_bad_endings` (:284-302, :396) at id level where `bad_ending_ids` is given - ready for `explain_batch(..., lens=)`"""
    from .ablation import trim_bad_endings
    seqs = diverse_beam_search_batch(engine, enc, beam_size, max_cap_length, word_map['<start>'], word_map['<end>'], diversity_prob)
    caps = [[caption_from_sequence(s, word_map) for s in groups] for groups in seqs]
    if bad_ending_ids is not None:
        bad = list(bad_ending_ids)                     # (trim_bad_endings makes the set)
        caps = [[c[:1] + trim_bad_endings(c[1:], bad) for c in groups] for groups in caps]
    return caps


def caption_batch(engine, enc, word_map, beam_size, max_cap_length):
    """the captions the explainers explain (`[<start>] + sen_idx`, models/gridTDmodel.py:474, :937) for every image of `enc`"""
    seqs = beam_search_batch(engine, enc, beam_size, max_cap_length, word_map['<start>'], word_map['<end>'])
    return [caption_from_sequence(s, word_map) for s in seqs]


def caption_from_sequence(seq, word_map):
    """`sen_idx` (:474): the sequence without <start>, <end>, <unk>, <pad>; the explainers prepend <start> (:937)."""
    drop = {word_map[k] for k in ('<start>', '<end>', '<unk>', '<pad>') if k in word_map}
    return [word_map['<start>']] + [int(w) for w in seq if w not in drop]
