"""The device work of the reference's ablation experiment (`EvaluationExperiments.ablation_experiment`, evaluation.py:82-311), batched.

Image ablation (:120-156): per explained word the 20 most relevant 8 x 8 patches are masked (`evaluation.block_image`), the masked image is
captioned again (`beam_search_batch`), the word is looked up in the new caption and the prefix before it is teacher-forced on the masked
image.  Word ablation (:234-253): the three most relevant preceding words are deleted (`lrpx_delete_topk_tokens`) and the shortened
caption is teacher-forced on the image itself.  The score of a word is `softmax(scores)[word]` (`lrpx_softmax_pick_rows`); the
differences the reference reports are the caller's subtraction.

Id-level by design: which words are object words or stop words, the plural stripping and the bad endings are word lists of the caller -
the entry points take rows, ids and id sets.  Rows are (image, word) pairs in any order; `row2img` names a row's image."""
import torch

from .. import _lib, evaluation
from .._lib import check, ptr, stream_ptr
from .beam import beam_search_batch

ROWS = 64          # rows per launch, as in `beam.beam_search_batch`: an image's numbers never depend on its batch
# masked images encoded at once: the engines' `encode` forms proj_pre / att_img with one GEMM over all (image, pixel) rows, which stays on
# one kernel (`dense_small`, csrc/dense_small.hip) up to 4096 rows - 16 images of at most 256 pixels; 21 images of 196 pixels take another
# kernel, which sums in another order
ENC_IMAGES = 16


def _rows(engine, x, n=None):
    x = torch.as_tensor(x)
    if n is not None and x.shape[:1] != (n,):
        raise ValueError("ablation: expected {} rows, got shape {}".format(n, tuple(x.shape)))
    return x.to(engine.device)


def softmax_pick(engine, scores, ids):
    """softmax(scores[r])[ids[r]] for (R, V) scores -> (R,)"""
    scores = scores.to(engine.device, torch.float32).contiguous()
    ids = ids.to(engine.device, torch.int64).contiguous()
    out = torch.empty(scores.shape[0], device=engine.device, dtype=torch.float32)
    if scores.shape[0]:
        check(_lib.load().lrpx_softmax_pick_rows(ptr(scores), scores.shape[1], scores.shape[0], scores.shape[1], ptr(ids), ptr(out), stream_ptr()))
    return out


def word_prob(engine, predictions, t_rows, targets, row2img=None):
    """the original score of a row's word (evaluation.py:122, :236): softmax(predictions[row2img[r], t_rows[r]])[targets[r]].
    predictions (B, T, V); row2img=None: row r is image r."""
    t = _rows(engine, t_rows).to(torch.int64)
    img = torch.arange(t.shape[0], device=engine.device) if row2img is None else _rows(engine, row2img, t.shape[0]).to(torch.int64)
    return softmax_pick(engine, predictions.to(engine.device)[img, t], _rows(engine, targets, t.shape[0]))


def _enc_rows(enc, idx):
    e = {k: (v[idx].contiguous() if torch.is_tensor(v) else v) for k, v in enc.items()}
    e["B"] = int(idx.shape[0])
    return e


def _teacherforce_last(engine, enc, caps, lens, targets, model_bias):
    """ONE teacher-forced trace over padded captions (n, L + 1) (column 0 = <start>, zeros behind a caption's `lens` tokens) on the n
    rows of `enc`; the scores are formed for the last valid step of each caption only -> softmax(scores)[targets] (n,)"""
    n, L = caps.shape[0], caps.shape[1] - 1
    tr = engine.trace(enc, caps, model_bias=model_bias, predictions=False)
    hc = tr["hc"].view(n, L, engine.H)[torch.arange(n, device=engine.device), lens.to(torch.int64) - 1]
    return softmax_pick(engine, engine.logits(hc.contiguous()), targets)


def delete_topk_tokens(engine, captions, t_rows, r_words, kdel=3):
    """evaluation.py:242-247 for R rows: the caption prefix captions[r, :t + 1] without its `kdel` most relevant words among 1 .. t
    (`1 + topk(r_words[r, 1:t + 1], kdel)`; <start> is never a candidate; ties: the earlier word).  Returns (short (R, max t + 2) int64,
    zeros behind a row's tokens, lens (R,) int32, deleted (R, kdel) int32: the dropped positions, most relevant first)."""
    dev = engine.device
    t_host = [int(v) for v in torch.as_tensor(t_rows).tolist()]
    R = len(t_host)
    captions = _rows(engine, captions, R).to(torch.int64).contiguous()
    r_words = _rows(engine, r_words, R).to(torch.float32).contiguous()
    if R == 0 or min(t_host) < 0 or max(t_host) >= captions.shape[1] or max(t_host) >= r_words.shape[1]:
        raise ValueError("delete_topk_tokens: a row needs t + 1 caption tokens and t + 1 relevances (t = {}, captions {}, r_words {})".format(
            t_host, tuple(captions.shape), tuple(r_words.shape)))
    t_dev = torch.tensor(t_host, dtype=torch.int32, device=dev)
    L = max(t_host) + 1
    short = torch.zeros(R, L + 1, dtype=torch.int64, device=dev)
    lens = torch.empty(R, dtype=torch.int32, device=dev)
    deleted = torch.empty(R, max(int(kdel), 1), dtype=torch.int32, device=dev)
    check(_lib.load().lrpx_delete_topk_tokens(ptr(captions), captions.shape[1], ptr(r_words), r_words.shape[1], ptr(t_dev), R, int(kdel),
                                              ptr(short), L + 1, ptr(lens), ptr(deleted), stream_ptr()))
    return short, lens, deleted[:, :int(kdel)]


def delete_tokens(engine, captions, t_rows, delete_ids):
    """evaluation.py:268-269 for R rows: `np.delete(captions[r, :t + 1], delete_ids[r])` with positions the caller drew (the random arm:
    `random.sample(range(1, t), 3)`).  As np.delete: a position counts once however often it is named, negative positions count from
    the end of the prefix, positions outside it are an IndexError.  Returns (short (R, max t + 2) int64, zeros behind a row's tokens,
    lens (R,) int32).  Host index arithmetic on a few ids per row; the teacher-forced pass is the device work."""
    t_host = [int(v) for v in torch.as_tensor(t_rows).tolist()]
    R = len(t_host)
    captions = _rows(engine, captions, R).to(torch.int64)
    ids = torch.as_tensor(delete_ids).to(torch.int64).cpu()
    if ids.dim() != 2 or ids.shape[0] != R:
        raise ValueError("delete_tokens: delete_ids must be (rows, kdel) positions for {} rows, got {}".format(R, tuple(ids.shape)))
    if R == 0 or min(t_host) < 0 or max(t_host) >= captions.shape[1]:
        raise ValueError("delete_tokens: a row needs t + 1 caption tokens (t = {}, captions {})".format(t_host, tuple(captions.shape)))
    cap_host = captions.cpu().tolist()
    L = max(t_host) + 1
    short = torch.zeros(R, L + 1, dtype=torch.int64)
    lens = torch.empty(R, dtype=torch.int32)
    for r, t in enumerate(t_host):
        gone = set()
        for d in ids[r].tolist():
            if d < -(t + 1) or d > t:
                raise IndexError("delete_tokens: position {} is out of bounds for the {} tokens of row {}".format(d, t + 1, r))
            gone.add(d % (t + 1))
        keep = [c for pos, c in enumerate(cap_host[r][:t + 1]) if pos not in gone]
        if not keep:
            raise ValueError("delete_tokens: row {} would be left without a token to teacher-force".format(r))
        short[r, :len(keep)] = torch.tensor(keep, dtype=torch.int64)
        lens[r] = len(keep)
    return short.to(engine.device), lens.to(engine.device)


def word_ablation(engine, enc, row2img, captions, t_rows, r_words, kdel=3, model_bias=False, delete_ids=None):
    """Row r explains word t = t_rows[r] of image row2img[r]: captions[r] holds its caption incl. <start> (at least t + 2 tokens),
    r_words[r, :t + 1] the relevance of the words before it.  The `kdel` most relevant of the words 1 .. t are deleted
    (`delete_topk_tokens`), the shortened prefix is teacher-forced on the image's own encoding `enc`, and the probability of
    captions[r, t + 1] at its last step is returned: new_prob (R,) (evaluation.py:236-253).  `model_bias` selects the explainer family's
    `teacherforce_forward`, as `TF_MODEL_BIAS` does in explainers/dropin.py.
    delete_ids (R, k): the positions to delete in place of the top-`kdel` relevant ones (`delete_tokens`; the random arm,
    evaluation.py:265-287) - `r_words` and `kdel` are then not read."""
    dev = engine.device
    t_host = [int(v) for v in torch.as_tensor(t_rows).tolist()]
    R = len(t_host)
    if R == 0:
        return torch.empty(0, device=dev)
    captions = _rows(engine, captions, R).to(torch.int64).contiguous()
    if max(t_host) + 1 >= captions.shape[1]:
        raise ValueError("word_ablation: a row needs t + 2 caption tokens (t up to {}, captions {})".format(max(t_host), tuple(captions.shape)))
    row2img = _rows(engine, row2img, R).to(torch.int64)
    if delete_ids is None:
        short, lens, _ = delete_topk_tokens(engine, captions, t_host, r_words, kdel)
    else:
        short, lens = delete_tokens(engine, captions, t_host, delete_ids)
    lens_host = lens.tolist() if delete_ids is not None else None
    targets = captions[torch.arange(R, device=dev), torch.tensor(t_host, dtype=torch.int64, device=dev) + 1]
    out = torch.empty(R, device=dev)
    for r0 in range(0, R, ROWS):
        r1 = min(R, r0 + ROWS)
        tmax = max(t_host[r0:r1])
        # the longest shortened prefix of the chunk
        Lc = tmax + 1 - min(int(kdel), tmax) if lens_host is None else max(lens_host[r0:r1])
        out[r0:r1] = _teacherforce_last(engine, _enc_rows(enc, row2img[r0:r1]), short[r0:r1, :Lc + 1].contiguous(), lens[r0:r1],
                                        targets[r0:r1], model_bias)
    return out


def trim_bad_endings(seq, bad_ending_ids):
    """`remove_bad_endings` (models/gridTDmodel.py:284-302) on ids: trailing ids of the set are dropped; a caption that would be left
    empty is kept as it was"""
    bad = set(int(b) for b in bad_ending_ids)
    out = list(seq)
    while out and out[-1] in bad:
        out.pop()
    return out if out else list(seq)


def image_ablation(engine, images, row2img, spatial, targets, start_id, end_id, special_ids, patch_size=8, num_delete_patches=20,
                   beam_size=3, max_cap_length=20, bad_ending_ids=(), model_bias=False):
    """Row r explains the word `targets[r]` of image row2img[r] with the saliency spatial[r] (H, W) (`evaluation.spatial_relevance(maps)`,
    or any other map: a random permutation, an expanded attention map).  Per row: `evaluation.block_image` -> mask * image -> `encode`
    -> `beam_search_batch` (the model's own defaults, models/gridTDmodel.py:400: beam 3, 20 steps) -> `sen_idx` (the sequence without
    `special_ids`, :475) without its bad endings -> the first occurrence of the target -> `[<start>] + sen_idx[:new_idx]` teacher-forced on
    the MASKED image's encoding -> the target's probability at the last step (evaluation.py:135-150).  In chunks of whole rows that keep a
    launch at or below 64 rows and `encode` at or below `ENC_IMAGES` images.  Returns (found (R,) bool, new_idx (R,) int64, -1 where the word is gone, new_prob (R,), NaN there,
    new captions: R lists of ids without <start>)."""
    dev = engine.device
    spatial = spatial.to(dev)
    R = spatial.shape[0]
    row2img = _rows(engine, row2img, R).to(torch.int64)
    tgt_host = [int(v) for v in torch.as_tensor(targets).tolist()]
    if len(tgt_host) != R:
        raise ValueError("image_ablation: {} targets for {} rows".format(len(tgt_host), R))
    images = images.to(dev, torch.float32)
    special = set(int(s) for s in special_ids)
    per = max(1, min(ROWS // int(beam_size), ENC_IMAGES))
    found, new_idx, caps_out = [], [], []
    prob = torch.full((R,), float("nan"), device=dev)
    for r0 in range(0, R, per):
        r1 = min(R, r0 + per)
        mask = evaluation.block_image(spatial[r0:r1], patch_size, num_delete_patches)
        enc = engine.encode(mask[:, None] * images[row2img[r0:r1]])
        seqs = beam_search_batch(engine, enc, beam_size, max_cap_length, start_id, end_id)
        hit, prefix = [], []
        for j, seq in enumerate(seqs):
            sen = trim_bad_endings([w for w in seq if w not in special], bad_ending_ids)
            caps_out.append(sen)
            k = sen.index(tgt_host[r0 + j]) if tgt_host[r0 + j] in sen else -1
            found.append(k >= 0)
            new_idx.append(k)
            if k >= 0:
                hit.append(j)
                prefix.append([int(start_id)] + sen[:k])
        if hit:
            L = max(len(p) for p in prefix)
            caps = torch.tensor([p + [0] * (L + 1 - len(p)) for p in prefix], dtype=torch.int64, device=dev)
            lens = torch.tensor([len(p) for p in prefix], dtype=torch.int32, device=dev)
            idx = torch.tensor(hit, dtype=torch.int64, device=dev)
            tg = torch.tensor([tgt_host[r0 + j] for j in hit], dtype=torch.int64, device=dev)
            prob[r0 + idx] = _teacherforce_last(engine, _enc_rows(enc, idx), caps, lens, tg, model_bias)
    return (torch.tensor(found, dtype=torch.bool, device=dev), torch.tensor(new_idx, dtype=torch.int64, device=dev), prob, caps_out)
