#!/usr/bin/env python3
"""Golden vectors of the reference's `diverse_beam_search` (models/gridTDmodel.py:304-398 and :2061, models/aoamodel.py:305,
models/adaptiveattention.py:276): tests/golden/dbs.npz.  Run where the reference is, with make_golden.py's stubs and its PyTorch-1.4 `/`
(`beam_idx = top_words / vocab_size`, aoamodel.py:360, raises IndexError under today's true division):

    python tests/golden/make_golden_dbs.py

The reference returns sentences; a word map of unique tokens gives the ids back, so what is stored per group is `sen_idx` (:391-392):
the sequence without <start>, <end>, <unk>, <pad>.  <pad>, <unk> and the default <end> of a draw are ids its free run does not emit - a
run of <unk> would be stored as empty sequences, which any engine output made of special ids equals.  Random-init weights never emit a
fixed <end>: as in make_golden.py's gen_beam, <end> is declared to be a word the free run produces.  Every drawn case is run at its
`diversity_prob` and at 0, with every `predict_next_word` call's scores recorded; tests/dbs_restate.py replays the scores and labels the
run.  A case is KEPT when every selection rests on a gap of at least 1e-3 (make_golden_ablation.py's margin) between neighbouring kept
candidates and to the first rejected one - the engines' scores differ from the reference's by rounding, and a test must not rest on
that.  The script asserts that the restatement reproduces every kept run; that each event the kernel has a path for occurs in a kept
case; that per model a kept case has no empty group, groups that differ, and a result that differs from the run at diversity 0; and
that at least half of the drawn cases were kept.  The V = 37 cases store their recorded scores too (a few KB each): tests/test_dbs_host.py
replays them without the reference, tests/test_gpu_dbs.py feeds them to the kernel.

Stored: n_cases, and per case c<i>_: model (grid / bu / aoa / ada), V, seed, fc_scale (`weights.scale_fc`), beam, steps, the special ids
pad / unk / start / end, div, sen (G rows, -1 padded), sen0 (the same at diversity 0), events (the flags of EVENTS, in that order),
min_gap; small-V cases also logits (calls, beam, V; unused rows zero)
and rows (calls)."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_stubs, load_pkg, ref_vgg_patch, to_torch_sd  # noqa: E402

import dbs_restate as R  # noqa: E402

GAP = 1e-3
FC = 100.0       # weights.scale_fc: random-init scores are flat, their candidates 1e-5 apart
EVENTS = ("partial", "passed_over", "g0_done_g1_selects", "fallback_after_g0_done", "differs_from_div0")
H = 512
EVERY = tuple(range(1, 11))
LATE = tuple(range(2, 12))
# <end> ids drawn besides those positions, keyed by (model, V, seed, fc scale, beam).  A scan of all word ids of V = 37 models (three
# seeds, fc scales 30 and 100, beam 2 .. 4) found these runs in which a group falls back after group 0 finished: that needs group 0 to
# complete all its beams while a later group has completed none.
EXTRA_ENDS = {("ada", 37, 0, 30.0, 2): (15, 20), ("aoa", 37, 2, 30.0, 3): (4,), ("aoa", 37, 2, 30.0, 2): (26,)}


class Const(nn.Module):
    """stands in for a model's image encoder: the one image is encoded once, not once per run"""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x):
        return self.out


def make_state(tag, V, seed, fc_scale, weights):
    """the seeded state a case runs on - here and in the tests"""
    mk = {"grid": weights.make_gridtd_state, "bu": weights.make_gridtd_bu_state, "aoa": weights.make_aoa_state, "ada": weights.make_adaatt_state}[tag]
    return weights.scale_fc(mk(seed=seed, vocab_size=V), fc_scale)


def build(tag, V, seed, fc_scale, weights):
    """(model, the argument `diverse_beam_search` takes for the one seeded image)"""
    import models.adaptiveattention as ada
    import models.aoamodel as aoa
    import models.gridTDmodel as gtd
    if tag == "bu":
        m = gtd.GridTDModelBU(H, H, V, 'bu')
        m.load_state_dict(to_torch_sd(make_state(tag, V, seed, fc_scale, weights)))
        return m.eval(), torch.from_numpy(weights.make_bu_features(seed + 7, 1))
    m = {"grid": lambda: gtd.GridTDModel(H, H, V, 'vgg16'), "aoa": lambda: aoa.AOAModel(H, H, 8, V, 'vgg16'),
         "ada": lambda: ada.AdaptiveAttentionCaptioningModel(H, H, V, 'vgg16')}[tag]()
    m.load_state_dict(to_torch_sd(make_state(tag, V, seed, fc_scale, weights)))
    m.eval()
    img = torch.from_numpy(weights.make_images(seed + 7, 1))
    with torch.no_grad():
        m.img_encoder = Const(m.img_encoder(img))
    return m, img


def run(model, x, wm, beam, steps, div):
    """the reference's own run -> (`sen_idx` per group, the scores of every `predict_next_word` call)"""
    calls = []
    orig = model.predict_next_word

    def recording(*a, **k):
        out = orig(*a, **k)
        calls.append(out[0].detach().clone())
        return out
    orig_div = torch.Tensor.__truediv__

    def div14(a, b):
        if torch.is_tensor(a) and not a.is_floating_point() and isinstance(b, int):
            return torch.div(a, b, rounding_mode="floor")
        return orig_div(a, b)
    model.predict_next_word = recording
    torch.Tensor.__truediv__ = div14
    out, stdout = None, sys.stdout
    try:
        sys.stdout = open(os.devnull, "w")               # (the reference prints every sentence)
        out = model.diverse_beam_search(x, beam, wm, max_cap_length=steps, diversity_prob=div)
    finally:
        sys.stdout.close()
        sys.stdout = stdout
        torch.Tensor.__truediv__ = orig_div
        del model.predict_next_word
    return [[wm[w] for w in s.split(' ') if w] for s in out], calls


def replay(calls, V, beam, steps, wm, div, log=None):
    it = iter(calls)
    seqs = R.diverse_beam_search(lambda t, g, s: next(it), V, beam, steps, wm['<start>'], wm['<end>'], div, log)
    assert next(it, None) is None, "the restatement made fewer calls than the reference"
    drop = {wm[k] for k in ('<start>', '<end>', '<unk>', '<pad>')}
    return [[w for w in s if w not in drop] for s in seqs]


def pad(rows):
    n = max([len(r) for r in rows] + [1])
    return np.array([list(r) + [-1] * (n - len(r)) for r in rows], np.int64)


def word_map(V, pad_id, unk_id, end_id):
    """unique tokens for all V ids, the special ones where the draw puts them (<start> = V - 2 as in `weights.make_word_map`)"""
    special = {pad_id: '<pad>', unk_id: '<unk>', V - 2: '<start>', end_id: '<end>'}
    assert len(special) == 4
    return {special.get(i, f"w{i}"): i for i in range(V)}


def free_run(model, x, V, beam, steps, div):
    """A word map whose <pad>, <unk> and <end> are ids the free run does not emit (`sen_idx` drops them: a run of <unk> would be
    stored as empty sequences), and that run's raw sequences from the restatement's replay."""
    emitted = {V - 2}
    for _ in range(6):
        pad_id, unk_id, end_id = [i for i in range(V) if i not in emitted][:3]
        wm = word_map(V, pad_id, unk_id, end_id)
        _, calls = run(model, x, wm, beam, steps, div)
        it = iter(calls)
        raw = R.diverse_beam_search(lambda t, g, s: next(it), V, beam, steps, wm['<start>'], wm['<end>'], div)
        now = {w for s in raw for w in s}
        if not now & {pad_id, unk_id, end_id}:
            return wm, raw
        emitted |= now
    raise AssertionError("no word map whose special ids the free run leaves alone")


def main():
    install_stubs()
    weights = load_pkg()
    ref_vgg_patch()
    # (model, V, seed, fc scale, beam, steps, diversity, steps of group 0's free run whose word becomes <end>)
    draws = [("aoa", 11027, 0, FC, 3, 20, 0.5, (11, 12, 14)), ("aoa", 11027, 0, FC, 2, 14, 0.5, (5, 9)),
             ("grid", 9586, 0, FC, 3, 16, 0.5, LATE), ("grid", 9586, 1, FC, 2, 16, 0.5, LATE), ("ada", 9586, 0, FC, 3, 16, 0.8, (4, 8, 12)),
             ("bu", 9586, 0, FC, 3, 12, 0.5, LATE), ("bu", 9586, 1, FC, 2, 12, 0.5, LATE),
             ("grid", 37, 1, FC, 3, 14, 0.5, EVERY), ("aoa", 37, 0, FC, 3, 14, 0.5, EVERY), ("ada", 37, 0, FC, 4, 12, 0.8, EVERY),
             ("bu", 37, 1, FC, 3, 12, 0.5, EVERY), ("grid", 37, 0, FC, 2, 14, 2.0, EVERY), ("bu", 37, 0, FC, 2, 12, 2.0, EVERY),
             ("ada", 37, 0, 30.0, 2, 12, 0.5, ()), ("aoa", 37, 2, 30.0, 3, 12, 0.5, ()), ("aoa", 37, 2, 30.0, 2, 12, 0.5, ())]
    g, kept, drawn, seen = {}, 0, 0, {e: 0 for e in EVENTS}
    varied = {}
    for tag, V, seed, fc_scale, beam, steps0, div, positions in draws:
        model, x = build(tag, V, seed, fc_scale, weights)
        wm, raw = free_run(model, x, V, beam, steps0, div)
        ends = [raw[0][1 + p] for p in positions if 1 + p < len(raw[0])] + list(EXTRA_ENDS.get((tag, V, seed, fc_scale, beam), ()))
        todo = [(None, steps0)] + [(e, steps0) for e in dict.fromkeys(ends) if e not in (wm['<pad>'], wm['<unk>'], wm['<start>'])]
        while todo:
            end, steps = todo.pop(0)
            drawn += 1
            wme = wm if end is None else word_map(V, wm['<pad>'], wm['<unk>'], int(end))
            sen, calls = run(model, x, wme, beam, steps, div)
            sen0, calls0 = run(model, x, wme, beam, steps, 0.0)
            log, log0 = {}, {}
            again, again0 = replay(calls, V, beam, steps, wme, div, log), replay(calls0, V, beam, steps, wme, 0.0, log0)
            gap = min(log["min_gap"], log0["min_gap"])
            print(f"{tag} V={V} seed={seed} beam={beam} steps={steps} <end>={wme['<end>']}: gap {gap:.2e}", {e: log[e] for e in EVENTS[:4]},
                  "differs" if sen != sen0 else "same", sen if V == 37 else [len(s) for s in sen], "group 0 done at", log["g0_done_step"])
            # the same run cut right after group 0's last beam completed: the groups it passed over never select again
            if steps == steps0 and log["g0_done_step"] is not None and 1 <= log["g0_done_step"] < steps - 1:
                todo.append((end, log["g0_done_step"] + 1))
            if gap < GAP:
                continue
            assert again == sen and again0 == sen0, (tag, V, end, again, sen)
            log["differs_from_div0"] = sen != sen0
            varied[tag] = varied.get(tag, 0) + (all(sen) and len({tuple(s) for s in sen}) > 1 and sen != sen0)
            c = f"c{kept}_"
            g[c + "model"], g[c + "V"], g[c + "seed"], g[c + "beam"], g[c + "steps"] = np.array(tag), np.int64(V), np.int64(seed), np.int64(beam), np.int64(steps)
            g[c + "pad"], g[c + "unk"], g[c + "start"], g[c + "end"] = (np.int64(wme[k]) for k in ('<pad>', '<unk>', '<start>', '<end>'))
            g[c + "div"], g[c + "sen"], g[c + "sen0"] = np.float64(div), pad(sen), pad(sen0)
            g[c + "events"], g[c + "min_gap"], g[c + "fc_scale"] = np.array([bool(log[e]) for e in EVENTS]), np.float64(gap), np.float64(fc_scale)
            if V == 37:
                lg = np.zeros((len(calls), beam, V), np.float32)
                for i, cl in enumerate(calls):
                    lg[i, :cl.shape[0]] = cl.numpy()
                g[c + "logits"], g[c + "rows"] = lg, np.array([cl.shape[0] for cl in calls], np.int64)
            for e in EVENTS:
                seen[e] += bool(log[e])
            kept += 1
    g["n_cases"] = np.int64(kept)
    print(f"kept {kept} of {drawn} drawn cases; events:", seen, "; cases per model whose groups are non-empty, differ and differ from the run "
          "without penalty:", varied)
    assert 2 * kept >= drawn, "fewer than half of the drawn cases rest on a gap of 1e-3"
    assert all(seen.values()), f"an event occurs in no kept case: {seen}"
    assert all(varied.get(tag, 0) >= 1 for tag in ("grid", "bu", "aoa", "ada")), f"a model without a case that could tell its engine from another: {varied}"
    np.savez_compressed(os.path.join(HERE, "dbs.npz"), **g)


if __name__ == "__main__":
    main()
