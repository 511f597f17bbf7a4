"""Host side of the diverse beam search.  The list-level restatement of the reference's loop (tests/dbs_restate.py) replays the scores
recorded from the reference's own runs (tests/golden/dbs.npz, written by make_golden_dbs.py) to the reference's sequences, and has the
two identities the algorithm promises; the ctypes mirror of `lrpx_dbs_batch` has the compiler's layout.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from conftest import GOLDEN
from lrp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbs_restate as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVENTS = ("partial", "passed_over", "g0_done_g1_selects", "fallback_after_g0_done", "differs_from_div0")


def golden_cases(small=None):
    """the cases of dbs.npz as dicts; small=True: those that carry their recorded scores (V = 37)"""
    with np.load(os.path.join(GOLDEN, "dbs.npz"), allow_pickle=False) as f:
        g = {k: f[k] for k in f.files}
    out = []
    for i in range(int(g["n_cases"])):
        c = {k[len(f"c{i}_"):]: v for k, v in g.items() if k.startswith(f"c{i}_")}
        c["model"] = str(c["model"])
        for k in ("V", "seed", "beam", "steps", "pad", "unk", "start", "end"):
            c[k] = int(c[k])
        c["div"], c["fc_scale"] = float(c["div"]), float(c["fc_scale"])
        c["wm"] = {'<pad>': c["pad"], '<unk>': c["unk"], '<start>': c["start"], '<end>': c["end"]}   # the special ids of the run's word map
        c["sen"], c["sen0"] = ([[int(w) for w in row if w >= 0] for row in c[k]] for k in ("sen", "sen0"))
        if small is None or small == ("logits" in c):
            out.append(c)
    return out


def sen_idx(seq, wm):
    """:391-392"""
    return [w for w in seq if w not in set(wm.values())]


def replay(c, log=None):
    """the restatement on the recorded scores of case c, in the order the reference called `predict_next_word`"""
    wm = c["wm"]
    it = iter(zip(c["logits"], c["rows"]))

    def step(t, g, seqs):
        lg, n = next(it)
        assert n == len(seqs)
        return torch.from_numpy(lg[:n].copy())
    seqs = R.diverse_beam_search(step, c["V"], c["beam"], c["steps"], wm['<start>'], c["end"], c["div"], log)
    assert next(it, None) is None
    return seqs, wm


def test_the_goldens_cover_every_path():
    """each event the kernel has a path for occurs in a stored case, and every stored selection rests on a gap of 1e-3"""
    cases = golden_cases()
    assert len(cases) >= 8 and len(golden_cases(small=True)) >= 4
    assert {c["model"] for c in cases} == {"grid", "bu", "aoa", "ada"} and {c["beam"] for c in cases} >= {2, 3}
    for j, e in enumerate(EVENTS):
        assert any(bool(c["events"][j]) for c in cases), e
    assert all(float(c["min_gap"]) >= 1e-3 for c in cases)
    assert all((c["sen"] != c["sen0"]) == bool(c["events"][4]) for c in cases)
    for model in ("grid", "bu", "aoa", "ada"):          # per model a case that tells its engine from another: no empty group, groups that
        assert any(c["model"] == model and all(c["sen"]) and len({tuple(s) for s in c["sen"]}) > 1 and c["sen"] != c["sen0"]      # differ,
                   for c in cases), model                                                     # and a result the penalty decided


def test_restatement_replays_the_recorded_scores_to_the_references_sequences():
    small = golden_cases(small=True)
    for c in small:
        log = {}
        seqs, wm = replay(c, log)
        assert [sen_idx(s, wm) for s in seqs] == c["sen"], (c["model"], c["end"])
        assert [bool(log[e]) for e in EVENTS[:4]] == [bool(x) for x in c["events"][:4]]
        assert log["min_gap"] >= float(c["min_gap"])


def _table_step(L, M=8):
    """scores that depend on a sequence's own length and last word, as a decoder's do - not on the loop step: a group that was passed
    over sees at the next step what it would have seen at this one"""
    return lambda t, g, seqs: torch.stack([L[len(s) - 1, s[-1] % M] for s in seqs])


@pytest.mark.parametrize("V", [37, 503])
def test_identities_of_the_restatement(V):
    """beam_size = 1 is the greedy beam; group 0 is the beam search at any diversity; at diversity 0 every group is.  A copy runs a
    step behind for every group that finished before it, so it equals the beam search unless max_cap_length cuts it short: here <end>
    cannot be chosen at positions 8 and later, so group 0 finishes by step 7 or never, and 7 + 3 < 12."""
    gen = torch.Generator().manual_seed(V)
    for trial in range(6):
        T, end = 12, 5
        L = torch.randn(T, 8, V, generator=gen) * 2.0
        L[:, :, end] += (-60.0 if trial % 2 else 2.0)
        L[8:, :, end] = -60.0
        for k in (1, 2, 3, 4):
            plain = R.beam_search(lambda t, seqs: _table_step(L)(t, 0, seqs), V, k, T, 1, end)
            assert R.diverse_beam_search(_table_step(L), V, k, T, 1, end, 0.0) == [plain] * k
            assert R.diverse_beam_search(_table_step(L), V, k, T, 1, end, 0.7)[0] == plain


def test_ctypes_mirror_of_the_dbs_state_has_the_compilers_layout(tmp_path):
    assert shutil.which("g++") is not None, "the layout check needs a host C++ compiler"
    fields = [n for n, _ in _lib.DbsBatch._fields_]
    src = tmp_path / "layout.cpp"
    body = "".join('    printf("%s %%zu\\n", offsetof(lrpx_dbs_batch, %s));\n' % (f, f) for f in fields)
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "lrpx.h"\nint main() {\n' + body +
                   '    printf("sizeof %zu\\n", sizeof(lrpx_dbs_batch));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for f in fields:
        assert int(got[f]) == getattr(_lib.DbsBatch, f).offset, f
    assert int(got["sizeof"]) == C.sizeof(_lib.DbsBatch)


def test_explainers_export_the_diverse_search():
    import lrp_amd.explainers as E
    from lrp_amd.explainers import beam
    assert E.diverse_beam_search_batch is beam.diverse_beam_search_batch and E.diverse_captions_batch is beam.diverse_captions_batch
    with pytest.raises(ValueError):
        E.diverse_beam_search_batch(None, {"B": 1}, 5, 10, 1, 2)
