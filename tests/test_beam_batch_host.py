"""Host side of the batched beam search and the ablation passes: the ctypes mirror of `lrpx_beam_batch` has the layout the C compiler
gives the header's struct, and the id-level `remove_bad_endings`.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import lrp_amd  # noqa: F401
from lrp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [n for n, _ in _lib.BeamBatch._fields_]


def test_ctypes_mirror_of_the_beam_state_has_the_compilers_layout(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler on this machine")
    src = tmp_path / "layout.cpp"
    body = "".join('    printf("%s %%zu\\n", offsetof(lrpx_beam_batch, %s));\n' % (f, f) for f in FIELDS)
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "lrpx.h"\nint main() {\n' + body +
                   '    printf("sizeof %zu\\n", sizeof(lrpx_beam_batch));\n    printf("limit %d\\n", LRPX_BEAM_MAX_STEPS);\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for f in FIELDS:
        assert int(got[f]) == getattr(_lib.BeamBatch, f).offset, f
    assert int(got["sizeof"]) == C.sizeof(_lib.BeamBatch)
    assert int(got["limit"]) == 1024


def test_trim_bad_endings_on_ids():
    """`remove_bad_endings` (models/gridTDmodel.py:284-302): trailing bad words go; a caption of bad words alone is kept as it was"""
    from lrp_amd.explainers.ablation import trim_bad_endings
    assert trim_bad_endings([7, 8, 9, 9], {9}) == [7, 8]
    assert trim_bad_endings([7, 9, 8], {9}) == [7, 9, 8]
    assert trim_bad_endings([9, 9], {9}) == [9, 9]
    assert trim_bad_endings([], {9}) == [] and trim_bad_endings([7], ()) == [7]


def test_explainers_export_the_ablation_passes():
    import lrp_amd.explainers as E
    from lrp_amd.explainers import beam
    assert E.beam_search_batch is beam.beam_search_batch and E.caption_batch is beam.caption_batch
    assert E.image_ablation is E.ablation.image_ablation and E.word_ablation is E.ablation.word_ablation and E.word_prob is E.ablation.word_prob
