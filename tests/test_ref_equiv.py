"""The reference-equivalent CPU mode (the cpu_baseline of bench.py) must give the oracle's numbers:
it replays the reference's op sequence (hooks + autograd, materialised epsilon rules, per-pixel loops)."""
import numpy as np
import pytest
import torch

import lrp_amd  # noqa: F401
from lrp_amd import weights
from conftest import rel_err
from oracle import lrp_oracle as O
from oracle import ref_equiv as RE


def test_ref_equiv_matches_oracle_and_accumulates():
    V = 211
    sd = O.state_to_torch(weights.make_gridtd_state(seed=2, vocab_size=V))
    img = torch.from_numpy(weights.make_images(3, 1))
    cap = weights.make_captions(4, 1, 2, V)[0]
    maps, rws, t_trace, t_words = RE.explain_words(sd, img, cap, [0, 1])
    w_maps, w_rws = O.gridtd_explain_caption(sd, img, cap, accumulate=True)
    for t in range(2):
        assert rel_err(maps[t], w_maps[t]) < 1e-5          # incl. the running-sum quirk of sample.grad
        assert np.abs(rws[t].numpy() - w_rws[t].numpy()).max() < 1e-5


def test_ref_equiv_against_the_reference_outputs_of_a_3_word_caption(golden_dir):
    """the CPU baseline that travels (oracle/ref_equiv.py) is a stand-in for the reference.  Its maps and r_words for a
    3-word caption against the reference's own `ExplainGridTDAttention.explain_caption` on the same state, image and caption
    (tests/golden/gridtd_T3.npz, written by make_golden.py: the running sums the reference returns, the last word's map in full, every
    word's map as a 4-strided subsample and as sum / max|R| / L2 over all pixels): the same numbers to 1e-5 incl. the running-sum quirk
    (tools/ref_timing.py --words 3 measured 4.2e-7 of the maps' maximum and 5.7e-7 on r_words).  The wall-time side of the stand-in
    (1.04x the reference's time at 20 words) needs the reference itself: profiles/r04_ref_equiv_vs_reference.json, by the same tool."""
    import os
    g = np.load(os.path.join(golden_dir, "gridtd_T3.npz"))
    T, V, seed = 3, int(g["V"]), int(g["seed"])
    sd = O.state_to_torch(weights.make_gridtd_state(seed=seed, vocab_size=V))
    img = torch.from_numpy(weights.make_images(seed, 1))
    cap = weights.make_captions(seed + 1, 1, T, V)[0]
    assert np.array_equal(cap, g["caption"])
    maps, rws, _, _ = RE.explain_words(sd, img, cap, list(range(T)))
    for t in range(T):
        m = maps[t].double()
        _, want_max, want_l2 = g[f"map_stats_{t}"]
        assert abs(m.abs().max().item() - want_max) < 1e-5 * want_max
        assert abs(m.pow(2).sum().sqrt().item() - want_l2) < 1e-5 * want_l2
        assert (m[..., ::4, ::4] - torch.from_numpy(g[f"map_sub4_{t}"]).double()).abs().max().item() < 1e-5 * want_max
        assert np.abs(rws[t].detach().numpy() - g[f"r_words_{t}"]).max() < 1e-5
    assert rel_err(maps[T - 1], torch.from_numpy(g[f"map_full_{T - 1}"])) < 1e-5
