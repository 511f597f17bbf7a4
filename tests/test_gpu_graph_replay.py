"""Captured steps (`explain_batch_graph` of both engines; explainers/engine_base.py: `_static_step`, `_CapturedGraph`): an eager
`explain_batch` captured once in a HIP graph and replayed from static buffers.  A replay issues the kernels of the eager step in the
same order on the same kind of buffers, as the recorded step of tests/test_gpu_replay.py does, so EVERY call - the capturing one and
every later replay, on new inputs and on the captured ones - must be BIT-IDENTICAL to `explain_batch` on the same engine and inputs.
No tolerance: the eager step is deterministic (tests/golden/explainer_bytes.json: equal digests over two processes).
tests/test_gpu_graph_primitives.py holds the pieces of a step to the same bar, one by one."""
import pytest
import torch

import lrp_amd  # noqa: F401

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _same(got, want, what):
    torch.cuda.synchronize()
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert not torch.isnan(g).any(), (what, i, "NaN in the replayed output")
        assert torch.equal(g, w), "%s, output %d: %d of %d elements differ from the eager step, largest difference %.3g" % (
            what, i, int((g != w).sum()), g.numel(), float((g.double() - w.double()).abs().max()))


def _clones(out):
    return tuple(t.clone() for t in out)          # (the returned tensors are the static outputs: the next call overwrites them)


def _bu_engine(force_f16=None):
    from lrp_amd import weights
    from lrp_amd.explainers.aoa import AOAEngine
    eng = AOAEngine(weights.make_aoa_state(seed=3, vocab_size=BU_V, feat_dim=2048, with_encoder=False))
    eng.force_f16 = force_f16
    return eng


BU_V, BU_B, BU_T = 503, 4, 5          # the shape of the defect as it was recorded (GRAPH_NOTE of tests/golden/make_golden_explainer_bytes.py)


def _bu_inputs(k):
    from lrp_amd import weights
    return (torch.from_numpy(weights.make_bu_features(10 + k, BU_B)).cuda(),
            torch.from_numpy(weights.make_captions(20 + k, BU_B, BU_T, BU_V)).cuda())


@pytest.mark.parametrize("force_f16", [True, False], ids=["split_products", "exact"])
def test_aoa_bottom_up_graph_replays_are_bit_identical(force_f16):
    """config 5's step (36 x 2048 region features): call 0 captures, calls 1 - 3 replay on new features and captions, call 4 on the
    inputs of call 0 again.  Split products: the amax rows of the trace and their atomics; exact: fp32 arithmetic throughout."""
    _need_gpu()
    eng = _bu_engine(force_f16)
    outs = []
    for k in range(5):
        feats, caps = _bu_inputs(k % 4)
        got = _clones(eng.explain_batch_graph(caps, 2, features=feats, predictions=True))
        _same(got, eng.explain_batch(caps, 2, features=feats, predictions=True), "call %d" % k)
        outs.append(got)
    _same(outs[4], outs[0], "call 4 against call 0 (the same inputs)")
    assert not torch.equal(outs[0][0], outs[1][0])          # (the inputs really differed)
    assert len(eng._graphs) == 1


def test_static_outputs_are_fully_rewritten():
    """nothing of a result is left over from the call before: NaN in every static output between two replays"""
    _need_gpu()
    eng = _bu_engine()
    for k in range(3):
        feats, caps = _bu_inputs(k)
        if k:
            (cap,) = eng._graphs.values()
            for t in cap.result:
                t.fill_(float("nan"))
        got = _clones(eng.explain_batch_graph(caps, 2, features=feats, predictions=True))
        _same(got, eng.explain_batch(caps, 2, features=feats, predictions=True), "call %d" % k)


def test_two_graphs_on_one_engine_and_a_replica():
    """heads 2 and 5: two captured graphs over the engine's persistent buffers, replayed alternately with an eager step on other inputs
    between every pair of replays; a replica captures its own while the parent's is replayed in between"""
    _need_gpu()
    eng = _bu_engine()
    other = _bu_inputs(7)
    for k in range(3):
        for head in (2, 5):
            feats, caps = _bu_inputs(k)
            got = _clones(eng.explain_batch_graph(caps, head, features=feats, predictions=True))
            eng.explain_batch(other[1], 7 - head, features=other[0], predictions=True)
            _same(got, eng.explain_batch(caps, head, features=feats, predictions=True), "head %d, call %d" % (head, k))
    assert len(eng._graphs) == 2
    rep = eng.replica()
    assert not hasattr(rep, "_graphs")
    for k in range(3):
        feats, caps = _bu_inputs(k + 1)
        got = _clones(rep.explain_batch_graph(caps, 2, features=feats, predictions=True))
        got_parent = _clones(eng.explain_batch_graph(caps, 5, features=feats, predictions=True))
        _same(got, eng.explain_batch(caps, 2, features=feats, predictions=True), "replica, call %d" % k)
        _same(got_parent, eng.explain_batch(caps, 5, features=feats, predictions=True), "parent beside the replica, call %d" % k)
    assert len(rep._graphs) == 1 and len(eng._graphs) == 2


def test_gridtd_vgg16_graph_replays_are_bit_identical():
    """the image path: VGG16 forward trace, gridTD decoder trace and relevance, VGG16 relevance chain, running sums"""
    _need_gpu()
    from lrp_amd import weights
    from lrp_amd.explainers.gridtd import GridTDEngine
    V, B, T = 307, 2, 3
    eng = GridTDEngine(weights.make_gridtd_state(seed=1, vocab_size=V))
    outs = []
    for k in range(4):          # call 0 captures, 1 and 2 replay on new inputs, 3 on the inputs of call 0
        img = torch.from_numpy(weights.make_images(30 + k % 3, B)).cuda()
        caps = torch.from_numpy(weights.make_captions(40 + k % 3, B, T, V)).cuda()
        got = _clones(eng.explain_batch_graph(img, caps, accumulate=True, predictions=True))
        assert len(got) == 3          # maps, r_words, predictions
        _same(got, eng.explain_batch(img, caps, accumulate=True, predictions=True), "call %d" % k)
        outs.append(got)
    _same(outs[3], outs[0], "call 3 against call 0 (the same inputs)")
    assert not torch.equal(outs[0][0], outs[1][0])
    # one image, as the drop-in calls it: a key, and a graph, of its own
    n = len(eng._graphs)
    first = _clones(eng.explain_batch_graph(img[:1], caps[:1]))
    second = _clones(eng.explain_batch_graph(img[:1], caps[:1]))
    assert len(eng._graphs) == n + 1
    _same(second, first, "B = 1, second replay against the first")
    _same(second, eng.explain_batch(img[:1], caps[:1]), "B = 1")


def test_aoa_vgg16_graph_replays_are_bit_identical():
    """the AoA image path (encoder in the state): B 1, T 2"""
    _need_gpu()
    from lrp_amd import weights
    from lrp_amd.explainers.aoa import AOAEngine
    V, B, T = 307, 1, 2
    eng = AOAEngine(weights.make_aoa_state(seed=2, vocab_size=V))
    for k in range(3):
        img = torch.from_numpy(weights.make_images(50 + k, B)).cuda()
        caps = torch.from_numpy(weights.make_captions(60 + k, B, T, V)).cuda()
        got = _clones(eng.explain_batch_graph(caps, 3, images=img, accumulate=True))
        _same(got, eng.explain_batch(caps, 3, images=img, accumulate=True), "call %d" % k)
