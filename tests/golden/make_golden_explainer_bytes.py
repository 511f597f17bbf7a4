#!/usr/bin/env python3
"""Output digests of the two caption explainers - `GridTDEngine` / `AOAEngine` (explainers/gridtd.py, explainers/aoa.py): the batch entry
points, the static-buffer drivers, the decode loops - and of the ten drop-in `Explain*` classes, recorded once from a checkout whose
bytes are to be kept.  tests/test_gpu_explainer_bytes.py runs the same group functions on the tree at hand and requires every sha256,
and the library call names of every recorded step, to be the recorded ones.  Writes tests/golden/explainer_bytes.json.

    python tests/golden/make_golden_explainer_bytes.py --commit <hash of the checkout this runs in>

Needs a GPU; run it from a checkout of that commit, never from a tree whose bytes are in question.  The groups run TWICE, each time in a
fresh process on freshly built engines (a captured HIP graph is made once per process, as in the suite): a digest that differs between
the two runs is not written - the generator stops and names it (the few-row fp32 dense kernel adds its K-split partials atomically; a
case that shows it has to move to a stable shape or mode, see the issue of the pull request that added this file).

Groups (one engine each, the smallest shapes that take every branch of the shared drivers):
  aoa_bu          bottom-up AoA, 36 x 2048 regions, V 503, B 4, T 5 (tests/test_gpu_replay.py's shapes): heads 2 and 5, lens None and
                  [5, 1, 3, 0]; explain_batch, explain_batch_replay (recording call + a replay on new inputs, call names kept);
                  sample_lrp, forwardlrp_context, beam_search of image 0
  aoa_bu_graph    the same engine and inputs: explain_batch_graph of heads 2 and 5, the capturing call (capture + first replay) and a
                  later replay on new inputs
  gridtd_resnet_mode0 / _mode1
                  the net and decoder of tests/test_gpu_gridtd_resnet.py (B 2, T 3, P 12, C 192, 45 x 51): explain_batch with lens None
                  and [3, 1], accumulate both ways, predictions and features returned; explain_stream at depth 2 over three batches;
                  greedy, sample_lrp, forwardlrp_context, beam_search
  gridtd_vgg      VGG16, V 307, B 2, T 2, lens None and [2, 1]: explain_batch (accumulate both ways), explain_batch_replay,
                  explain_batch_guided (gradcam both ways), explain_batch_gradient (cam both ways)
  gridtd_vgg_graph  the same engine and inputs: explain_batch_graph, the capturing call and a later replay on new inputs
  aoa_vgg         VGG16, head 3, same sizes: explain_batch, explain_batch_gradient of the four kinds
  dropin_gridtd / dropin_aoa
                  the five classes of each model on those VGG16 states: explain_caption of a tensor image without a caption (the beam
                  path) and with a three-word caption, explain_caption_wordt(1), explain_cnn twice (the accumulation),
                  teacherforce_forward, the attributes of the trace; AoA also explain_caption_words

GRAPH_NOTE says where the digests of the graph groups' later replays come from.  None of these entry points takes an output buffer, so
there is nothing to pre-fill.  Each group stores one digest of its inputs, so that a changed draw is told apart from a changed explainer."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from make_golden_resnet import bottleneck_net  # noqa: E402

JSON = os.path.join(HERE, "explainer_bytes.json")
SKIP = [1, 2, 3, 5, 8, 13]
GRAPH_NOTE = ("explain_batch_graph: the capturing call (capture + first replay, *_call0) was digested from the graph itself.  On the recorded "
              "commit every later replay of a captured graph differed from the eager step (bottom-up AoA, B 4, T 5: r_words off by up to 2.0) and "
              "from one process to the next, so the digests of the later replays (*_call1, new inputs) are those of the EAGER step on the same "
              "inputs: what a replay has to give (tests/test_gpu_graph_replay.py).  The generator takes them from `explain_batch`, the test from "
              "the replayed graph.")
RECORDING = False          # True while the generator records (run_all): the later replays of the graph groups come from the eager step


def sha(*items):
    """sha256 over tensors / arrays (their bytes) and lists of ints (as int64)"""
    h = hashlib.sha256()
    for t in items:
        if isinstance(t, (list, tuple)):
            t = np.asarray([int(v) for v in t], dtype=np.int64)
        elif isinstance(t, int):
            t = np.asarray([t], dtype=np.int64)
        h.update(torch.as_tensor(t).detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _put(res, name, out):
    """digest a result now (static outputs of a recording / graph are overwritten by the next call)"""
    torch.cuda.synchronize()
    assert name not in res, name
    if isinstance(out, (list, tuple)) and any(torch.is_tensor(v) for v in out):
        out = [sha(*out)]
    res[name] = sha(out) if not isinstance(out, list) or not out or not isinstance(out[0], str) else out[0]


def _calls(eng):
    """library call names of every recorded step of the engine, in the order the recordings were made"""
    return [[fn.__name__ for fn, _ in rec.calls] for rec in eng._recordings.values()]


def _lens_tag(lens):
    return "full" if lens is None else "lens" + "".join(str(n) for n in lens)


def _args(**kw):
    d = dict(embed_dim=512, hidden_dim=512, encoder='vgg16', weight='', save_path='/tmp', dataset='synthetic', height=224, width=224,
             num_head=8)
    d.update(kw)
    return types.SimpleNamespace(**d)


# ---- AoA, bottom-up ----------------------------------------------------------------------------------------------------------------------
def aoa_bu(graph=False):
    from lrp_amd import weights
    from lrp_amd.explainers.aoa import AOAEngine
    V, B, T = 503, 4, 5
    sd = weights.make_aoa_state(seed=3, vocab_size=V, feat_dim=2048, with_encoder=False)
    feats = [weights.make_bu_features(10 + k, B) for k in range(2)]
    caps = [weights.make_captions(20 + k, B, T, V) for k in range(2)]
    digest = sha(*feats, *caps, *[v for _, v in sorted(sd.items())])
    eng = AOAEngine(sd)
    feats, caps = [torch.from_numpy(f).cuda() for f in feats], [torch.from_numpy(c).cuda() for c in caps]
    res = {}
    for head in () if graph else (2, 5):
        for lens in (None, [5, 1, 3, 0]):
            _put(res, "explain_batch_h%d_%s" % (head, _lens_tag(lens)), eng.explain_batch(caps[0], head, features=feats[0], lens=lens, predictions=True))
        for k in range(2):              # call 0 records, call 1 replays on new inputs
            _put(res, "replay_h%d_call%d" % (head, k), eng.explain_batch_replay(caps[k], head, features=feats[k], predictions=True))
    if graph:
        for head in (2, 5):
            _put(res, "graph_h%d_call0" % head, eng.explain_batch_graph(caps[0], head, features=feats[0], predictions=True))
            later = eng.explain_batch if RECORDING else eng.explain_batch_graph
            _put(res, "graph_h%d_call1" % head, later(caps[1], head, features=feats[1], predictions=True))
        return digest, res, []
    wm = weights.make_word_map(V)
    enc = eng.encode(features=feats[0])
    _put(res, "sample_lrp", eng.sample_lrp(enc, T, wm['<start>'], wm['<end>'], SKIP))
    _put(res, "forwardlrp_context", eng.forwardlrp_context(enc, caps[0], [6, 2, 4, 3], SKIP)[:2])
    _put(res, "beam_search", eng.beam_search(eng.encode(features=feats[0][:1]), 3, T, wm['<start>'], wm['<end>']))
    return digest, res, _calls(eng)


# ---- gridTD on the small bottleneck ResNet -----------------------------------------------------------------------------------------------
def gridtd_resnet(mode):
    from lrp_amd import weights
    from lrp_amd.LRPtools import lrp_modules
    from lrp_amd.explainers.gridtd import GridTDEngine
    g = np.load(os.path.join(HERE, "gridtd_resnet.npz"))
    x = np.load(os.path.join(HERE, "resnet_engine.npz"))["x"]
    V = int(g["V"])
    net = bottleneck_net(np.random.RandomState(int(g["net_seed"])), lrp_modules.resAdd, 12, [1, 2, 1])
    sd = weights.make_gridtd_resnet_state(seed=int(g["decoder_seed"]), vocab_size=V, feat_dim=192, num_pixels=12)
    digest = sha(x, g["caption"], *[v for _, v in sorted(sd.items())], *[v for _, v in sorted(net.state_dict().items())])
    eng = GridTDEngine(sd, encoder=net.cuda(), encoder_conv_mode=mode)
    x, cap = torch.from_numpy(x).cuda(), torch.from_numpy(g["caption"]).cuda()
    res = {}
    for lens in (None, [3, 1]):
        for acc in (False, True):
            out = eng.explain_batch(x, cap, lens=lens, accumulate=acc, return_features=True, predictions=True)
            _put(res, "explain_batch_%s_acc%d" % (_lens_tag(lens), acc), out[:4])
    batches = [(x, cap), (x[1:], cap[1:]), (x.flip(0), cap.flip(0), [2, 3])]
    for acc in (False, True):
        for i, out in enumerate(eng.explain_stream(batches, depth=2, accumulate=acc)):
            _put(res, "explain_stream_acc%d_batch%d" % (acc, i), out)
    wm = weights.make_word_map(V)
    enc = eng.encode(x)
    _put(res, "greedy", eng.greedy(enc, 4, wm['<start>'], wm['<end>']))
    _put(res, "sample_lrp", eng.sample_lrp(enc, 3, wm['<start>'], wm['<end>'], SKIP))
    _put(res, "forwardlrp_context", eng.forwardlrp_context(enc, cap, [4, 2], SKIP)[:2])
    _put(res, "beam_search", eng.beam_search(eng.encode(x[:1]), 2, 3, wm['<start>'], wm['<end>']))
    return digest, res, []


# ---- the VGG16 engines -------------------------------------------------------------------------------------------------------------------
VGG_V, VGG_B, VGG_T = 307, 2, 2


def _vgg_inputs():
    from lrp_amd import weights
    imgs = [weights.make_images(30 + k, VGG_B) for k in range(2)]
    caps = [weights.make_captions(40 + k, VGG_B, VGG_T, VGG_V) for k in range(2)]
    return imgs, caps


def gridtd_vgg():
    from lrp_amd import weights
    from lrp_amd.explainers.gridtd import GridTDEngine
    sd = weights.make_gridtd_state(seed=1, vocab_size=VGG_V)
    imgs, caps = _vgg_inputs()
    digest = sha(*imgs, *caps, *[v for _, v in sorted(sd.items())])
    eng = GridTDEngine(sd)
    imgs, caps = [torch.from_numpy(f).cuda() for f in imgs], [torch.from_numpy(c).cuda() for c in caps]
    res = {}
    for lens in (None, [2, 1]):
        tag = _lens_tag(lens)
        for acc in (False, True):
            _put(res, "explain_batch_%s_acc%d" % (tag, acc), eng.explain_batch(imgs[0], caps[0], lens=lens, accumulate=acc, predictions=True))
        for flag in (False, True):
            _put(res, "guided_%s_gradcam%d" % (tag, flag), eng.explain_batch_guided(imgs[0], caps[0], lens=lens, gradcam=flag, return_features=True)[:3])
            _put(res, "gradient_%s_cam%d" % (tag, flag), eng.explain_batch_gradient(imgs[0], caps[0], lens=lens, cam=flag, return_features=True)[:3])
    for k in range(2):
        _put(res, "replay_call%d" % k, eng.explain_batch_replay(imgs[k], caps[k], accumulate=True, predictions=True))
    return digest, res, _calls(eng)


def gridtd_vgg_graph():
    from lrp_amd import weights
    from lrp_amd.explainers.gridtd import GridTDEngine
    sd = weights.make_gridtd_state(seed=1, vocab_size=VGG_V)
    imgs, caps = _vgg_inputs()
    digest = sha(*imgs, *caps, *[v for _, v in sorted(sd.items())])
    eng = GridTDEngine(sd)
    imgs, caps = [torch.from_numpy(f).cuda() for f in imgs], [torch.from_numpy(c).cuda() for c in caps]
    res = {}
    _put(res, "graph_call0", eng.explain_batch_graph(imgs[0], caps[0], accumulate=True, predictions=True))
    later = eng.explain_batch if RECORDING else eng.explain_batch_graph
    _put(res, "graph_call1", later(imgs[1], caps[1], accumulate=True, predictions=True))
    return digest, res, []


def aoa_vgg():
    from lrp_amd import weights
    from lrp_amd.explainers.aoa import AOAEngine
    sd = weights.make_aoa_state(seed=2, vocab_size=VGG_V)
    imgs, caps = _vgg_inputs()
    digest = sha(imgs[0], caps[0], *[v for _, v in sorted(sd.items())])
    eng = AOAEngine(sd)
    img, cap = torch.from_numpy(imgs[0]).cuda(), torch.from_numpy(caps[0]).cuda()
    res = {}
    for lens in (None, [2, 1]):
        tag = _lens_tag(lens)
        for acc in (False, True):
            out = eng.explain_batch(cap, 3, images=img, lens=lens, accumulate=acc, return_features=True, predictions=True)
            _put(res, "explain_batch_%s_acc%d" % (tag, acc), out[:3])
        for kind in ("gradient", "guided", "gradcam", "guided_gradcam"):
            _put(res, "%s_%s" % (kind, tag), eng.explain_batch_gradient(cap, 3, img, kind=kind, lens=lens, return_features=True)[:3])
    return digest, res, []


# ---- the drop-in classes -----------------------------------------------------------------------------------------------------------------
GRIDTD_CLASSES = ("ExplainGridTDAttention", "ExplainiGridTDGuidedGradient", "ExplainGridTDGuidedGradCam", "ExplainGridTDGradient",
                  "ExplainGridTDGradCam")
AOA_CLASSES = ("ExplainAOAAttention", "ExplainAOAGradient", "ExplainAOAGuidedGradient", "ExplainAOAGuidedGradCam", "ExplainAOAGradCam")


def _dropin(module, classes, sd, head):
    from lrp_amd import weights
    from lrp_amd.explainers import engine_cache
    engine_cache.clear()
    wm = weights.make_word_map(VGG_V)
    state = {k: torch.from_numpy(v) for k, v in sd.items()}
    img = torch.from_numpy(weights.make_images(31, 1))
    cap3 = [wm['<start>']] + [int(c) for c in weights.make_captions(12, 1, 3, VGG_V)[0][1:]]
    digest = sha(img, cap3, *[v for _, v in sorted(sd.items())])
    h = () if head is None else (head,)
    res = {}
    for name in classes:
        ex = getattr(module, name)(_args(), wm, model=state)
        maps, words = ex.explain_caption(img, *h)                                  # no caption: the explainer's own beam search
        _put(res, name + "/beam_caption", [ex.caption_length] + list(ex.beam_caption_encode))
        _put(res, name + "/explain_caption_beam", [torch.tensor(len(maps))] + list(maps) + list(words))
        maps, words = ex.explain_caption(img, *h, caption_encode=cap3)
        assert len(maps) == 3 and ex.caption_length == 3 and ex.num_pixels == 196
        _put(res, name + "/explain_caption", list(maps) + list(words))
        attrs = [ex.img, ex.predictions, ex.alphas, ex.image_features] + ([ex.betas] if head is None else [])
        _put(res, name + "/attributes", attrs)
        r, rw = ex.explain_caption_wordt(1, *h)
        _put(res, name + "/explain_caption_wordt", (r, rw))
        _put(res, name + "/explain_cnn_1", ex.explain_cnn(r))
        _put(res, name + "/explain_cnn_2", ex.explain_cnn(r))
        _put(res, name + "/teacherforce_forward", ex.teacherforce_forward(img, cap3))
        if head is not None:
            _put(res, name + "/explain_caption_words", ex.explain_caption_words(img, caption_encode=cap3))
    engine_cache.clear()
    return digest, res, []


def dropin_gridtd():
    from lrp_amd import weights
    from lrp_amd.explainers import gridtd
    return _dropin(gridtd, GRIDTD_CLASSES, weights.make_gridtd_state(seed=1, vocab_size=VGG_V), None)


def dropin_aoa():
    from lrp_amd import weights
    from lrp_amd.explainers import aoa
    return _dropin(aoa, AOA_CLASSES, weights.make_aoa_state(seed=2, vocab_size=VGG_V), 3)


# name -> f() = (digest of the inputs, {case: digest of the output}, [library call names of each recorded step]); the test runs these
GROUPS = {"aoa_bu": aoa_bu, "gridtd_resnet_mode0": lambda: gridtd_resnet(0), "gridtd_resnet_mode1": lambda: gridtd_resnet(1),
          "gridtd_vgg": gridtd_vgg, "aoa_vgg": aoa_vgg, "dropin_gridtd": dropin_gridtd, "dropin_aoa": dropin_aoa,
          "aoa_bu_graph": lambda: aoa_bu(graph=True), "gridtd_vgg_graph": gridtd_vgg_graph}          # (a HIP graph is captured once per process: groups of their own)


def run_all():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lrp_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_explainer_bytes: needs a GPU")
    global RECORDING
    RECORDING = True
    cases = {}
    for name, fn in GROUPS.items():
        digest, res, calls = fn()
        cases[name] = {"inputs": digest, "outputs": res, "recorded_calls": calls}
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit of the checkout (library and Python tree) this runs in")
    ap.add_argument("--out", default=JSON)
    ap.add_argument("--one-run", help="(internal) run the groups once in this process and write their digests to this file")
    a = ap.parse_args()
    if a.one_run:
        with open(a.one_run, "w") as f:
            json.dump(run_all(), f)
        return
    if not a.commit:
        ap.error("--commit is required")
    runs = []
    for k in range(2):          # two fresh processes, one after the other: this one never opens the GPU
        tmp = "%s.run%d" % (a.out, k)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--one-run", tmp], check=True)
        with open(tmp) as f:
            runs.append(json.load(f))
        os.remove(tmp)
    unstable = ["%s/%s" % (g, n) for g in runs[0] for n in runs[0][g]["outputs"] if runs[0][g]["outputs"][n] != runs[1][g]["outputs"].get(n)]
    unstable += [g + "/recorded_calls" for g in runs[0] if runs[0][g]["recorded_calls"] != runs[1][g]["recorded_calls"]]
    if unstable or sorted(runs[0]) != sorted(runs[1]):
        raise SystemExit("not written: %d outputs differ between two runs of this checkout: %s" % (len(unstable), ", ".join(unstable)))
    g = {"recorded_from_commit": a.commit, "compare": "sha256 of every output; every case was bit-stable over two runs in fresh processes",
         "graph_note": GRAPH_NOTE,
         "cases": runs[0]}
    with open(a.out, "w") as f:
        json.dump(g, f, indent=0, sort_keys=True)
        f.write("\n")
    print(os.path.basename(a.out) + ":", os.path.getsize(a.out), "bytes;", len(runs[0]), "groups,",
          sum(len(c["outputs"]) for c in runs[0].values()), "digests, all equal over two runs")


if __name__ == "__main__":
    main()
