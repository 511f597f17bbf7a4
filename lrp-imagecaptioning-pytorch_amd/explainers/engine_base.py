"""What `GridTDEngine` (explainers/gridtd.py) and `AOAEngine` (explainers/aoa.py) share: the choice of the encoder (`_init_encoder`: VGG16,
a bottleneck ResNet as a module or from its state-dict keys, or none), the fc scores, the index tables, replicas, the
decode loops of the reference's models, the static-buffer drivers (HIP graph / recorded step), the stream pipeline, and the tail of
every batch entry point.  Host logic only: it sequences the library calls of the engine's own `_step` / `relevance` / ... in the order
the two engines each used to spell out.

An engine provides: `device, sd, V, H, C, p_fc_fwd, p_fc_fwd_h, p_proj_rel, p_proj_rel_h, p_proj_rel_6, dense_bf16x6, force_f16`, the
encoder as `cnn` (None: region features only), `vgg` (the same object when it is VGG16, else None) and `resnet` (all three set by
`_init_encoder`), and the hooks
`_decode_trace`, `_decode_step`, `_reweight`, `_BEAM_STATE`."""
import copy

import numpy as np
import torch

from .. import _lib, ops
from .._lib import EPI_PLAIN, EPI_REL, check, ptr, stream_ptr

VGG_PREFIX = "img_encoder.encoder."


def _t(v, dev):
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(v)
    return v.detach().to(device=dev, dtype=torch.float32).contiguous()


def resnet_encoder_keys(state):
    """does the state dict hold a bottleneck ResNet under `img_encoder.encoder.` (key names of models/resnet.py) rather than VGG16's
    numbered `features` layers?"""
    return VGG_PREFIX + "conv1.weight" in state


_LRP_PARAM_KEYS = ("alpha", "beta", "ignore_bias")      # the reference's own names (lrp_wrapper.add_lrp(model, lrp_params))
_OWN = object()                                         # `_maps_stage`: read the engine's own `lrp_params`


def _lrp_rule(where, lrp_params):
    """`lrp_params` of an engine or a drop-in explainer -> None (the preset: None, or alpha 1 with beta 0) or (alpha, beta) of the
    general Conv2d rule.  ValueError, named after `where`, for anything but a dict, unknown keys, non-finite or non-numeric values and
    ignore_bias=False (the batched paths run the rule without bias).  Host logic: nothing touches the device."""
    if lrp_params is None:
        return None
    if not isinstance(lrp_params, dict):
        raise ValueError("{}: lrp_params must be None or a dict with the keys {}, got {!r}".format(where, _LRP_PARAM_KEYS, lrp_params))
    unknown = sorted(str(k) for k in lrp_params if k not in _LRP_PARAM_KEYS)
    if unknown:
        raise ValueError("{}: lrp_params has unknown keys {} (known: {})".format(where, unknown, _LRP_PARAM_KEYS))
    vals = []
    for k, default in (("alpha", 1.), ("beta", 0.)):
        v = lrp_params.get(k, default)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(float(v)):
            raise ValueError("{}: lrp_params[{!r}] must be a finite number, got {!r}".format(where, k, v))
        vals.append(float(v))
    if not lrp_params.get("ignore_bias", True):
        raise ValueError("{}: lrp_params['ignore_bias'] = False is not built on the batched paths (the rule runs without bias)".format(where))
    return None if vals == [1., 0.] else (vals[0], vals[1])


class _CapturedGraph(object):
    """a step captured in a HIP graph, with the surface of `_lib.Recording`: `result` (static outputs) and `replay()`"""

    def __init__(self, step, inputs):
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.result = step(*inputs)
        self.inputs = inputs

    def replay(self):
        self.graph.replay()
        return self.result


class EngineBase(object):
    _BEAM_STATE = ()                  # trace tensors (B, T+1, H) a beam search reorders with its beams
    _ENCODER_CONV_MODES = (0, 1)

    # ---- the encoder ---------------------------------------------------------------------------------------------------------------------
    def _init_encoder(self, state, device, encoder, encoder_conv_mode, need_encoder=True):
        """The head of both engines' constructors: the encoder (models/gridTDmodel.py:23-37, models/aoamodel.py:31-51) as `self.cnn` -
        `ops.Vgg16` built from the VGG16 keys under `img_encoder.encoder.` (`self.vgg` is then the same object), or `ops.ResNetEncoder`:
        from `encoder=`, an nn.Module on the GPU that `ops.match_bottleneck_resnet` accepts, or from a state dict whose encoder keys are
        those of models/resnet.py (`ops.bottleneck_resnet_from_state`).  A mode or a net the ResNet engine does not run is refused by
        host logic, before any device work.  need_encoder=False: a state without encoder keys gives `cnn = None` (region features
        only).  Sets `device, encoder_conv_mode, cnn, vgg, resnet`; returns the other tensors of `state` on the device."""
        name = type(self).__name__
        if isinstance(encoder_conv_mode, bool) or encoder_conv_mode not in self._ENCODER_CONV_MODES:
            raise ValueError("{}: encoder_conv_mode {!r}: the ResNet encoder engine has modes 0 (fp32 MFMA) and 1 (exact bf16 "
                             "split)".format(name, encoder_conv_mode))
        self.encoder_conv_mode = encoder_conv_mode
        from_state = encoder is None and resnet_encoder_keys(state)
        if encoder is not None:
            ops.match_bottleneck_resnet(encoder)          # host logic: a net the engine does not run is refused before any device work
            tensors = list(encoder.parameters()) + list(encoder.buffers())
            if not tensors or any(t.device.type != "cuda" for t in tensors):
                raise ValueError("ResNetEncoder: the model must live on the GPU (no CPU path)")
        elif from_state:
            encoder = ops.bottleneck_resnet_from_state(state, VGG_PREFIX)
        _lib.load()   # fail loudly without the HIP library
        if not torch.cuda.is_available():
            raise _lib.LrpxError("the LRP hot path needs an MI355X; there is no CPU fallback")
        dev = torch.device(device)
        self.device = dev
        sd = {k: _t(v, dev) for k, v in state.items() if not k.startswith(VGG_PREFIX)}
        self.vgg = None
        if encoder is not None:
            self.cnn = ops.ResNetEncoder(encoder.to(dev) if from_state else encoder, conv_mode=encoder_conv_mode)
        else:
            names = [k for k in state if k.startswith(VGG_PREFIX) and k.endswith(".weight")]
            if names or need_encoder:
                self.vgg = ops.Vgg16([_t(state[k], dev) for k in names],
                                     [_t(state[k.replace(".weight", ".bias")], dev) for k in names])
            self.cnn = self.vgg
        self.resnet = encoder is not None
        self.lrp_params = None          # the Conv2d rule of the encoder stage (`_maps_stage`); None: the preset, alpha 1 beta 0
        return sd

    def _maps_stage(self, entry, lrp_params=_OWN):
        """The encoder stage of `entry` under `self.lrp_params` ({"alpha": .., "beta": ..}; a drop-in explainer passes its own value, the
        engine may be shared): validated here, at the top of the entry point and before any device work (`_lrp_rule`).  Returns
        `maps_of(feat, row2img)`: `self.cnn.relevance` - today's call - for None or alpha 1 / beta 0; else the encoder's
        `relevance_alpha_beta` (a ResNet encoder: in the engine's mode; VGG16: in the context's resolved conv mode, 0 or 1 - the split
        modes 2 / 3 have no alpha-beta chain, ValueError).  The decoder is not touched: the reference applies alpha / beta to Conv2d only.
        Without an encoder any value but None is a ValueError."""
        where = "{}.{}".format(type(self).__name__, entry)
        params = getattr(self, "lrp_params", None) if lrp_params is _OWN else lrp_params
        rule = _lrp_rule(where, params)
        if self.cnn is None:
            if params is not None:
                raise ValueError("{}: lrp_params is the encoder's Conv2d rule and this engine has no encoder".format(where))
            return None
        if rule is None:
            return self.cnn.relevance
        alpha, beta = rule
        if self.resnet:
            return lambda feat, row2img: self.cnn.relevance_alpha_beta(feat, row2img, alpha, beta)
        o, cm, ff = _lib.VggOpts(), _lib.C.c_int(0), _lib.C.c_int(0)
        o.conv_mode = -1 if self.vgg.conv_mode is None else int(self.vgg.conv_mode)
        o.forward_f16 = -1 if self.vgg.forward_f16 is None else int(self.vgg.forward_f16)
        check(_lib.load().lrpx_vgg16_resolve_opts(_lib.C.byref(o), _lib.C.byref(cm), _lib.C.byref(ff)))      # (host logic: no launch)
        mode = cm.value
        if mode not in (0, 1):
            raise ValueError("{}: the alpha-beta rule runs in conv modes 0 and 1, the encoder context is in mode {}".format(where, mode))
        return lambda feat, row2img: self.vgg.relevance_alpha_beta(feat, row2img, alpha, beta, conv_mode=mode)

    def _features_stage(self, entry):
        """an entry point on region features: there is no encoder stage, so `lrp_params` must be None (ValueError otherwise)"""
        if getattr(self, "lrp_params", None) is not None:
            raise ValueError("{}.{}: lrp_params is the encoder's Conv2d rule and features have no encoder stage".format(type(self).__name__, entry))

    def _preset_only(self, entry, why):
        """refuse `entry` under a Conv2d rule other than the preset (after validating `lrp_params`)"""
        where = "{}.{}".format(type(self).__name__, entry)
        params = getattr(self, "lrp_params", None)
        if params is None:
            return
        if self.cnn is None:
            raise ValueError("{}: lrp_params is the encoder's Conv2d rule and this engine has no encoder".format(where))
        if _lrp_rule(where, params) is not None:
            raise NotImplementedError("{}: not built under lrp_params = {!r} - {}".format(where, params, why))

    _NO_STATIC_AB = "the per-trace coefficients of the alpha-beta chain are made lazily: the step is not recordable"
    _NO_GRAD_AB = "alpha / beta belong to the LRP Conv2d rule; the gradient family has none"

    def _refuse_resnet(self, entry, missing):
        if self.resnet:
            raise NotImplementedError("{}.{}: not built for a ResNet encoder - {}".format(type(self).__name__, entry, missing))

    _NO_GRAPH = "the ResNet engine's trace has not been captured in a HIP graph (the recording is missing)"
    _NO_RECORDING = ("the recording of the ResNet engine's step (_lib.Recording has only been built and checked around the VGG16 chain's "
                    "calls) is missing")

    # ---- hooks -------------------------------------------------------------------------------------------------------------------------
    def _decode_trace(self, enc, B, T, lrp=False):
        """a zeroed trace for T decoding steps of B rows; lrp=True: for the loops whose steps are re-weighted (`_reweight`)"""
        raise NotImplementedError

    def _decode_step(self, tr, enc, t, toks):
        """decoder step t of the model's own forward (correct LSTM bias) for all rows; column t of `toks` is its input"""
        raise NotImplementedError

    def _reweight(self, tr, t, pred, skip, hcw, log_softmax):
        """`get_lrp_weight_step`: the fc input of step t re-weighted by the relevance of the arg-max word of `pred` -> hcw (B,H)"""
        raise NotImplementedError

    # ---- scores, index tables, arithmetic, replicas -----------------------------------------------------------------------------------
    def logits(self, hc_rows, fast=False, amax=None):
        """fc scores (gridTD: fc(context_hat + h2), models/gridTDmodel.py:990) for R rows -> (R,V).  fast=True (the (T,V) block a trace
        keeps, not the decisions of a decoding loop): split products on the fp16 matrix cores (csrc/dense_f16x3.hip, fp32-grade: <= 2e-7
        of a row's maximum); `amax`: the rows' maxima where the kernel that wrote them recorded them."""
        R = hc_rows.shape[0]
        out = torch.empty(R, self.V, device=self.device)
        if fast and R >= 128 and self.p_fc_fwd_h is not None and self._f16():
            hc_rows = hc_rows.contiguous()
            ops.conv_mfma(hc_rows, self.p_fc_fwd_h, R, 0, self.H, -(-self.V // 32) * 32, 1, EPI_PLAIN, pix_per_map=1, oc_split=self.V,
                          bias=self.sd["fc.bias"], out0=out, f16x3=1, in_amax=amax if amax is not None else ops.amax_maps(hc_rows, R))
            return out
        ops.conv_mfma(hc_rows, self.p_fc_fwd, R, 0, self.H, -(-self.V // 32) * 32, 1, EPI_PLAIN, pix_per_map=1,
                      oc_split=self.V, bias=self.sd["fc.bias"], out0=out)
        return out

    def _row_index(self, B, T):
        """(idx (T, B*T): row of word t - s of the same image, clamped; row -> image; row -> row) as int32 device tables, cached"""
        key = (B, T)
        if key not in self._idx_cache:
            b = torch.arange(B, device=self.device).view(B, 1)
            t = torch.arange(T, device=self.device).view(1, T)
            s = torch.arange(T, device=self.device).view(T, 1, 1)
            idx = (b * T + (t - s).clamp(min=0)).to(torch.int32).reshape(T, B * T).contiguous()
            row2img = (b + 0 * t).to(torch.int32).reshape(B * T).contiguous()
            rowid = torch.arange(B * T, device=self.device, dtype=torch.int32)
            self._idx_cache[key] = (idx, row2img, rowid)
        return self._idx_cache[key]

    def _conv_mode(self):
        """the encoder's own conv mode: a ResNet engine's `encoder_conv_mode`, `vgg.conv_mode`, None without an encoder"""
        if self.resnet:
            return self.encoder_conv_mode
        return self.vgg.conv_mode if self.vgg is not None else None

    def _f16(self):
        """the decoder GEMMs on the fp16 split products?  (ops.decoder_f16: with conv modes 2 / 3 only - the engine's own `vgg.conv_mode` or
        the process default; `force_f16` overrides per engine).  With a ResNet encoder the mode is the engine's `encoder_conv_mode`
        (0 / 1): never, whatever `lrpx_set_conv_mode` says."""
        if self.force_f16 is not None:
            return bool(self.force_f16)
        return ops.decoder_f16(self._conv_mode())

    def replica(self):
        """A second execution context over the SAME weights (device tensors and packed blobs are shared): own encoder trace / workspace
        buffers, so that several batches can be in flight on separate HIP streams."""
        r = copy.copy(self)
        if self.cnn is not None:
            r.cnn = self.cnn.replica()
            r.vgg = None if self.resnet else r.cnn
        r._idx_cache = {}
        for k in ("_graphs", "_replicas", "_streams", "_recordings"):     # a replica never shares another engine's streams / buffer sets
            r.__dict__.pop(k, None)
        return r

    # ---- decode loops -------------------------------------------------------------------------------------------------------------------
    def beam_search(self, enc, beam_size, max_cap_length, start_id, end_id):
        """The model's `beam_search` (models/gridTDmodel.py:400-478; models/aoamodel.py: the same algorithm on the AoA step) for ONE image
        (enc of a single image, as the reference asserts :411): returns the chosen token sequence incl. <start> (`seq`, :469-472)."""
        from .beam import run_beam_search
        assert enc["B"] == 1, "beam search captions one image (models/gridTDmodel.py:411)"
        nb = int(beam_size)
        encb = {k: (v.expand(nb, *v.shape[1:]).contiguous() if torch.is_tensor(v) else v) for k, v in enc.items()}
        encb["B"] = nb
        T = int(max_cap_length)
        tr = self._decode_trace(encb, nb, T)
        toks = torch.zeros(nb, T + 1, dtype=torch.int64, device=self.device)

        def step(t, prev):
            toks[:, t] = prev
            self._decode_step(tr, encb, t, toks)

        def reorder(t, src):
            sel = torch.tensor(src, dtype=torch.int64, device=self.device)
            for k in self._BEAM_STATE:
                tr[k][:len(src), t + 1] = tr[k][sel, t + 1]

        return run_beam_search(step, lambda t: self.logits(tr["hc"][:, t].contiguous()), reorder, self.V, nb, T,
                               start_id, end_id, self.device)

    def _skip_mask(self, skip_ids):
        """(V,) uint8: 1 for the ids exempt from the re-weighting (the reference's STOP_WORDS and special tokens)"""
        skip = torch.zeros(self.V, dtype=torch.uint8, device=self.device)
        skip[torch.as_tensor(sorted(int(i) for i in skip_ids), dtype=torch.int64, device=self.device)] = 1
        return skip

    def _lrp_step(self, tr, enc, t, toks, skip, hcw, log_softmax):
        """step t, its scores, and the scores recomputed from the re-weighted fc input"""
        self._decode_step(tr, enc, t, toks)
        pred = self.logits(tr["hc"][:, t].contiguous())
        self._reweight(tr, t, pred, skip, hcw, log_softmax)
        return pred, self.logits(hcw)

    def sample_lrp(self, enc, max_length, start_id, end_id, skip_ids):
        """The model's `sample_lrp`, greedy (models/gridTDmodel.py:631-702, models/aoamodel.py:679-745): LRP-inference decoding.  Every
        step's logits are recomputed from the fc input re-weighted by the predicted word's relevance (`get_lrp_weight_step`, :548-577 /
        :597-626 - the AoA model hands it the log-softmax of the scores, :721-723) before the next word is taken.  `skip_ids`: ids
        exempt from the re-weighting.  Returns (seq int64 (B,max_length), seq_logprobs float32 (B,max_length)); like the reference,
        tokens after <end> are 0 and nothing is written once every sequence has finished (:699-700 / :742-744)."""
        lib = _lib.load()
        B, T, dev = enc["B"], max_length, self.device
        skip = self._skip_mask(skip_ids)
        toks = torch.zeros(B, T + 1, dtype=torch.int64, device=dev)
        toks[:, 0] = start_id
        lps = torch.zeros(B, T, dtype=torch.float32, device=dev)
        tr = self._decode_trace(enc, B, T, lrp=True)
        hcw = torch.empty(B, self.H, device=dev)
        nxt = torch.empty(B, dtype=torch.int64, device=dev)
        lp = torch.empty(B, dtype=torch.float32, device=dev)
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        for t in range(T):
            _, wpred = self._lrp_step(tr, enc, t, toks, skip, hcw, True)
            check(lib.lrpx_argmax_logprob_rows(ptr(wpred), self.V, B, self.V, ptr(nxt), ptr(lp), stream_ptr()))
            alive = unfinished.any()                                        # the reference's `break`
            unfinished = unfinished & (nxt != end_id)
            toks[:, t + 1] = torch.where(alive, nxt * unfinished, torch.zeros_like(nxt))
            lps[:, t] = torch.where(alive, lp, torch.zeros_like(lp))
        return toks[:, 1:].contiguous(), lps

    def forwardlrp_context(self, enc, captions, caption_lengths, skip_ids):
        """The forward half of the model's `forwardlrp_context` (models/gridTDmodel.py:579-630, models/aoamodel.py:628-677; LRP-inference
        fine-tuning): teacher-forced decoding with the model's own forward where every step's scores are recomputed
        from the fc input re-weighted by the relevance of the step's arg-max word (`get_lrp_weight_step`, handed the RAW scores here by
        both models).  captions (B, >= L) int64 incl. <start> in column 0; L = max(caption_lengths) - 1.  Dropout is the identity
        (evaluation mode).  Returns (predictions (B,L,V), weighted_predictions (B,L,V), L).  The loss and its gradients
        (train.py:211-263) are training and stay outside the path."""
        B, dev = enc["B"], self.device
        L = int(max(caption_lengths)) - 1
        captions = captions.to(dev, torch.int64).contiguous()
        assert captions.shape[0] == B and captions.shape[1] >= L
        skip = self._skip_mask(skip_ids)
        toks = captions[:, :L + 1].contiguous() if captions.shape[1] > L else torch.cat(
            [captions, captions.new_zeros(B, 1)], 1).contiguous()          # column t is the input of step t
        tr = self._decode_trace(enc, B, L, lrp=True)
        hcw = torch.empty(B, self.H, device=dev)
        preds = torch.empty(B, L, self.V, device=dev)
        wpreds = torch.empty(B, L, self.V, device=dev)
        for t in range(L):
            preds[:, t], wpreds[:, t] = self._lrp_step(tr, enc, t, toks, skip, hcw, False)
        return preds, wpreds, L

    # ---- static-buffer drivers ------------------------------------------------------------------------------------------------------------
    def _static_step(self, graph, key, src, captions, step):
        """`step(src, captions)` - an eager `explain_batch` - from static buffers, one set per `key`, kept in `self._graphs` (graph=True) or
        `self._recordings`; both are created on first use and never copied into a `replica()`.

        Recorded step (`_lib.Recording`): the first call with a key runs the step eagerly on static copies of the inputs and keeps its
        library calls - functions, arguments, and every buffer they point at; later calls copy the inputs into those static buffers and
        issue the same calls again: the same kernels in the same order on the same stream, as ordinary launches (they overlap with other
        streams' kernels like any launch; a HIP graph replay did not), without the interpreter's ~9 us per launch.  Bit-identical to the
        eager step by construction.  Captions of equal length only (`lens` makes the launch sequence data-dependent).

        HIP graph: the launches of a step (~450 with the VGG16 chain, ~330 bottom-up) issued by one hipGraphLaunch.  Worth it for a
        SINGLE batch in flight (the host issues ~4 us per launch); with batches in flight on several streams eager launches are faster
        (profiles/graph_replay_fix.txt) - a replayed graph does not overlap with its neighbours the way independent kernels do.
        Every replay is bit-identical to the eager step too (tests/test_gpu_graph_replay.py): the library clears with a kernel while
        its stream is being captured (csrc/lrpx_core.hip: clear_async; a captured hipMemsetAsync did not clear a trace's arena on replay).

        Either way the returned tensors are the static outputs: overwritten by the next call with the same key on this engine (take
        `replica()`s for batches in flight)."""
        store = self.__dict__.setdefault("_graphs" if graph else "_recordings", {})
        rec = store.get(key)
        if rec is None:
            inputs = (src.clone(), captions.clone())
            # warm-up outside the capture / recording: one-time work (kernel attributes, index caches, workspace allocations) must not be replayed
            if graph:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    step(*inputs)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                rec = store[key] = _CapturedGraph(step, inputs)
            else:
                step(*inputs)
                rec = _lib.Recording()
                with rec:
                    rec.result = step(*inputs)
                rec.inputs = inputs
                store[key] = rec
                return rec.result
        rec.inputs[0].copy_(src)
        rec.inputs[1].copy_(captions)
        return rec.replay()

    def _explain_stream(self, batches, depth, explain):
        """Explain an iterable of independent (images, captions[, lens]) batches with `depth` batches in flight, each on its own HIP
        stream and buffer set: `explain(replica, images, captions, lens)` is the engine's `explain_batch`.  Batches are independent
        (no exchange step), and roughly a seventh of a batch's time is the decoder's lock-step chain of small
        latency-bound kernels: it overlaps the MFMA-bound CNN relevance chain of the neighbouring batch.  Yields (maps, r_words) in
        input order; each result is complete (its stream has been synchronised) when it is yielded.  Results are bit-identical to
        serial `explain_batch` calls."""
        depth = max(1, int(depth))
        if not hasattr(self, "_replicas"):
            self._replicas, self._streams = [self], [torch.cuda.Stream(device=self.device)]
        while len(self._replicas) < depth:
            self._replicas.append(self.replica())
            self._streams.append(torch.cuda.Stream(device=self.device))
        for rep in self._replicas[1:]:                                     # kept between calls: the rule may have been set since
            rep.lrp_params = getattr(self, "lrp_params", None)
        pending = []
        for i, batch in enumerate(batches):
            images, captions = batch[0], batch[1]
            lens = batch[2] if len(batch) > 2 else None
            k = i % depth
            st = self._streams[k]
            st.wait_stream(torch.cuda.current_stream(self.device))     # inputs produced on the caller's stream
            with torch.cuda.stream(st):
                out = explain(self._replicas[k], images, captions, lens)
                ev = torch.cuda.Event()
                ev.record(st)
            for t in out:
                t.record_stream(torch.cuda.current_stream(self.device))
            # the side stream reads the caller's tensors (`.to()` copies nothing when they already are device fp32 / int64):
            # keep them alive until the batch's event has completed, or the caching allocator could hand their memory to
            # the caller's next batch while this one is still queued
            pending.append((out, ev, images, captions))
            if len(pending) >= depth:
                o, e, _, _ = pending.pop(0)
                e.synchronize()
                yield o
        for o, e, _, _ in pending:
            e.synchronize()
            yield o

    # ---- the tail of the batch entry points, shared rules -----------------------------------------------------------------------------
    def _finish(self, rg, B, T, feat, r_words, row2img, maps_of, map_shape, accumulate=False, extra=(), features=None):
        """`feat` (rows, P, C): the decoder's result for the valid (image, word) rows (all B*T, or the compact rows of captions of
        unequal length, `rg`; explainers/ragged.py) -> the entry point's tuple.  `maps_of(feat, row2img)`: the encoder stage (not
        called without rows: every caption empty).  Unequal lengths: back to the padded (image, word) layout, zeros behind an image's
        last word, running sums per image over ITS words with `accumulate`; else `cumsum_maps` (the running sums the reference
        returns, lrp_wrapper.py:64-82 quirk).  Returns (maps (B,T,*map_shape), r_words (B,T,T)) + extra [+ (feat (B,T,P,C),) +
        features: with features=(tr, enc), the `return_features` members]."""
        maps = maps_of(feat, row2img) if feat.shape[0] else feat.new_zeros(0, *map_shape)
        if rg is not None and not rg.full:
            maps = ops.scatter_maps(maps, rg, accumulate=accumulate)
            if features is not None:
                feat = ops.scatter_maps(feat, rg)
        elif accumulate:
            maps = ops.cumsum_maps(maps, B, T)
        out = (maps.view(B, T, *map_shape), r_words.view(B, T, T)) + tuple(extra)
        if features is not None:
            out = out + (feat.view(B, T, *feat.shape[1:]),) + tuple(features)
        return out

    def _proj_rule(self, a_proj, n, P, x, row2img, out, u=None, kind=None, in_amax=None):
        """the `img_projector` dense rule over n x P (word, pixel) rows: out = x * (W^T a_proj) [+ u].  Split products on the fp16
        matrix cores while `_f16()` ("f16"; csrc/dense_f16x3.hip); in the default (exact) arithmetic the same tile on the bf16 matrix cores
        with operands split exactly into three bf16 parts ("b6": six products, fp32 range - what conv mode 1 is for the VGG16
        chains); the fp32 MFMA where the sizes do not fit or `dense_bf16x6` is off ("f32").  kind=None: chosen here."""
        H, Cc = self.H, self.C
        if kind is None:
            kind = "f16" if self.p_proj_rel_h is not None and self._f16() else \
                "b6" if self.p_proj_rel_6 is not None and self.dense_bf16x6 else "f32"
        kw = dict(pix_per_map=P, oc_split=Cc, x=x, u=u, map2img=row2img, out0=out)
        if kind == "f16":
            ops.conv_mfma(a_proj, self.p_proj_rel_h, n, 0, H, -(-Cc // 32) * 32, 1, EPI_REL, f16x3=1,
                          in_amax=in_amax if in_amax is not None else ops.amax_maps(a_proj, n), **kw)
        elif kind == "b6":
            ops.conv_mfma(a_proj, self.p_proj_rel_6, n, 0, H, -(-Cc // 32) * 32, 1, EPI_REL, bf16x6=1, **kw)
        else:
            ops.conv_mfma(a_proj, self.p_proj_rel, n, 0, H, Cc, 1, EPI_REL, **kw)

    def grad_cam(self, enc, d_feat, row2img):
        """`grad_cam` (models/gridTDmodel.py:1760-1771, models/aoamodel.py:1669-1689) for every (image, word) row: (rows,P,C) gradients
        at the encoder's features -> (rows,P) heat maps."""
        rows, P = d_feat.shape[0], d_feat.shape[1]
        cam = torch.empty(rows, P, device=self.device, dtype=torch.float32)
        check(_lib.load().lrpx_gradcam(ptr(enc["feats"]), ptr(d_feat.contiguous()), ptr(row2img), ptr(cam), rows, P, self.C, stream_ptr()))
        return cam
