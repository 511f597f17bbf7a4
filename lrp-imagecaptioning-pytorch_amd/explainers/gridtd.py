"""Batched gridTD LRP engine + the drop-in `ExplainGridTDAttention` explainer.

Reference: models/gridTDmodel.py:705-1211 (`ExplainGridTDAttention`).  The reference explains one
image at a time with ~50k tiny tensor ops per image; here a batch of B images x T words is traced
and explained in lock-step by HIP kernels behind the lrpx C ABI (see csrc/decoder_gridtd.hip; the model-agnostic kernels: csrc/decoder_blocks.hip).
The host logic below only sequences kernel launches; torch is used for device memory."""
import ctypes as C

import torch

from .. import _lib, ops
from .._lib import (EPI_PLAIN, EPI_REL, GridGradState, GridRelState, GridStepArgs, GridTrace, PACK_DENSE, PACK_DENSE_T, check, ptr,
                    ptr_at, stream_ptr)
from .dropin import ExplainerBase
from .engine_base import VGG_PREFIX, EngineBase, _t, resnet_encoder_keys  # noqa: F401  (the names are read from here too)
from .ragged import ragged


class GridTDEngine(EngineBase):
    """Device-resident gridTD model + trace/relevance pipelines.  `state` is the reference model's
    `state_dict` (torch tensors or numpy arrays, names of models/gridTDmodel.py:111-130).

    The encoder (models/gridTDmodel.py:23-37) is `self.cnn`: `ops.Vgg16` built from the VGG16 keys under `img_encoder.encoder.`
    (`self.vgg` is then the same object), or `ops.ResNetEncoder` - from `encoder=`, an nn.Module on the GPU that
    `ops.match_bottleneck_resnet` accepts, or from a state dict whose encoder keys are those of models/resnet.py
    (`ops.bottleneck_resnet_from_state`).  `encoder_conv_mode` (0 / 1, default 1: the exact bf16 split) is the ResNet engine's
    arithmetic, fixed here; the decoder GEMMs of such an engine are never on the fp16 split products.  Image and feature-map sizes
    come from the images and the encoder; the decoder's own sizes C (`img_projector`) and P (`AdaAttention.W_v_proj`: 196 in the
    reference, :127 - a stride-32 ResNet therefore runs at 448 x 448) must match them (`encode` checks).  DESIGN.md 5.11."""

    ENCODER_CONV_MODES = EngineBase._ENCODER_CONV_MODES

    def __init__(self, state, device="cuda", encoder=None, encoder_conv_mode=1):
        self._build(state, device, encoder, encoder_conv_mode)

    def _build(self, state, device, encoder, encoder_conv_mode, need_encoder=True):
        sd = self._init_encoder(state, device, encoder, encoder_conv_mode, need_encoder)          # (explainers/engine_base.py)
        self.sd = sd
        self.V, self.E = sd["embedding.weight"].shape
        self.H = sd["fc.weight"].shape[1]
        self.C = sd["img_projector.weight"].shape[1]
        self.P = sd["AdaAttention.W_v_proj.weight"].shape[0]
        H, E, Cc = self.H, self.E, self.C
        Kg = sd["global_img_feature_proj.weight"].shape[1]       # C: the mean of the encoder's features; bottom-up (`GridTDBUEngine`): H
        assert H == 512 and E == 512, "kernels are built for hidden=embed=512 (config.py:123-124)"
        # --- forward weights
        a, l = "AdaLSTM.lstm_cell.", "LanguageLSTM."
        self.Wcat1 = torch.cat([torch.cat([sd[a + "weight_ih"], sd[a + "weight_hh"]], 1),
                                torch.cat([sd["AdaLSTM.x_gate.weight"], sd["AdaLSTM.h_gate.weight"]], 1)], 0).contiguous()
        self.bcat1 = torch.cat([sd[a + "bias_ih"] + sd[a + "bias_hh"],
                                sd["AdaLSTM.x_gate.bias"] + sd["AdaLSTM.h_gate.bias"]]).contiguous()
        self.Wcat2 = torch.cat([sd[l + "weight_ih"], sd[l + "weight_hh"]], 1).contiguous()
        self.bcat2_explainer = (sd[l + "bias_ih"] + sd[l + "bias_ih"]).contiguous()   # quirk: gridTDmodel.py:789
        self.bcat2_model = (sd[l + "bias_ih"] + sd[l + "bias_hh"]).contiguous()       # nn.LSTMCell
        # gate rows interleaved for the fused decoder step of the teacher-forced trace (lrpx_gridtd_fwd_steps): row 16 j + 4 gate + u = row
        # gate * H + 4 j + u, so that one workgroup of a gate linear holds the i, f, g, o pre-activations of the hidden units 4j .. 4j+3
        self.fused_steps = H % 16 == 0 and E % 16 == 0          # False: the 7-launch step (A/B; the decoding loops always use it)
        if self.fused_steps:
            jj, qq, uu = torch.meshgrid(torch.arange(H // 4), torch.arange(4), torch.arange(4), indexing="ij")
            il = (qq * H + 4 * jj + uu).reshape(-1).to(self.Wcat1.device)
            self.Wcat1_il, self.bcat1_il = self.Wcat1[:4 * H][il].contiguous(), self.bcat1[:4 * H][il].contiguous()
            self.Wcat2_il = self.Wcat2[il].contiguous()
            self.bcat2_explainer_il, self.bcat2_model_il = self.bcat2_explainer[il].contiguous(), self.bcat2_model[il].contiguous()
        self.w_proj2d = sd["img_projector.weight"].reshape(H, Cc).contiguous()
        kc = ops.conv_kc(0, 1, Cc)
        self.p_proj_fwd = ops.pack_weights(self.w_proj2d, H, Cc, 1, PACK_DENSE, kc)
        self.p_attv_fwd = ops.pack_weights(sd["AdaAttention.W_v_proj.weight"], self.P, H, 1, PACK_DENSE, kc)
        self.p_fc_fwd = ops.pack_weights(sd["fc.weight"], self.V, H, 1, PACK_DENSE, kc)
        # fp16 split-product packs (csrc/dense_f16x3.hip): built always, USED only while ops.decoder_f16() says so (`_f16()`: conv modes 2 / 3)
        self.force_f16 = None            # True / False: this engine's decoder GEMMs on / off the fp16 split products whatever the conv mode (A/B and tests)
        self.p_fc_fwd_h = ops.pack_weights_f16x2(sd["fc.weight"], self.V, H, _lib.PACK_FWD, taps=1) if H % 64 == 0 else None
        # --- guided-backprop weights: full gate matrices, contraction over the 4H gate rows (gridTDmodel.py:1637-1659)
        self.p_g2 = ops.pack_weights(self.Wcat2, 4 * H, 3 * H, 1, PACK_DENSE_T, kc)
        self.p_g1 = ops.pack_weights(sd[a + "weight_ih"].contiguous(), 4 * H, 2 * E + H, 1, PACK_DENSE_T, kc)
        self.p_gp_grad = self.p_gp_rel = ops.pack_weights(sd["global_img_feature_proj.weight"], E, Kg, 1, PACK_DENSE_T, kc)
        # --- relevance weights: g-gate rows of the LSTMs, [W_ih^g | W_hh^g]  (gridTDmodel.py:1019-1024)
        wg1 = torch.cat([sd[a + "weight_ih"][2 * H:3 * H], sd[a + "weight_hh"][2 * H:3 * H]], 1).contiguous()
        wg2 = torch.cat([sd[l + "weight_ih"][2 * H:3 * H], sd[l + "weight_hh"][2 * H:3 * H]], 1).contiguous()
        self.p_wg1 = ops.pack_weights(wg1, H, 2 * E + 2 * H, 1, PACK_DENSE_T, kc)
        self.p_wg2 = ops.pack_weights(wg2, H, 3 * H, 1, PACK_DENSE_T, kc)
        self.p_gp_rel = ops.pack_weights(sd["global_img_feature_proj.weight"], E, Kg, 1, PACK_DENSE_T, kc)
        self.p_proj_rel = ops.pack_weights(self.w_proj2d, H, Cc, 1, PACK_DENSE_T, kc)
        # the projector rule runs over every (word, pixel) row: split products on the fp16 matrix cores (csrc/dense_f16x3.hip)
        self.p_proj_rel_h = ops.pack_weights_f16x2(self.w_proj2d, H, Cc, _lib.PACK_BWD_PLAIN, taps=1) if H % 64 == 0 else None
        # ... in the default (exact) arithmetic: the same tile on the bf16 matrix cores with operands split exactly into three bf16 parts
        # (dense_f16x3.hip, B6: six products, fp32 range - what conv mode 1 is for the VGG16 chains); the fp32 MFMA where the sizes do not fit
        self.p_proj_rel_6 = ops.pack_weights_bf16x3(self.w_proj2d, H, Cc, _lib.PACK_BWD_PLAIN, taps=1) if (H % 32 == 0 and Cc % 4 == 0) else None
        self.dense_bf16x6 = True         # False: those rules on the fp32 MFMA kernel (A/B and tests)
        # ... and the lock-step gate rules (rows = images x words): the few-row kernel of the same file.  `lockstep_f16 = False`
        # puts them back on the fp32 MFMA (csrc/dense_small.hip; A/B: tools/phase_times.py --lockstep-fp32)
        self.lockstep_f16 = H % 16 == 0 and E % 16 == 0
        self.p_wg1_h = ops.pack_weights_f16x2(wg1, H, 2 * E + 2 * H, _lib.PACK_BWD_PLAIN, taps=1) if self.lockstep_f16 else None
        self.p_wg2_h = ops.pack_weights_f16x2(wg2, H, 3 * H, _lib.PACK_BWD_PLAIN, taps=1) if self.lockstep_f16 else None
        self.p_gp_rel_h = ops.pack_weights_f16x2(sd["global_img_feature_proj.weight"], E, Kg, _lib.PACK_BWD_PLAIN, taps=1) if self.lockstep_f16 else None
        torch.cuda.synchronize()
        self._idx_cache = {}

    # ------------------------------------------------------------------------------------------
    def _alloc_trace(self, B, T, grad=False):
        dev, H, E, P = self.device, self.H, self.E, self.P
        shapes = {"xh1": (B, T, 2 * E + 2 * H), "xh2": (B, T, 3 * H), "alpha": (B, T, P), "beta": (B, T)}
        for k in ("h1", "c1", "h2", "c2"):
            shapes[k] = (B, T + 1, H)
        for k in ("g1", "i1", "f1", "g2", "i2", "f2", "s", "ctx", "ctx_hat", "hc"):
            shapes[k] = (B, T, H)
        names = ["xh1", "xh2", "h1", "c1", "h2", "c2", "g1", "i1", "f1", "g2", "i2", "f2", "s", "ctx", "ctx_hat", "hc",
                 "alpha", "beta"]
        if grad:     # the gradient explainers also keep the output gates and the sentinel gate (:1323-1422)
            for k in ("o1", "o2", "sgate"):
                shapes[k] = (B, T, H)
            names += ["o1", "o2", "sgate"]
        tr = dict(B=B, T=T)
        tr.update(ops.zeros_arena(dev, shapes))            # one allocation, one fill
        c = GridTrace()
        c.B, c.T, c.H, c.E, c.P = B, T, H, E, P
        for k in names:
            setattr(c, k, ptr(tr[k]))
        tr["_c"] = c
        return tr

    def feature_shape(self, images):
        """(h, w, C) of the encoder's feature map for these images (host arithmetic)"""
        if self.resnet:
            if images.dim() != 4:
                raise ValueError("GridTDEngine: images must be (B, 3, H, W), got {}".format(tuple(images.shape)))
            return self.cnn.feature_shape(int(images.shape[2]), int(images.shape[3]))
        return self.cnn.feat_hw + (512,)

    def _check_sizes(self, images):
        """the decoder is built for P pixels of C channels (`AdaAttention.W_v_proj`, `img_projector`): refuse other images here, before
        any kernel runs.  Returns the feature map's (h, w)."""
        h, w, c = self.feature_shape(images)
        if h * w != self.P or c != self.C:
            raise ValueError("GridTDEngine: {}x{} images give a {}x{} feature map = {} pixels of {} channels; the decoder is built for {} "
                             "pixels (AdaAttention.W_v_proj) of {} channels (img_projector)".format(
                                 int(images.shape[2]), int(images.shape[3]), h, w, h * w, c, self.P, self.C))
        return h, w

    GRADIENT_MISSING = "the gradient chain through the ResNet encoder (guided backprop / plain gradient of ops.ResNetEncoder) is missing"

    def encode(self, images):
        """Encoder forward + the image-side constants of get_hidden_parameters (gridTDmodel.py:941-950)."""
        lib = _lib.load()
        st = stream_ptr()
        B = images.shape[0]
        H, E, Cc, P = self.H, self.E, self.C, self.P
        self._check_sizes(images)
        images = images.to(self.device, torch.float32).contiguous()
        feats = self.cnn.forward(images)                                   # (B,P,C) NHWC view into the trace
        enc = dict(B=B, feats=feats)
        enc["avg"] = torch.empty(B, Cc, device=self.device)
        check(lib.lrpx_mean_pixels(ptr(feats), ptr(enc["avg"]), B, P, Cc, st))
        enc["proj_pre"] = torch.empty(B, P, H, device=self.device)
        ops.conv_mfma(feats, self.p_proj_fwd, B, 0, Cc, H, 1, EPI_PLAIN, pix_per_map=P, oc_split=H,
                      bias=self.sd["img_projector.bias"], out0=enc["proj_pre"])
        enc["Vp"] = torch.empty_like(enc["proj_pre"])
        check(lib.lrpx_relu(ptr(enc["proj_pre"]), ptr(enc["Vp"]), enc["Vp"].numel(), st))
        enc["glob_pre"] = torch.empty(B, E, device=self.device)
        check(lib.lrpx_linear_small(ptr(enc["avg"]), Cc, ptr(self.sd["global_img_feature_proj.weight"]),
                                    ptr(self.sd["global_img_feature_proj.bias"]), ptr(enc["glob_pre"]), E, B, Cc, E, 0, st))
        enc["glob"] = torch.empty_like(enc["glob_pre"])
        check(lib.lrpx_relu(ptr(enc["glob_pre"]), ptr(enc["glob"]), enc["glob"].numel(), st))
        # time-invariant part of the attention scores: W_v_proj(V) + b  (gridTDmodel.py:79)
        enc["att_img"] = torch.empty(B, P, P, device=self.device)
        ops.conv_mfma(enc["Vp"], self.p_attv_fwd, B, 0, H, -(-P // 32) * 32, 1, EPI_PLAIN, pix_per_map=P, oc_split=P,
                      bias=self.sd["AdaAttention.W_v_proj.bias"], out0=enc["att_img"])
        return enc

    def _step(self, tr, enc, t, tokens, model_bias, after_lstm1=None):
        lib = _lib.load()
        st = stream_ptr()
        B, T, H, E = tr["B"], tr["T"], self.H, self.E
        c = C.byref(tr["_c"])
        sd = self.sd
        check(lib.lrpx_gridtd_fwd_pre(c, t, ptr(enc["glob"]), ptr(sd["embedding.weight"]), ptr(tokens),
                                      tokens.shape[1], st))
        W1 = 2 * E + 2 * H
        if "_zz1" not in tr:
            tr["_zz1"] = torch.empty(B, 5 * H, device=self.device)
            tr["_zz2"] = torch.empty(B, 4 * H, device=self.device)
            tr["_att_scr"] = torch.empty(B, 3 * self.P, device=self.device)
        zz1 = tr["_zz1"]
        check(lib.lrpx_linear_small(ptr_at(tr["xh1"], t * W1), T * W1, ptr(self.Wcat1), ptr(self.bcat1), ptr(zz1),
                                    5 * H, B, W1, 5 * H, 0, st))
        check(lib.lrpx_gridtd_fwd_lstm(c, t, ptr(zz1), 5 * H, 1, st))
        if after_lstm1 is not None:
            after_lstm1(t)
        aa = "AdaAttention."
        scr = tr["_att_scr"]
        check(lib.lrpx_gridtd_fwd_attention(c, t, ptr(enc["Vp"]), ptr(enc["att_img"]), ptr(sd[aa + "W_g_proj.weight"]),
                                            ptr(sd[aa + "W_s_proj.weight"]), ptr(sd[aa + "W_s_proj.bias"]),
                                            ptr(sd[aa + "w_h.weight"]), ptr(scr), st))
        zz2 = tr["_zz2"]
        b2 = self.bcat2_model if model_bias else self.bcat2_explainer
        check(lib.lrpx_linear_small(ptr_at(tr["xh2"], t * 3 * H), T * 3 * H, ptr(self.Wcat2), ptr(b2), ptr(zz2), 4 * H,
                                    B, 3 * H, 4 * H, 0, st))
        check(lib.lrpx_gridtd_fwd_lstm(c, t, ptr(zz2), 4 * H, 2, st))

    def trace(self, enc, captions, model_bias=False, predictions=True, grad=False):
        """get_hidden_parameters (gridTDmodel.py:952-1012) for B images under teacher forcing.
        captions: (B,T+1) int64 on device, column 0 = <start>.  grad=True: the gradient explainers' trace
        (:1323-1422: correct LSTM bias, output + sentinel gates kept)."""
        lib = _lib.load()
        B, T = captions.shape[0], captions.shape[1] - 1
        captions = captions.to(self.device, torch.int64).contiguous()      # (token ids index the embedding table: never another width)
        tr = self._alloc_trace(B, T, grad)
        model_bias = model_bias or grad
        # the T steps in one native call (lrpx_gridtd_fwd_steps: the launches of `_step`, its host loop in C)
        H, P, dev = self.H, self.P, self.device
        tr["_zz1"], tr["_zz2"], tr["_att_scr"] = torch.empty(B, 5 * H, device=dev), torch.empty(B, 4 * H, device=dev), torch.empty(B, 3 * P, device=dev)
        sa, sd, aa = GridStepArgs(), self.sd, "AdaAttention."
        sa.glob, sa.emb, sa.tok, sa.tok_ld = ptr(enc["glob"]), ptr(sd["embedding.weight"]), ptr(captions), captions.shape[1]
        sa.w_cat1, sa.b_cat1, sa.w_cat2 = ptr(self.Wcat1), ptr(self.bcat1), ptr(self.Wcat2)
        sa.b_cat2 = ptr(self.bcat2_model if model_bias else self.bcat2_explainer)
        if self.fused_steps:         # gate rows interleaved: gate linear + LSTM cell in one launch (lrpx_gridtd_fwd_steps)
            sa.w_il1, sa.b_il1, sa.w_il2 = ptr(self.Wcat1_il), ptr(self.bcat1_il), ptr(self.Wcat2_il)
            sa.b_il2 = ptr(self.bcat2_model_il if model_bias else self.bcat2_explainer_il)
        sa.Vp, sa.att_img = ptr(enc["Vp"]), ptr(enc["att_img"])
        sa.Wg, sa.Ws, sa.bs, sa.wh = ptr(sd[aa + "W_g_proj.weight"]), ptr(sd[aa + "W_s_proj.weight"]), ptr(sd[aa + "W_s_proj.bias"]), ptr(sd[aa + "w_h.weight"])
        sa.zz1, sa.zz2, sa.att_scratch = ptr(tr["_zz1"]), ptr(tr["_zz2"]), ptr(tr["_att_scr"])
        check(lib.lrpx_gridtd_fwd_steps(C.byref(tr["_c"]), 0, T, C.byref(sa), stream_ptr()))
        tr["captions"] = captions
        tr["logit"] = torch.empty(B * T, device=self.device)
        check(lib.lrpx_target_logit(ptr(tr["hc"]), ptr(self.sd["fc.weight"]), ptr(self.sd["fc.bias"]), ptr(captions),
                                    T + 1, ptr(tr["logit"]), B, T, self.H, stream_ptr()))
        if predictions:
            tr["pred"] = self.logits(tr["hc"].view(B * T, self.H), fast=True).view(B, T, self.V)
        return tr

    def logits(self, hc_rows, fast=False):
        return EngineBase.logits(self, hc_rows, fast)

    def greedy(self, enc, max_cap_length, start_id, end_id, model_bias=True):
        """GridTDModel.greedy_search (gridTDmodel.py:480-520): argmax per step; after the first <end> the
        sequence is padded with 0.  Returns int64 (B, max_cap_length) incl. <start>."""
        lib = _lib.load()
        B = enc["B"]
        T = max_cap_length - 1
        toks = torch.zeros(B, T + 1, dtype=torch.int64, device=self.device)
        toks[:, 0] = start_id
        tr = self._alloc_trace(B, T)
        nxt = torch.empty(B, dtype=torch.int64, device=self.device)
        unfinished = torch.ones(B, dtype=torch.bool, device=self.device)
        for t in range(T):
            self._step(tr, enc, t, toks, model_bias)
            lg = self.logits(tr["hc"][:, t].contiguous())
            check(lib.lrpx_argmax_rows(ptr(lg), self.V, B, self.V, ptr(nxt), stream_ptr()))
            unfinished = unfinished & (nxt != end_id)          # token bookkeeping (integers), :500-505
            toks[:, t + 1] = nxt * unfinished
        return toks

    # the decode loops of explainers/engine_base.py (beam_search, sample_lrp, forwardlrp_context) on this model's step
    _BEAM_STATE = ("h1", "c1", "h2", "c2")

    def _decode_trace(self, enc, B, T, lrp=False):
        tr = self._alloc_trace(B, T)
        if lrp:      # `sample_lrp` / `forwardlrp_context` run the model's own forward: the sentinel gate on the NEW h1 (gridTDmodel.py:617)
            lib, H, W1 = _lib.load(), self.H, 2 * self.E + 2 * self.H
            c = C.byref(tr["_c"])
            xg, zg = torch.empty(B, W1, device=self.device), torch.empty(B, H, device=self.device)
            w_gate, b_gate = self.Wcat1[4 * H:], self.bcat1[4 * H:]          # [x_gate | h_gate] rows of the fused weight

            def sentinel_new_h(t):
                st = stream_ptr()
                check(lib.lrpx_gridtd_fwd_gate_input(c, t, ptr(xg), st))
                check(lib.lrpx_linear_small(ptr(xg), W1, ptr(w_gate), ptr(b_gate), ptr(zg), H, B, W1, H, 0, st))
                check(lib.lrpx_gridtd_fwd_sentinel(c, t, ptr(zg), H, st))
            tr["_after_lstm1"] = sentinel_new_h
        return tr

    def _decode_step(self, tr, enc, t, toks):
        self._step(tr, enc, t, toks, True, after_lstm1=tr.get("_after_lstm1"))

    def _reweight(self, tr, t, pred, skip, hcw, log_softmax):
        """`get_lrp_weight_step` (models/gridTDmodel.py:548-577): always on the raw scores"""
        check(_lib.load().lrpx_gridtd_lrp_reweight(C.byref(tr["_c"]), t, ptr(pred), self.V, self.V, ptr(self.sd["fc.weight"]), ptr(skip),
                                                   ptr(hcw), stream_ptr()))

    # ------------------------------------------------------------------------------------------
    def relevance(self, enc, tr, lens=None, want_r_feat=True):
        """explain_caption_wordt (gridTDmodel.py:1014-1135) for every (image, word) row at once.
        Returns r_feat (B*T, P, C) relevance of the encoder output (NHWC), r_words (B*T, T) and the row -> image table.
        lens (one caption length per image, list / array / tensor; explainers/ragged.py): words past an image's length are
        skipped by the lock-step kernels (their r_words rows stay zero), and the (word, pixel) rules run on the VALID rows only -
        r_feat is then COMPACT, (sum(lens), P, C) in image-major order, with the matching row -> image table."""
        lib = _lib.load()
        st = stream_ptr()
        B, T, H, E, P, Cc = tr["B"], tr["T"], self.H, self.E, self.P, self.C
        rows = B * T
        dev = self.device
        rg = ragged(lens, B, T, dev)
        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        rs = dict(r_h2n=e(rows, H), r_c2=e(rows, H), r_c1=e(rows, H), r_ch0=e(rows, H), r_h2p=e(rows, H),
                  r_glob=e(rows, E), A=e(rows, H), rx=e(rows, 2 * E + 2 * H), wacc=ops.zeros(rows, T, H, device=dev),
                  r_words=e(rows, T))
        c = GridRelState()
        c.lens = ptr(rg.lens) if rg is not None else None
        for k, v in rs.items():
            setattr(c, k, ptr(v))
        ctr, crs = C.byref(tr["_c"]), C.byref(c)
        idx, row2img, _ = self._row_index(B, T)
        check(lib.lrpx_gridtd_rel_init(ctr, crs, ptr(self.sd["fc.weight"]), ptr(tr["logit"]), ptr(tr["captions"]),
                                       T + 1, st))
        W1 = 2 * E + 2 * H
        f16 = 1 if (self.lockstep_f16 and self._f16()) else 0
        # the T lock-steps in one native call (lrpx_gridtd_rel_steps): phase 0, LanguageLSTM dense rule, phase 1, AdaLSTM dense rule, phase 2
        d2 = ops.conv_desc(rs["A"], self.p_wg2_h if f16 else self.p_wg2, rows, 0, H, 3 * H, 1, EPI_REL, pix_per_map=1, oc_split=3 * H,
                           x=tr["xh2"], map2img=idx[0], out0=rs["rx"], f16x3=f16)
        d1 = ops.conv_desc(rs["A"], self.p_wg1_h if f16 else self.p_wg1, rows, 0, H, W1, 1, EPI_REL, pix_per_map=1, oc_split=W1,
                           x=tr["xh1"], map2img=idx[0], out0=rs["rx"], f16x3=f16)
        check(lib.lrpx_gridtd_rel_steps(ctr, crs, T, C.byref(d2), C.byref(d1), ptr(idx), idx.shape[1], st))
        return self._rel_tail(enc, tr, rg, rs, ctr, crs, row2img, f16)

    def _rel_tail(self, enc, tr, rg, rs, ctr, crs, row2img, f16):
        """global feature path (:1116-1124) and projector (:1125-1128)"""
        lib, st = _lib.load(), stream_ptr()
        B, T, H, E, P, Cc = tr["B"], tr["T"], self.H, self.E, self.P, self.C
        rows = B * T
        e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)
        a_glob = e(rows, E)
        check(lib.lrpx_gridtd_rel_glob(ctr, crs, ptr(enc["glob_pre"]), ptr(a_glob), st))
        r_avg = e(rows, Cc)
        ops.conv_mfma(a_glob, self.p_gp_rel_h if f16 else self.p_gp_rel, rows, 0, E, -(-Cc // 32) * 32 if f16 else Cc, 1, EPI_REL,
                      pix_per_map=1, oc_split=Cc, x=enc["avg"], map2img=row2img, out0=r_avg, f16x3=f16)
        U = e(rows, Cc)
        check(lib.lrpx_rel_avg_u(ptr(r_avg), ptr(enc["avg"]), ptr(U), rows, T, Cc, P, st))
        check(lib.lrpx_rel_words_norm(ptr(rs["r_words"]), rows, T, st))
        n, rowlist = rows, None
        if rg is not None and not rg.full:       # unequal lengths: the (word, pixel) rule on the valid rows only, compact
            n, rowlist, row2img = rg.n, rg.rows, rg.row2img
            if n == 0:
                return e(0, P, Cc), rs["r_words"], row2img
            U = ops.gather_rows(U, rowlist)
        a_proj = e(n, P, H)
        check(lib.lrpx_gridtd_rel_pix_rows(ctr, crs, ptr(enc["Vp"]), ptr(enc["proj_pre"]), ptr(a_proj), ptr(rowlist), n, st))
        r_feat = e(n, P, Cc)
        self._proj_rule(a_proj, n, P, enc["feats"], row2img, r_feat, u=U)
        return r_feat, rs["r_words"], row2img

    def _static(self, graph, images, captions, accumulate, predictions, *key):
        images = images.to(self.device, torch.float32)
        captions = captions.to(self.device, torch.int64)
        key = (tuple(images.shape), tuple(captions.shape), bool(accumulate), bool(predictions)) + key + (self._f16(),)
        return self._static_step(graph, key, images, captions,
                                 lambda i, c: self.explain_batch(i, c, accumulate=accumulate, predictions=predictions))

    def explain_batch_graph(self, images, captions, accumulate=False, predictions=False):
        """`explain_batch` replayed from a captured HIP graph, one per (B,T) shape (explainers/engine_base.py: `_static_step`)."""
        self._preset_only("explain_batch_graph", self._NO_STATIC_AB)
        self._refuse_resnet("explain_batch_graph", self._NO_GRAPH)
        return self._static(True, images, captions, accumulate, predictions)

    def explain_batch_replay(self, images, captions, accumulate=False, predictions=False):
        """`explain_batch` as a RECORDED step, one per input shape and stream (explainers/engine_base.py: `_static_step`)."""
        self._preset_only("explain_batch_replay", self._NO_STATIC_AB)
        self._refuse_resnet("explain_batch_replay", self._NO_RECORDING)
        return self._static(False, images, captions, accumulate, predictions, _lib.stream_ptr().value,
                            self.vgg.conv_mode if self.vgg is not None else None)

    def guided_gradient(self, enc, tr, lens=None, mask_features=True):
        """ExplainiGridTDGuidedGradient.explain_caption_wordt (gridTDmodel.py:1588-1675) for every (image, word)
        row: decoder BPTT with alpha/beta constant.  `tr` must be a grad=True trace.
        Returns d_feat (B*T, P, C), r_words (B*T, T), row2img.  With `lens` d_feat holds the valid rows only (as `relevance`)."""
        lib = _lib.load()
        st = stream_ptr()
        B, T, H, E, P, Cc = tr["B"], tr["T"], self.H, self.E, self.P, self.C
        rows = B * T
        rg = ragged(lens, B, T, self.device)
        lens = rg.lens if rg is not None else None
        e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)
        gs = dict(d_h2n=e(rows, H), d_c2=e(rows, H), d_c1=e(rows, H), d_ch0=e(rows, H), d_h2p=e(rows, H),
                  d_glob=e(rows, E), gates=e(rows, 4 * H), dx=e(rows, 3 * H), wacc=ops.zeros(rows, T, H, device=self.device),
                  r_words=e(rows, T))
        c = GridGradState()
        c.lens = ptr(lens)
        for k, v in gs.items():
            setattr(c, k, ptr(v))
        ctr, cgs = C.byref(tr["_c"]), C.byref(c)
        _, row2img, _ = self._row_index(B, T)
        check(lib.lrpx_gridtd_grad_init(ctr, cgs, ptr(self.sd["fc.weight"]), ptr(tr["captions"]), T + 1, st))
        for s in range(T):
            check(lib.lrpx_gridtd_grad_step(ctr, cgs, s, 0, st))
            ops.conv_mfma(gs["gates"], self.p_g2, rows, 0, 4 * H, 3 * H, 1, EPI_PLAIN, pix_per_map=1, oc_split=3 * H,
                          out0=gs["dx"])
            check(lib.lrpx_gridtd_grad_step(ctr, cgs, s, 1, st))
            ops.conv_mfma(gs["gates"], self.p_g1, rows, 0, 4 * H, 2 * E + H, 1, EPI_PLAIN, pix_per_map=1,
                          oc_split=2 * E + H, out0=gs["dx"])
            check(lib.lrpx_gridtd_grad_step(ctr, cgs, s, 2, st))
        d_avg = e(rows, Cc)
        ops.conv_mfma(gs["d_glob"], self.p_gp_grad, rows, 0, E, Cc, 1, EPI_PLAIN, pix_per_map=1, oc_split=Cc, out0=d_avg)
        U = e(rows, Cc)
        check(lib.lrpx_scale(ptr(d_avg), ptr(U), d_avg.numel(), 1.0 / P, st))                    # :1667
        check(lib.lrpx_rel_words_norm(ptr(gs["r_words"]), rows, T, st))
        rowlist = None
        if rg is not None and not rg.full:
            rows, rowlist, row2img = rg.n, rg.rows, rg.row2img
            if rows == 0:
                return e(0, P, Cc), gs["r_words"], row2img
            U = ops.gather_rows(U, rowlist)
        a_proj = e(rows, P, H)
        check(lib.lrpx_spread_pixels_rows(ptr(gs["wacc"]), ptr(tr["alpha"]), ptr(lens), ptr(a_proj), B, T, H, P, ptr(rowlist),
                                          rows, st))
        if mask_features:
            mask = e(B, P, Cc)
            check(lib.lrpx_positive_mask(ptr(enc["feats"]), ptr(mask), mask.numel(), st))         # :1674
        else:   # ExplainGridTDGradient.explain_caption_wordt (:1424-1505): same BPTT, no `features <= 0` gate
            mask = torch.ones(B, P, Cc, device=self.device, dtype=torch.float32)
        d_feat = e(rows, P, Cc)
        self._proj_rule(a_proj, rows, P, mask, row2img, d_feat, u=U)                                  # :1668, :1674
        return d_feat, gs["r_words"], row2img

    def explain_batch_guided(self, images, captions, lens=None, return_features=False, gradcam=False):
        """Batched `ExplainiGridTDGuidedGradient.explain_caption`: guided-backprop maps (B,T,3,224,224) and word
        scores (B,T,T).  (No running sums here: the reference zeroes the image gradient per word, :1717.)
        gradcam=True: `ExplainGridTDGuidedGradCam` (:1796-1836) - every map times the 16x expanded Grad-CAM heat map of the
        same (guided) decoder gradient."""
        self._preset_only("explain_batch_guided", self._NO_GRAD_AB)
        self._refuse_resnet("explain_batch_guided", self.GRADIENT_MISSING)
        images = images.to(self.device, torch.float32).contiguous()
        captions = captions.to(self.device, torch.int64).contiguous()
        B, T = captions.shape[0], captions.shape[1] - 1
        enc = self.encode(images)
        tr = self.trace(enc, captions, predictions=False, grad=True)
        rg = ragged(lens, B, T, self.device)
        d_feat, r_words, row2img = self.guided_gradient(enc, tr, rg)

        def maps_of(d_feat, row2img):
            maps = self.vgg.guided_backprop(d_feat, row2img)
            if gradcam:
                maps = ops.guided_gradcam(maps, self.grad_cam(enc, d_feat, row2img), int(round(self.P ** 0.5)))
            return maps
        return self._finish(rg, B, T, d_feat, r_words, row2img, maps_of, (3, 224, 224), features=(tr, enc) if return_features else None)

    def explain_batch_gradient(self, images, captions, lens=None, cam=False, return_features=False):
        """Batched `ExplainGridTDGradient.explain_caption` (models/gridTDmodel.py:1214-1539): plain
        decoder gradient + autograd gradient through the encoder -> maps (B,T,3,224,224), word scores (B,T,T).
        cam=True: `ExplainGridTDGradCam` (:1752-1771) - the per-word result is the Grad-CAM heat map (B,T,196)."""
        self._preset_only("explain_batch_gradient", self._NO_GRAD_AB)
        self._refuse_resnet("explain_batch_gradient", self.GRADIENT_MISSING)
        images = images.to(self.device, torch.float32).contiguous()
        captions = captions.to(self.device, torch.int64).contiguous()
        B, T = captions.shape[0], captions.shape[1] - 1
        enc = self.encode(images)
        tr = self.trace(enc, captions, predictions=False, grad=True)
        rg = ragged(lens, B, T, self.device)
        d_feat, r_words, row2img = self.guided_gradient(enc, tr, rg, mask_features=False)
        return self._finish(rg, B, T, d_feat, r_words, row2img, (lambda d, m: self.grad_cam(enc, d, m)) if cam else self.vgg.gradient,
                            (self.P,) if cam else (3, 224, 224), features=(tr, enc) if return_features else None)

    def explain_batch(self, images, captions, lens=None, accumulate=False, return_features=False, predictions=False):
        """Batched `explain_caption` (gridTDmodel.py:1141-1156): images (B,3,H,W) - 224 x 224 for VGG16, what gives P feature pixels for
        a ResNet encoder (448 x 448 at P = 196) - captions (B,T+1) int64.
        Returns maps (B,T,3,H,W) and r_words (B,T,T) (row t holds t+1 valid entries).
        accumulate=True reproduces the running sums the reference returns (lrp_wrapper.py:64-82 quirk).
        predictions=True also computes the (B,T,V) scores the reference's explainer keeps (`self.predictions`, :1011; read
        by evaluation.py:109) and returns them as a third tensor.  The instance attribute `lrp_params` ({"alpha": 2., "beta": 1.};
        None: the preset) selects the encoder's Conv2d rule (explainers/engine_base.py: `_maps_stage`); the decoder's rules, r_words and
        the feature relevance do not depend on it."""
        maps_of = self._maps_stage("explain_batch")
        images = images.to(self.device, torch.float32).contiguous()
        captions = captions.to(self.device, torch.int64).contiguous()
        B, T = captions.shape[0], captions.shape[1] - 1
        enc = self.encode(images)
        tr = self.trace(enc, captions, predictions=predictions)
        rg = ragged(lens, B, T, self.device)
        r_feat, r_words, row2img = self.relevance(enc, tr, rg)
        # unequal caption lengths (models/gridTDmodel.py:1147-1153 explains `caption_length` words): the chain runs on the
        # sum(lens) valid maps; `_finish` takes the result back to the padded layout
        return self._finish(rg, B, T, r_feat, r_words, row2img, maps_of, tuple(images.shape[1:]), accumulate=accumulate,
                            extra=(tr["pred"],) if predictions else (), features=(tr, enc) if return_features else None)

    def explain_stream(self, batches, depth=3, accumulate=False):
        """`explain_batch` over an iterable of (images, captions[, lens]) batches, `depth` in flight (explainers/engine_base.py)."""
        self._maps_stage("explain_stream")                # a refusal here, not inside the generator's first step
        return self._explain_stream(batches, depth, lambda eng, images, captions, lens: eng.explain_batch(images, captions, lens=lens,
                                                                                                         accumulate=accumulate))


class GridTDBUEngine(GridTDEngine):
    """The bottom-up gridTD model, `GridTDModelBU` (models/gridTDmodel.py:1863-2464): P = 36 region features of C = 2048 channels
    in place of an encoder.  `state` has the key names and shapes of `GridTDModelBU.state_dict()`: `img_projector.weight` (H, C) - a
    Linear -, `global_img_feature_proj.weight` (E, H), `AdaAttention.W_v_proj.weight` (P, H), no `img_encoder.` keys.  Anything else is
    refused (ValueError naming the key) by host logic, before the library is loaded.

    The decoder is `GridTDEngine`'s.  The image side differs (:1912-1915): the global feature is
    relu(global_img_feature_proj(mean_k relu(img_projector(F))[k])) - the mean of the PROJECTED regions -, so its relevance returns under
    the projector rule: r_avg = eps(r_glob, avg, glob_pre, W_gp), r_vp[k] = r_proj[k] + eps(r_avg, Vp[k] / P, avg, eye),
    r_feat[k] = eps(r_vp[k], F[k], proj_pre[k], W_proj) (`_rel_tail`; csrc/decoder_gridtd.hip: lrpx_gridtd_rel_pix_rows_avg).  The
    region relevance (B, T, P, C) is the result: there is no CNN stage, no running sum, and no gradient explainer (the reference
    defines none for this model).  DESIGN.md 5.14."""

    NO_GRADIENT = "no gradient explainer is defined for the bottom-up model (models/gridTDmodel.py:1863-2464 has none)"

    def __init__(self, state, device="cuda"):
        self._check_state(state)
        self._build(state, device, None, 1, need_encoder=False)

    @staticmethod
    def _check_state(state):
        """host logic: the three ways a state is not `GridTDModelBU`'s"""
        for k in state:
            if k.startswith("img_encoder."):
                raise ValueError("GridTDBUEngine: the state holds the encoder key {!r}; the bottom-up model has no encoder "
                                 "(GridTDEngine explains a model with one)".format(k))
        wp, wg = state["img_projector.weight"], state["global_img_feature_proj.weight"]
        if len(wp.shape) != 2:
            raise ValueError("GridTDBUEngine: 'img_projector.weight' is {}-D {}; the bottom-up model's projector is a Linear, "
                             "(H, C)".format(len(wp.shape), tuple(wp.shape)))
        if len(wg.shape) != 2 or wg.shape[1] != wp.shape[0]:
            raise ValueError("GridTDBUEngine: 'global_img_feature_proj.weight' is {}; the bottom-up model takes the global feature from "
                             "the mean of the projected regions, (E, H = {})".format(tuple(wg.shape), wp.shape[0]))

    def feature_shape(self, features):
        """(P, 1, C) of the region features (host arithmetic): the regions as a P x 1 map"""
        if features.dim() != 3:
            raise ValueError("GridTDBUEngine: features must be (B, P, C) region features, got {} (this model has no encoder: images are "
                             "not accepted)".format(tuple(features.shape)))
        return int(features.shape[1]), 1, int(features.shape[2])

    def _check_sizes(self, features):
        p, _, c = self.feature_shape(features)
        if p != self.P or c != self.C:
            raise ValueError("GridTDBUEngine: {} regions of {} channels; the decoder is built for {} regions (AdaAttention.W_v_proj) of {} "
                             "channels (img_projector)".format(p, c, self.P, self.C))
        return p, 1

    def encode(self, features):
        """The image-side constants of `GridTDModelBU.forward` (:1912-1915) from (B, P, C) region features on any device: `Vp`,
        `proj_pre`, `avg` (the mean of Vp over the regions, (B, H)), `glob_pre`, `glob`, `att_img`."""
        self._check_sizes(features)                                        # before any launch
        lib = _lib.load()
        st = stream_ptr()
        H, E, Cc, P = self.H, self.E, self.C, self.P
        feats = features.to(self.device, torch.float32).contiguous()
        B = feats.shape[0]
        e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)
        enc = dict(B=B, feats=feats)
        enc["proj_pre"] = e(B, P, H)
        ops.conv_mfma(feats, self.p_proj_fwd, B, 0, Cc, H, 1, EPI_PLAIN, pix_per_map=P, oc_split=H,
                      bias=self.sd["img_projector.bias"], out0=enc["proj_pre"])
        enc["Vp"] = e(B, P, H)
        check(lib.lrpx_relu(ptr(enc["proj_pre"]), ptr(enc["Vp"]), enc["Vp"].numel(), st))
        enc["avg"] = e(B, H)
        check(lib.lrpx_mean_pixels(ptr(enc["Vp"]), ptr(enc["avg"]), B, P, H, st))
        enc["glob_pre"] = e(B, E)
        check(lib.lrpx_linear_small(ptr(enc["avg"]), H, ptr(self.sd["global_img_feature_proj.weight"]),
                                    ptr(self.sd["global_img_feature_proj.bias"]), ptr(enc["glob_pre"]), E, B, H, E, 0, st))
        enc["glob"] = e(B, E)
        check(lib.lrpx_relu(ptr(enc["glob_pre"]), ptr(enc["glob"]), enc["glob"].numel(), st))
        enc["att_img"] = e(B, P, P)
        ops.conv_mfma(enc["Vp"], self.p_attv_fwd, B, 0, H, -(-P // 32) * 32, 1, EPI_PLAIN, pix_per_map=P, oc_split=P,
                      bias=self.sd["AdaAttention.W_v_proj.bias"], out0=enc["att_img"])
        return enc

    def _rel_tail(self, enc, tr, rg, rs, ctr, crs, row2img, f16):
        """the tail in the order `GridTDModelBU.forward` dictates: the epsilon rule of `global_img_feature_proj` on x = avg (K = E,
        n_oc = H) -> r_avg (rows, H); the pixel rule with the mean term (r_avg joins the bracket before the division by z~(proj_pre));
        the projector rule WITHOUT a `u`."""
        lib, st = _lib.load(), stream_ptr()
        B, T, H, E, P, Cc = tr["B"], tr["T"], self.H, self.E, self.P, self.C
        rows = B * T
        e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)
        a_glob = e(rows, E)
        check(lib.lrpx_gridtd_rel_glob(ctr, crs, ptr(enc["glob_pre"]), ptr(a_glob), st))
        r_avg = e(rows, H)
        ops.conv_mfma(a_glob, self.p_gp_rel_h if f16 else self.p_gp_rel, rows, 0, E, -(-H // 32) * 32 if f16 else H, 1, EPI_REL,
                      pix_per_map=1, oc_split=H, x=enc["avg"], map2img=row2img, out0=r_avg, f16x3=f16)
        check(lib.lrpx_rel_words_norm(ptr(rs["r_words"]), rows, T, st))
        n, rowlist = rows, None
        if rg is not None and not rg.full:       # unequal lengths: the (word, region) rules on the valid rows only, compact
            n, rowlist, row2img = rg.n, rg.rows, rg.row2img
            if n == 0:
                return e(0, P, Cc), rs["r_words"], row2img
        a_proj = e(n, P, H)
        check(lib.lrpx_gridtd_rel_pix_rows_avg(ctr, crs, ptr(enc["Vp"]), ptr(enc["proj_pre"]), ptr(r_avg), ptr(enc["avg"]), ptr(a_proj),
                                               ptr(rowlist), n, st))
        r_feat = e(n, P, Cc)
        self._proj_rule(a_proj, n, P, enc["feats"], row2img, r_feat)
        return r_feat, rs["r_words"], row2img

    def explain_batch(self, features, captions, lens=None, return_features=False, predictions=False):
        """Every word of B captions explained on (B, P, C) region features; captions (B, T+1) int64, column 0 = <start>.  Returns
        r_feat (B, T, P, C) - the relevance of the region features, zero in rows behind an image's last word (`lens`) - and r_words
        (B, T, T) (row t holds t + 1 valid entries); then the (B, T, V) scores with predictions=True; then the trace and `encode`'s
        dict with return_features=True."""
        self._maps_stage("explain_batch")                 # no encoder: `lrp_params` must be None
        enc = self.encode(features)
        captions = captions.to(self.device, torch.int64).contiguous()
        B, T = captions.shape[0], captions.shape[1] - 1
        tr = self.trace(enc, captions, predictions=predictions)
        rg = ragged(lens, B, T, self.device)
        r_feat, r_words, row2img = self.relevance(enc, tr, rg)
        out = self._finish(rg, B, T, r_feat, r_words, row2img, lambda feat, m: feat, (self.P, self.C),
                           extra=(tr["pred"],) if predictions else ())
        return out + ((tr, enc) if return_features else ())

    def _static(self, graph, features, captions, predictions, *key):
        features = features.to(self.device, torch.float32)
        captions = captions.to(self.device, torch.int64)
        key = (tuple(features.shape), tuple(captions.shape), bool(predictions)) + key + (self._f16(),)
        return self._static_step(graph, key, features, captions, lambda f, c: self.explain_batch(f, c, predictions=predictions))

    def explain_batch_graph(self, features, captions, predictions=False):
        """`explain_batch` replayed from a captured HIP graph, one per (B, T) shape (explainers/engine_base.py: `_static_step`)."""
        self._check_sizes(features)
        return self._static(True, features, captions, predictions)

    def explain_batch_replay(self, features, captions, predictions=False):
        """`explain_batch` as a RECORDED step, one per input shape and stream (explainers/engine_base.py: `_static_step`)."""
        self._check_sizes(features)
        return self._static(False, features, captions, predictions, _lib.stream_ptr().value)

    def explain_stream(self, batches, depth=3):
        """`explain_batch` over an iterable of (features, captions[, lens]) batches, `depth` in flight (explainers/engine_base.py)."""
        self._maps_stage("explain_stream")
        return self._explain_stream(batches, depth, lambda eng, features, captions, lens: eng.explain_batch(features, captions, lens=lens))

    def _no_gradient(self, entry):
        raise NotImplementedError("GridTDBUEngine.{}: {}".format(entry, self.NO_GRADIENT))

    def guided_gradient(self, enc, tr, lens=None, mask_features=True):
        self._no_gradient("guided_gradient")

    def explain_batch_guided(self, features, captions, lens=None, return_features=False, gradcam=False):
        self._no_gradient("explain_batch_guided")

    def explain_batch_gradient(self, features, captions, lens=None, cam=False, return_features=False):
        self._no_gradient("explain_batch_gradient")


# ------------------------------------------------------------------------------------------------
# drop-in explainer (models/gridTDmodel.py:705-1211)
# ------------------------------------------------------------------------------------------------
class ExplainGridTDAttention(ExplainerBase):
    """Same constructor, attributes and methods as the reference's `ExplainGridTDAttention`
    (models/gridTDmodel.py:705-1156): `explain_caption(img_filepath) -> (relevance_imgs, relevance_preceeding_words)`,
    `explain_caption_wordt(t)`, `explain_cnn(R)`, `teacherforce_forward(img, ids)`; attributes `.model .word_map .img
    .beam_caption .beam_caption_encode .predictions .alphas .betas .args`.  Conventions: explainers/dropin.py; the caption the
    reference explains is `beam_search(beam_size=2, max_cap_length=50)` (:935-937).

    ResNet encoders (`args.encoder` 'resnet101' / 'renset50', models/gridTDmodel.py:26-31): a `GridTDModel` hands over its
    `model.img_encoder.encoder` (used as it is when it lives on the GPU, rebuilt from the state dict otherwise); a state dict or
    `args.weight` with models/resnet.py key names is built by `ops.bottleneck_resnet_from_state`.  `args.height` / `args.width` size
    the images (448 x 448 for the reference's 196 attention pixels); `args.encoder_conv_mode` (optional, default 1) is the
    engine's.  The gradient-family subclasses refuse such a model (NotImplementedError)."""
    NEEDS_ENCODER_GRADIENT = False      # the gradient family: VGG16 only

    def _engine_key(self):
        from . import engine_cache
        mode = getattr(self.args, "encoder_conv_mode", 1)
        return engine_cache.fingerprint("gridtd", self.args.weight if self.model is None else self.model,
                                        extra=() if mode == 1 else (("encoder_conv_mode", mode),))

    def _refuse_resnet(self):
        raise NotImplementedError("{}: not built for a ResNet encoder - {}".format(type(self).__name__, GridTDEngine.GRADIENT_MISSING))

    def _build_engine(self, state):
        encoder = None
        if hasattr(self.model, "state_dict"):
            enc = getattr(getattr(self.model, "img_encoder", None), "encoder", None)
            if resnet_encoder_keys(state) and isinstance(enc, torch.nn.Module) and all(
                    t.device.type == "cuda" for t in list(enc.parameters()) + list(enc.buffers())):
                encoder = enc                  # the model's own module (else: rebuilt from the same tensors by the engine)
        if self.NEEDS_ENCODER_GRADIENT and resnet_encoder_keys(state):
            self._refuse_resnet()              # before anything is uploaded
        return GridTDEngine(state, encoder=encoder, encoder_conv_mode=getattr(self.args, "encoder_conv_mode", 1))

    def _accept_engine(self, engine):
        if self.NEEDS_ENCODER_GRADIENT and engine.resnet:
            self._refuse_resnet()

    def get_hidden_parameters(self, img, caption_encode=None, max_cap_length=50):
        """Forward trace (:933-1012).  `img`: file path or a (1,3,H,W) tensor of the encoder's image size (224 x 224 for VGG16)."""
        self._hidden_parameters(img, caption_encode, 2, max_cap_length)

    def _explain_rows(self, head_idx):
        return self.engine.relevance(self._enc, self._tr)

    def explain_caption_wordt(self, t):
        """(:1014-1135) -> (r_img_feature (1,C,h,w), r_words (t+1,))"""
        return self._explain_wordt(t)

    def explain_caption(self, img_filepath, t_list=None, caption_encode=None):
        """(:1141-1156) -> ([T] x (1,3,H,W), [T] x (t+1,)); the LRP maps are the reference's running sums."""
        return self._explain_caption(img_filepath, caption_encode)


class ExplainiGridTDGuidedGradient(ExplainGridTDAttention):
    """Drop-in for the reference's `ExplainiGridTDGuidedGradient` (models/gridTDmodel.py:1585-1723; the spelling is
    the reference's): guided backprop instead of LRP, same `explain_caption` surface."""
    EX_TYPE = 'GuidedBackpropagate'
    TF_MODEL_BIAS = True
    NEEDS_ENCODER_GRADIENT = True
    _RUNNING_SUMS = False

    def get_hidden_parameters(self, img, caption_encode=None, max_cap_length=50):
        super().get_hidden_parameters(img, caption_encode, max_cap_length)
        if self.caption_length:
            self._trace(grad=True)             # :1323-1422 (correct LSTM bias)

    def _explain_rows(self, head_idx):
        return self.engine.guided_gradient(self._enc, self._tr)

    def _cnn(self, d_feat, row2img):
        return self.engine.vgg.guided_backprop(d_feat, row2img)

    def explain_cnn(self, d_img_feature):          # (the reference's argument name in this family)
        return super().explain_cnn(d_img_feature)


class ExplainGridTDGuidedGradCam(ExplainiGridTDGuidedGradient):
    """Drop-in for `ExplainGridTDGuidedGradCam` (models/gridTDmodel.py:1796-1836): the guided-backprop map of every word
    times the Grad-CAM heat map of the same decoder gradient expanded 16x by `skimage.transform.pyramid_expand` (:1826).
    (`d_img_feature[self.image_features < 0] = 0`, :1815, never selects anything: the features are ReLU outputs.)"""
    EX_TYPE = 'GuidedGradCam'

    def grad_cam(self, img_feature, grads):
        """(1,C,h,w) features and gradients -> (h, w) heat map (:1799-1810)"""
        return _grad_cam_one(img_feature, grads).view(img_feature.shape[-2], img_feature.shape[-1])

    def explain_cnn(self, d_img_feature):
        guided = self.engine.vgg.guided_backprop(*self._one_map(d_img_feature))
        cam = self.grad_cam(self.image_features, d_img_feature).reshape(1, -1)
        return ops.guided_gradcam(guided, cam, self.image_features.shape[-1])

    def _cnn(self, d_feat, row2img):
        eng = self.engine
        return ops.guided_gradcam(eng.vgg.guided_backprop(d_feat, row2img), eng.grad_cam(self._enc, d_feat, row2img),
                                  int(round(eng.P ** 0.5)))


class ExplainGridTDGradient(ExplainiGridTDGuidedGradient):
    """Drop-in for the reference's `ExplainGridTDGradient` (models/gridTDmodel.py:1214-1539): plain gradient - the same
    hand-written decoder BPTT as the guided explainer without its three gates, and the autograd gradient through the
    encoder (`explain_cnn`, :1507-1521).  (In the reference the guided class derives from this one; here the
    inheritance runs the other way, the surface is the same.)"""
    EX_TYPE = 'gradient'

    def _explain_rows(self, head_idx):
        return self.engine.guided_gradient(self._enc, self._tr, mask_features=False)

    def _cnn(self, d_feat, row2img):
        return self.engine.vgg.gradient(d_feat, row2img)


class ExplainGridTDGradCam(ExplainGridTDGradient):
    """Drop-in for `ExplainGridTDGradCam` (models/gridTDmodel.py:1752-1771): `explain_caption` returns per word the
    (1, 196) Grad-CAM heat map of the plain decoder gradient."""
    EX_TYPE = 'GradCam'

    def grad_cam(self, img_feature, grads):
        """(1,C,h,w) features and gradients -> (h*w,) heat map, as the reference's method of the same name."""
        return _grad_cam_one(img_feature, grads).view(-1)

    def explain_cnn(self, d_img_feature):
        return self.grad_cam(self.image_features, d_img_feature).unsqueeze(0)

    def _cnn(self, d_feat, row2img):
        return self.engine.grad_cam(self._enc, d_feat, row2img)


def _grad_cam_one(img_feature, grads):
    """(1,C,h,w) features and gradients at them -> the (1, h*w) Grad-CAM heat map (:1760-1771, :1799-1810)"""
    f = ops.nchw_to_nhwc(img_feature.to(torch.float32))
    g = ops.nchw_to_nhwc(grads.to(torch.float32))
    cam = torch.empty(1, f.shape[1], device=f.device, dtype=torch.float32)
    check(_lib.load().lrpx_gradcam(ptr(f), ptr(g), ptr(None), ptr(cam), 1, f.shape[1], f.shape[2], stream_ptr()))
    return cam
