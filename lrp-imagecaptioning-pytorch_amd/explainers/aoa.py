"""Batched AoA (attention-on-attention, 8-head) LRP engine + the drop-in `ExplainAOAAttention` explainer.

Reference: models/aoamodel.py:748-1254.  Also serves the bottom-up variant (36 x 2048 region features, no CNN
stage; SURVEY §8(a) row A-BU): pass `features=` instead of images.  The encoder is VGG16 or a bottleneck ResNet.
Host logic only sequences HIP kernels."""
import ctypes as C

import numpy as np
import torch

from .. import _lib, ops
from .._lib import (AoaGradState, AoaRelState, AoaStepArgs, AoaTrace, EPI_PLAIN, EPI_REL, PACK_DENSE, PACK_DENSE_T, STAB_EPS, check, ptr, ptr_at,
                    stream_ptr)
from .dropin import ExplainerBase
from .engine_base import EngineBase, resnet_encoder_keys
from .ragged import ragged


class AOAEngine(EngineBase):
    """`state`: the reference `AOAModel` state_dict (models/aoamodel.py:116-142).  Without encoder weights
    (bottom-up model, :1795-1797) only `features=` inputs are accepted.

    The encoder (models/aoamodel.py:31-51) is chosen as `GridTDEngine`'s is (`EngineBase._init_encoder`): VGG16 from its keys, or
    `ops.ResNetEncoder` from models/resnet.py key names (`ops.bottleneck_resnet_from_state`), in encoder conv mode 1 (the exact bf16
    split).  `AOAResNetEngine` below is the same engine with the encoder handed over as a module and the mode as a parameter.
    The attention runs over any number of pixels, so a ResNet encoder takes any image size it accepts (the reference's default
    224 x 224 gives P = 49 at C = 2048); only the channel count must be `img_projector`'s (`encode` checks).  DESIGN.md 5.13."""

    _GUIDED_GRADCAM_MISSING = ("Guided Grad-CAM expands the heat map by a fixed 16 (models/aoamodel.py:1743), which is not the image at a "
                              "ResNet's stride of 32: the reference's own class fails there")
    _GRADCAM_MAX_PIXELS = 256          # lrpx_gradcam's limit on the pixels of a heat map

    def __init__(self, state, num_head=8, device="cuda"):
        self._build(state, num_head, device, None, 1)

    def _build(self, state, num_head, device, encoder, encoder_conv_mode):
        sd = self._init_encoder(state, device, encoder, encoder_conv_mode, need_encoder=False)          # (explainers/engine_base.py)
        self.sd = sd
        self.NH = num_head
        self.V, self.E = sd["embedding.weight"].shape
        self.H = sd["fc.weight"].shape[1]
        w_proj = sd["img_projector.weight"]
        self.C = w_proj.shape[1]
        H, E, Cc = self.H, self.E, self.C
        assert H == 512, "kernels are built for hidden=512 (config.py:188)"
        l = "LanguageLSTM."
        self.Wcat = torch.cat([sd[l + "weight_ih"], sd[l + "weight_hh"]], 1).contiguous()          # (4H, E+2H)
        self.bcat_explainer = (sd[l + "bias_ih"] + sd[l + "bias_ih"]).contiguous()                  # quirk :873
        self.bcat_model = (sd[l + "bias_ih"] + sd[l + "bias_hh"]).contiguous()
        # gate rows interleaved for the fused decoder step (lrpx_aoa_fwd_steps): row 16 j + 4 gate + u = row gate * H + 4 j + u, so
        # that one workgroup of the gate linear holds the i, f, g, o pre-activations of the hidden units 4j .. 4j+3
        jj, qq, uu = torch.meshgrid(torch.arange(H // 4), torch.arange(4), torch.arange(4), indexing="ij")
        il = (qq * H + 4 * jj + uu).reshape(-1).to(self.device)
        self.Wcat_il = self.Wcat[il].contiguous()
        self.bcat_model_il, self.bcat_explainer_il = self.bcat_model[il].contiguous(), self.bcat_explainer[il].contiguous()
        # the decoupled teacher-forced trace (lrpx_aoa_fwd_recurrence, include/lrpx.h): input part and recurrent part of the gate rows
        self.decoupled = H % 16 == 0 and E % 16 == 0          # False: the stepwise kernels (A/B; the decoding loops always use them)
        self.W_ih_il = self.Wcat_il[:, :E + H].contiguous()
        self.W_hh_il = self.Wcat_il[:, E + H:].contiguous()
        self.Wqg = torch.cat([sd["decoder_multihead_attention.q_proj.weight"], sd["decoder_aoa_linear_gate.weight"]], 0).contiguous()
        self.bqg = torch.cat([sd["decoder_multihead_attention.q_proj.bias"], sd["decoder_aoa_linear_gate.bias"]]).contiguous()
        self.w_proj2d = w_proj.reshape(H, Cc).contiguous()
        kc = ops.conv_kc(0, 1, Cc)
        self.p_proj_fwd = ops.pack_weights(self.w_proj2d, H, Cc, 1, PACK_DENSE, kc)
        self.p_k_fwd = ops.pack_weights(sd["decoder_k_proj.weight"], H, H, 1, PACK_DENSE, kc)
        self.p_v_fwd = ops.pack_weights(sd["decoder_v_proj.weight"], H, H, 1, PACK_DENSE, kc)
        self.p_fc_fwd = ops.pack_weights(sd["fc.weight"], self.V, H, 1, PACK_DENSE, kc)
        # fp16 split-product packs (csrc/dense_f16x3.hip): built always, USED only while ops.decoder_f16() says so (`_f16()`: conv modes 2 / 3)
        self.force_f16 = None            # True / False: this engine's decoder GEMMs on / off the fp16 split products whatever the conv mode (A/B and tests)
        self.p_fc_fwd_h = ops.pack_weights_f16x2(sd["fc.weight"], self.V, H, _lib.PACK_FWD, taps=1) if H % 64 == 0 else None
        # plain GEMMs over all (image, word) rows of the decoupled trace: (pack for the fp16 split-product kernel, fp32 pack)
        self._plain = {}
        self.tok_table = None
        if self.decoupled:
            for name, w in (("ih", self.W_ih_il), ("qg", self.Wqg), ("lin", sd["decoder_aoa_linear.weight"])):
                n, k = w.shape
                self._plain[name] = (ops.pack_weights_f16x2(w, n, k, _lib.PACK_FWD, taps=1) if k % 64 == 0 else None,
                                     ops.pack_weights(w, n, k, 1, PACK_DENSE, kc), n, k)
            # The embedding part of the gate pre-activations depends on the TOKEN alone: tok_table[v] = embedding[v] W_ie^T (V x 4H, once per
            # model, exact fp32 products on the fp32 matrix cores); the image part is one small linear per trace (W_ig, bias).  The trace then
            # needs no GEMM over its B*T rows for the LSTM input at all (lrpx_aoa_fwd_recurrence_tab).
            w_ie = self.W_ih_il[:, :E].contiguous()
            self.W_ig_il = self.W_ih_il[:, E:].contiguous()
            self.tok_table = torch.empty(self.V, 4 * H, device=self.device)
            ops.conv_mfma(sd["embedding.weight"], ops.pack_weights(w_ie, 4 * H, E, 1, PACK_DENSE, kc), self.V, 0, E, 4 * H, 1, EPI_PLAIN,
                          pix_per_map=1, oc_split=4 * H, out0=self.tok_table)
        wg = torch.cat([sd[l + "weight_ih"][2 * H:3 * H], sd[l + "weight_hh"][2 * H:3 * H]], 1).contiguous()
        self.p_wg = ops.pack_weights(wg, H, E + 2 * H, 1, PACK_DENSE_T, kc)
        self.p_lin_rel = ops.pack_weights(sd["decoder_aoa_linear.weight"], H, H, 1, PACK_DENSE_T, kc)
        self.p_v_rel = ops.pack_weights(sd["decoder_v_proj.weight"], H, H, 1, PACK_DENSE_T, kc)
        self.p_proj_rel = ops.pack_weights(self.w_proj2d, H, Cc, 1, PACK_DENSE_T, kc)
        # the v_proj / projector rules run over every (word, pixel) row: split products on the fp16 matrix cores
        # (csrc/dense_f16x3.hip)
        self.p_v_rel_h = self.p_proj_rel_h = None
        self.p_v_rel_head = None
        if H % 64 == 0:
            self.p_v_rel_h = ops.pack_weights_f16x2(sd["decoder_v_proj.weight"], H, H, _lib.PACK_BWD_PLAIN, taps=1)
            self.p_proj_rel_h = ops.pack_weights_f16x2(self.w_proj2d, H, Cc, _lib.PACK_BWD_PLAIN, taps=1)
            dk = H // self.NH
            if dk % 64 == 0:      # `lrp_mha` passes one head: the v_proj rule contracts over that head's dk rows of W_v only
                self.p_v_rel_head = [ops.pack_weights_f16x2(sd["decoder_v_proj.weight"][h * dk:(h + 1) * dk].contiguous(), dk, H,
                                                            _lib.PACK_BWD_PLAIN, taps=1) for h in range(self.NH)]
        # ... in the default (exact) arithmetic: the same tiles on the bf16 matrix cores with operands split exactly into three bf16 parts
        # (dense_f16x3.hip, B6: six products, fp32 range - what conv mode 1 is for the VGG16 chains); the fp32 MFMA where the sizes do not fit
        self.p_v_rel_6 = self.p_proj_rel_6 = self.p_v_rel_head6 = None
        if H % 32 == 0 and Cc % 4 == 0:
            self.p_v_rel_6 = ops.pack_weights_bf16x3(sd["decoder_v_proj.weight"], H, H, _lib.PACK_BWD_PLAIN, taps=1)
            self.p_proj_rel_6 = ops.pack_weights_bf16x3(self.w_proj2d, H, Cc, _lib.PACK_BWD_PLAIN, taps=1)
            dk = H // self.NH
            if dk % 32 == 0:
                self.p_v_rel_head6 = [ops.pack_weights_bf16x3(sd["decoder_v_proj.weight"][h * dk:(h + 1) * dk].contiguous(), dk, H,
                                                              _lib.PACK_BWD_PLAIN, taps=1) for h in range(self.NH)]
        self.dense_bf16x6 = True         # False: those rules on the fp32 MFMA kernel (A/B and tests)
        self.head_only = True            # (False: the v_proj rule over all H columns, 7/8 of them zero; A/B and tests)
        # ... and the lock-step gate rule / the aoa_linear rule (rows = images x words): the few-row kernel of the same file
        self.fused_steps = True          # decoder steps as 4 launches instead of 7 (False: the unfused kernels; A/B and tests)
        self.fused_rel = True            # relevance lock-steps as ONE launch each (False: GEMM + point-wise kernel; A/B and tests)
        self.fused_rel_exact = True      # ... also while the decoder GEMMs are exact (modes 0 / 1): dense_ks_kernel<REL, FUSE> (False: two launches; A/B and tests)
        self.lockstep_f16 = H % 16 == 0 and E % 16 == 0
        self.p_wg_h = ops.pack_weights_f16x2(wg, H, E + 2 * H, _lib.PACK_BWD_PLAIN, taps=1) if self.lockstep_f16 else None
        self.p_lin_rel_h = ops.pack_weights_f16x2(sd["decoder_aoa_linear.weight"], H, H, _lib.PACK_BWD_PLAIN, taps=1) if self.lockstep_f16 else None
        # gradient explainers (:1435-1499): contraction over the 4H gate rows / over the outputs of the two aoa linears
        self.p_gates_grad = ops.pack_weights(self.Wcat, 4 * H, E + 2 * H, 1, PACK_DENSE_T, kc)
        self.p_gate_grad = ops.pack_weights(sd["decoder_aoa_linear_gate.weight"], H, H, 1, PACK_DENSE_T, kc)
        torch.cuda.synchronize()
        self._idx_cache = {}

    # ------------------------------------------------------------------------------------------
    def encode(self, images=None, features=None):
        """(:999-1009) image-side constants; `features`: (B,P,C) region/pixel features instead of images."""
        H, Cc = self.H, self.C
        if features is None:
            if self.cnn is None:
                raise ValueError("this AoA model has no encoder: pass features=(B,P,C)")
            self._feature_pixels(images)          # (host arithmetic: a ResNet of another width is refused before any device work)
        lib = _lib.load()
        st = stream_ptr()
        if features is None:
            feats = self.cnn.forward(images.to(self.device, torch.float32).contiguous())
        else:
            feats = features.to(self.device, torch.float32).contiguous()
        B, P, _ = feats.shape
        e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)
        enc = dict(B=B, P=P, feats=feats)
        enc["proj_pre"] = e(B, P, H)
        ops.conv_mfma(feats, self.p_proj_fwd, B, 0, Cc, H, 1, EPI_PLAIN, pix_per_map=P, oc_split=H,
                      bias=self.sd["img_projector.bias"], out0=enc["proj_pre"])
        enc["Vp"] = e(B, P, H)
        check(lib.lrpx_relu(ptr(enc["proj_pre"]), ptr(enc["Vp"]), enc["Vp"].numel(), st))
        enc["glob"] = e(B, H)
        check(lib.lrpx_mean_pixels(ptr(enc["Vp"]), ptr(enc["glob"]), B, P, H, st))
        enc["key"], enc["value"] = e(B, P, H), e(B, P, H)
        ops.conv_mfma(enc["Vp"], self.p_k_fwd, B, 0, H, H, 1, EPI_PLAIN, pix_per_map=P, oc_split=H,
                      bias=self.sd["decoder_k_proj.bias"], out0=enc["key"])
        ops.conv_mfma(enc["Vp"], self.p_v_fwd, B, 0, H, H, 1, EPI_PLAIN, pix_per_map=P, oc_split=H,
                      bias=self.sd["decoder_v_proj.bias"], out0=enc["value"])
        return enc

    def _feature_pixels(self, images):
        """P = h w of the encoder's feature map for these images (host arithmetic).  A ResNet encoder whose feature channels are not
        `img_projector`'s input width is refused here, before any kernel runs."""
        if not self.resnet:
            return self.cnn.feat_hw[0] * self.cnn.feat_hw[1]
        if images.dim() != 4:
            raise ValueError("{}: images must be (B, 3, H, W), got {}".format(type(self).__name__, tuple(images.shape)))
        h, w, c = self.cnn.feature_shape(int(images.shape[2]), int(images.shape[3]))
        if c != self.C:
            raise ValueError("{}: the encoder gives {} feature channels; the decoder is built for {} (img_projector)".format(
                type(self).__name__, c, self.C))
        return h * w

    def _alloc_trace(self, B, T, P, grad=False):
        dev, H, E, NH = self.device, self.H, self.E, self.NH
        shapes = {"xh": (B, T, E + 2 * H), "h": (B, T + 1, H), "c": (B, T + 1, H), "alpha": (B, T, NH, P)}
        for k in ("g", "i", "f", "ctx", "lin", "c_aoa", "hc"):
            shapes[k] = (B, T, H)
        if grad:      # the gradient explainers also keep the output gate and sigmoid(aoa gate)  (:1309-1376)
            shapes["o"], shapes["sg"] = (B, T, H), (B, T, H)
        shapes["_amax"] = (3, B * T)      # row maxima (float bits) the decoupled trace records for its GEMMs' operand scales
        tr = dict(B=B, T=T, P=P)
        tr.update(ops.zeros_arena(dev, shapes))            # one allocation, one fill
        c = AoaTrace()
        c.B, c.T, c.H, c.E, c.P, c.NH = B, T, H, E, P, NH
        names = ["xh", "h", "c", "g", "i", "f", "ctx", "lin", "c_aoa", "hc", "alpha"]
        if grad:
            names += ["o", "sg"]
        for k in names:
            setattr(c, k, ptr(tr[k]))
        tr["_c"] = c
        return tr

    def _step(self, tr, enc, t, captions, bias):
        """one decoder step of `get_hidden_parameters` (models/aoamodel.py:1020-1052) for all B images"""
        lib = _lib.load()
        st = stream_ptr()
        B, T, H, E = tr["B"], tr["T"], self.H, self.E
        c = C.byref(tr["_c"])
        W = E + 2 * H
        sd = self.sd
        if "_zz" not in tr:
            tr["_zz"] = torch.empty(B, 4 * H, device=self.device)
            tr["_qg"] = torch.empty(B, 2 * H, device=self.device)
            tr["_lin"] = torch.empty(B, H, device=self.device)
        zz, qg, lin = tr["_zz"], tr["_qg"], tr["_lin"]
        check(lib.lrpx_aoa_fwd_pre(c, t, ptr(enc["glob"]), ptr(sd["embedding.weight"]), ptr(captions), captions.shape[1], st))
        check(lib.lrpx_linear_small(ptr_at(tr["xh"], t * W), T * W, ptr(self.Wcat), ptr(bias), ptr(zz), 4 * H, B, W,
                                    4 * H, 0, st))
        check(lib.lrpx_aoa_fwd_lstm(c, t, ptr(zz), 4 * H, st))
        check(lib.lrpx_linear_small(ptr_at(tr["h"], (t + 1) * H), (T + 1) * H, ptr(self.Wqg), ptr(self.bqg), ptr(qg),
                                    2 * H, B, H, 2 * H, 0, st))
        check(lib.lrpx_aoa_fwd_attention(c, t, ptr(qg), 2 * H, ptr(enc["key"]), ptr(enc["value"]), st))
        check(lib.lrpx_linear_small(ptr_at(tr["ctx"], t * H), T * H, ptr(sd["decoder_aoa_linear.weight"]),
                                    ptr(sd["decoder_aoa_linear.bias"]), ptr(lin), H, B, H, H, 0, st))
        check(lib.lrpx_aoa_fwd_post(c, t, ptr(qg), 2 * H, ptr(lin), st))

    # the decode loops of explainers/engine_base.py (beam_search, sample_lrp, forwardlrp_context) on this model's step
    _BEAM_STATE = ("h", "c")

    def _decode_trace(self, enc, B, T, lrp=False):
        return self._alloc_trace(B, T, enc["P"])

    def _decode_step(self, tr, enc, t, toks):
        self._step(tr, enc, t, toks, self.bcat_model)

    def _reweight(self, tr, t, pred, skip, hcw, log_softmax):
        """`get_lrp_weight_step` (models/aoamodel.py:597-626): `sample_lrp` hands it the log-softmax of the scores (:721-723),
        `forwardlrp_context` the raw scores"""
        B, T, H = tr["B"], tr["T"], self.H
        check(_lib.load().lrpx_lrp_reweight_rows(ptr(pred), self.V, self.V, ptr_at(tr["h"], (t + 1) * H), (T + 1) * H,
                                                 ptr_at(tr["c_aoa"], t * H), T * H, ptr(self.sd["fc.weight"]), ptr(skip),
                                                 ptr(hcw), B, H, 1 if log_softmax else 0, stream_ptr()))

    def _plain_rows(self, x, name, bias, amax=None):
        """x (R, K) @ W^T + bias -> (R, N) for one of the trace's plain linears over all (image, word) rows: split products on the
        fp16 matrix cores (as `logits(fast=True)`: <= 2e-7 of a row's maximum; operand scale per ROW), the fp32 MFMA kernel where K is
        no multiple of 64.  The kernel never depends on the number of rows: an image's TRACE is the same in every batch (the recurrence in
        slices of <= 64 images; `tests/test_gpu_aoa.py::test_trace_is_the_same_in_every_batch`: B = 1 / 64 / 65 bit for bit).  The (T,V)
        `pred` block is the exception: `logits(fast=True)` takes the fp32 kernel below 128 rows (scores equal to rounding)."""
        p_h, p_f, n, k = self._plain[name]
        if not self._f16():
            p_h = None
        R = x.shape[0]
        out = torch.empty(R, n, device=self.device)
        if p_h is not None:
            ops.conv_mfma(x, p_h, R, 0, k, -(-n // 32) * 32, 1, EPI_PLAIN, pix_per_map=1, oc_split=n, bias=bias, out0=out, f16x3=1,
                          in_amax=amax if amax is not None else ops.amax_maps(x, R))      # (amax: recorded by the kernel that wrote x)
        else:
            ops.conv_mfma(x, p_f, R, 0, k, -(-n // 32) * 32, 1, EPI_PLAIN, pix_per_map=1, oc_split=n, bias=bias, out0=out)
        return out

    def _trace_decoupled(self, tr, enc, captions, model_bias):
        """get_hidden_parameters' loop (models/aoamodel.py:1019-1052) with the recurrence decoupled (include/lrpx.h,
        lrpx_aoa_fwd_recurrence): one GEMM for the input part of all gate pre-activations, T launches of K = H for the recurrence,
        then q / gate linear, attention, decoder_aoa_linear and the gated sum once over all B*T rows."""
        lib = _lib.load()
        st = stream_ptr()
        B, T, H, E = tr["B"], tr["T"], self.H, self.E
        R = B * T
        c = C.byref(tr["_c"])
        sd = self.sd
        check(lib.lrpx_aoa_fwd_inputs(c, ptr(enc["glob"]), ptr(sd["embedding.weight"]), ptr(captions), captions.shape[1], None, st))
        bias_il = self.bcat_model_il if model_bias else self.bcat_explainer_il
        gimg = torch.empty(B, 4 * H, device=self.device)                     # glob W_ig^T + bias: the image part of every step's z
        for b0 in range(0, B, 64):          # slices of <= 64 rows: the same (MFMA) kernel whatever the batch size - an image's trace never depends on its batch
            nb = min(64, B - b0)
            check(lib.lrpx_linear_small(ptr_at(enc["glob"], b0 * H), H, ptr(self.W_ig_il), ptr(bias_il), ptr_at(gimg, b0 * 4 * H), 4 * H, nb, H, 4 * H, 0, st))
        check(lib.lrpx_aoa_fwd_recurrence_tab(c, ptr(self.W_hh_il), ptr(self.tok_table), ptr(gimg), ptr(captions), captions.shape[1], st))
        hn = torch.empty(R, H, device=self.device)
        am = tr["_amax"].view(torch.int32)                                    # [3][R] row maxima of hn / ctx / hc (ctx: zeroed with the trace)
        check(lib.lrpx_aoa_fwd_gather_h(c, ptr(hn), ptr(am[0]), st))
        qg = self._plain_rows(hn, "qg", self.bqg, amax=am[0])
        check(lib.lrpx_aoa_fwd_attention_all(c, ptr(qg), 2 * H, ptr(enc["key"]), ptr(enc["value"]), ptr(am[1]), st))
        lin = self._plain_rows(tr["ctx"].view(R, H), "lin", sd["decoder_aoa_linear.bias"], amax=am[1])
        check(lib.lrpx_aoa_fwd_post_all(c, ptr(qg), 2 * H, ptr(lin), ptr(am[2]), st))

    def trace(self, enc, captions, model_bias=False, predictions=True, grad=False):
        """grad=True: the trace of the gradient explainers (:1309-1376): correct LSTM bias, output gate and aoa gate kept."""
        model_bias = model_bias or grad
        lib = _lib.load()
        st = stream_ptr()
        B, T = captions.shape[0], captions.shape[1] - 1
        H, E = self.H, self.E
        captions = captions.to(self.device, torch.int64).contiguous()
        tr = self._alloc_trace(B, T, enc["P"], grad)
        c = C.byref(tr["_c"])
        W = E + 2 * H
        bias = self.bcat_model if model_bias else self.bcat_explainer
        sd = self.sd
        if self.decoupled and T > 0:          # (any B: the recurrence runs in slices of <= 64 images inside the library)
            self._trace_decoupled(tr, enc, captions, model_bias)
            tr["captions"] = captions
            tr["logit"] = torch.empty(B * T, device=self.device)
            check(lib.lrpx_target_logit(ptr(tr["hc"]), ptr(sd["fc.weight"]), ptr(sd["fc.bias"]), ptr(captions), T + 1,
                                        ptr(tr["logit"]), B, T, H, st))
            if predictions:
                tr["pred"] = self.logits(tr["hc"].view(B * T, H), fast=True, amax=tr["_amax"].view(torch.int32)[2]).view(B, T, self.V)
            return tr
        # the T decoder steps (:1019-1052) in one native call (the host loop of `_step` in C: the bottom-up path is bound by the
        # launch rate of the interpreter otherwise)
        tr["_zz"], tr["_qg"], tr["_lin"] = (torch.empty(B, n * H, device=self.device) for n in (4, 2, 1))
        sa = AoaStepArgs()
        sa.glob, sa.emb, sa.tok, sa.tok_ld = ptr(enc["glob"]), ptr(sd["embedding.weight"]), ptr(captions), captions.shape[1]
        sa.w_cat, sa.b_cat, sa.w_qg, sa.b_qg = ptr(self.Wcat), ptr(bias), ptr(self.Wqg), ptr(self.bqg)
        if self.fused_steps:
            sa.w_cat_il, sa.b_cat_il = ptr(self.Wcat_il), ptr(self.bcat_model_il if model_bias else self.bcat_explainer_il)
        sa.w_lin, sa.b_lin = ptr(sd["decoder_aoa_linear.weight"]), ptr(sd["decoder_aoa_linear.bias"])
        sa.key, sa.value, sa.zz, sa.qg, sa.lin = ptr(enc["key"]), ptr(enc["value"]), ptr(tr["_zz"]), ptr(tr["_qg"]), ptr(tr["_lin"])
        check(lib.lrpx_aoa_fwd_steps(c, 0, T, C.byref(sa), st))
        tr["captions"] = captions
        tr["logit"] = torch.empty(B * T, device=self.device)
        check(lib.lrpx_target_logit(ptr(tr["hc"]), ptr(sd["fc.weight"]), ptr(sd["fc.bias"]), ptr(captions), T + 1,
                                    ptr(tr["logit"]), B, T, H, st))
        if predictions:
            tr["pred"] = self.logits(tr["hc"].view(B * T, H), fast=True).view(B, T, self.V)
        return tr

    def gradient(self, enc, tr, head_idx, lens=None):
        """`ExplainAOAGradient.explain_caption_wordt` (models/aoamodel.py:1435-1499; the guided and Grad-CAM classes
        inherit it unchanged) for every (image, word) row in lock-step.  `tr` must be a grad=True trace.
        Returns d_feat (B*T, P, C), r_words (B*T, T), row2img.  With `lens` (explainers/ragged.py) d_feat holds the valid
        (image, word) rows only, compact, with the matching row -> image table."""
        lib = _lib.load()
        st = stream_ptr()
        B, T, H, E, P, Cc = tr["B"], tr["T"], self.H, self.E, tr["P"], self.C
        rows = B * T
        rg = ragged(lens, B, T, self.device)
        lens = rg.lens if rg is not None else None
        e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)
        gs = dict(d_h=e(rows, H), d_c=e(rows, H), dA=e(rows, H), dB=e(rows, H), gates=e(rows, 4 * H),
                  dx=e(rows, E + 2 * H), d_glob=e(rows, H), r_words=e(rows, T))
        c = AoaGradState()
        c.lens = ptr(lens)
        for k, v in gs.items():
            setattr(c, k, ptr(v))
        ctr, cgs = C.byref(tr["_c"]), C.byref(c)
        _, row2img, _ = self._row_index(B, T)
        check(lib.lrpx_aoa_grad_init(ctr, cgs, ptr(self.sd["fc.weight"]), ptr(tr["captions"]), T + 1, st))

        def dense(a, wp, n):      # (rows, K) @ packed (K, n) -> (rows, n), fp32 MFMA
            out = e(rows, n)
            ops.conv_mfma(a, wp, rows, 0, a.shape[1], -(-n // 32) * 32, 1, EPI_PLAIN, pix_per_map=1, oc_split=n, out0=out)
            return out
        d_ctx = dense(gs["dA"], self.p_lin_rel, H)                                   # :1469  d_A @ W_aoa_linear
        t1 = dense(gs["dB"], self.p_gate_grad, H)                                    # :1470  d_B @ W_aoa_linear_gate
        check(lib.lrpx_accumulate(ptr(gs["d_h"]), ptr(t1), rows * H, st))
        dk = H // self.NH
        check(lib.lrpx_keep_cols(ptr(d_ctx), rows, H, head_idx * dk, (head_idx + 1) * dk, st))   # gradient_mha :1428
        for s in range(T):
            check(lib.lrpx_aoa_grad_step(ctr, cgs, s, 0, st))
            ops.conv_mfma(gs["gates"], self.p_gates_grad, rows, 0, 4 * H, E + 2 * H, 1, EPI_PLAIN, pix_per_map=1,
                          oc_split=E + 2 * H, out0=gs["dx"])
            check(lib.lrpx_aoa_grad_step(ctr, cgs, s, 1, st))
        # pixels: d_value = alpha (x) d_ctx[head]; through v_proj and the projector both stay rank-1 in the pixel index
        u = dense(d_ctx, self.p_v_rel, H)                                            # :1489  d_value @ W_v
        v1 = dense(u, self.p_proj_rel, Cc)                                           # :1492
        v2 = dense(gs["d_glob"], self.p_proj_rel, Cc)
        check(lib.lrpx_scale(ptr(v2), ptr(v2), v2.numel(), 1.0 / P, st))             # :1491  d_glob / P
        check(lib.lrpx_rel_words_norm(ptr(gs["r_words"]), rows, T, st))
        n, rowlist = rows, None
        if rg is not None and not rg.full:
            n, rowlist, row2img = rg.n, rg.rows, rg.row2img
        d_feat = e(n, P, Cc)
        if n:
            check(lib.lrpx_aoa_grad_pix_rows(ctr, head_idx, ptr(v1), ptr(v2), ptr(d_feat), Cc, ptr(rowlist), n, st))
        return d_feat, gs["r_words"], row2img

    def explain_batch_gradient(self, captions, head_idx, images, kind="gradient", lens=None, return_features=False):
        """Batched `explain_caption` of ExplainAOAGradient (kind="gradient", :1501-1534), ExplainAOAGuidedGradient
        ("guided", :1621-1640), ExplainAOAGradCam ("gradcam", :1669-1689; result (B,T,P) heat maps) and
        ExplainAOAGuidedGradCam ("guided_gradcam", :1714-1751; VGG16 only).  With a ResNet encoder the maps are
        `ResNetEncoder.gradient` / `.guided_backprop(relus="stem")` (the reference hooks the encoder's direct children, :1596-1613: the
        stem's ReLU alone) at the images' own size."""
        self._preset_only("explain_batch_gradient", self._NO_GRAD_AB)
        if kind == "guided_gradcam":
            self._refuse_resnet("explain_batch_gradient(kind='guided_gradcam')", self._GUIDED_GRADCAM_MISSING)
        if kind == "gradcam" and self.cnn is not None and self._feature_pixels(images) > self._GRADCAM_MAX_PIXELS:           # before any launch
            raise ValueError("{}: a feature map of {} pixels; Grad-CAM heat maps are built for at most {} (lrpx_gradcam)".format(
                type(self).__name__, self._feature_pixels(images), self._GRADCAM_MAX_PIXELS))
        enc = self.encode(images)
        captions = captions.to(self.device, torch.int64).contiguous()
        B, T = captions.shape[0], captions.shape[1] - 1
        tr = self.trace(enc, captions, predictions=False, grad=True)
        rg = ragged(lens, B, T, self.device)
        d_feat, r_words, row2img = self.gradient(enc, tr, head_idx, rg)
        P = enc["P"]

        def maps_of(d_feat, row2img):
            if kind == "gradcam":
                return self.grad_cam(enc, d_feat, row2img)
            if kind not in ("guided", "guided_gradcam"):
                return self.cnn.gradient(d_feat, row2img)
            maps = self._guided_backprop(d_feat, row2img)
            if kind == "guided_gradcam":         # ExplainAOAGuidedGradCam (:1714-1751): x the expanded Grad-CAM map
                maps = ops.guided_gradcam(maps, self.grad_cam(enc, d_feat, row2img), int(round(P ** 0.5)))
            return maps
        return self._finish(rg, B, T, d_feat, r_words, row2img, maps_of, (P,) if kind == "gradcam" else tuple(images.shape[1:]),
                            features=(tr, enc) if return_features else None)

    def _guided_backprop(self, d_feat, row2img):
        if self.resnet:
            return self.cnn.guided_backprop(d_feat, row2img, relus="stem")
        return self.cnn.guided_backprop(d_feat, row2img)

    def relevance(self, enc, tr, head_idx, lens=None, compact=True):
        """explain_caption_wordt (:1064-1156) for every (image, word) row -> r_feat (B*T,P,C), r_words (B*T,T), row -> image.
        lens (one caption length per image; explainers/ragged.py): padded words are skipped by the lock-step kernels and, with
        compact=True (the image path: the rows feed the VGG16 chain), the (word, pixel) rules run on the valid rows only:
        r_feat is then (sum(lens), P, C) with the matching row -> image table."""
        lib = _lib.load()
        st = stream_ptr()
        B, T, P, H, E, Cc = tr["B"], tr["T"], tr["P"], self.H, self.E, self.C
        rows = B * T
        rg = ragged(lens, B, T, self.device)
        lens = rg.lens if rg is not None else None
        e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)
        rs = dict(r_hn=e(rows, H), r_glob=e(rows, H), A=e(rows, H), rx=e(rows, E + 2 * H), r_words=e(rows, T))
        c = AoaRelState()
        c.lens = ptr(lens)
        for k, v in rs.items():
            setattr(c, k, ptr(v))
        ctr, crs = C.byref(tr["_c"]), C.byref(c)
        idx, row2img, rowid = self._row_index(B, T)
        check(lib.lrpx_aoa_rel_init(ctr, crs, ptr(self.sd["fc.weight"]), ptr(tr["logit"]), ptr(tr["captions"]), T + 1, st))
        # decoder_aoa_linear dense rule (:1107-1110): r_ctx = ctx * (W^T (r_caoa / z~(lin)))
        r_ctx = e(rows, H)
        f16 = 1 if (self.lockstep_f16 and self._f16()) else 0
        ops.conv_mfma(rs["A"], self.p_lin_rel_h if f16 else self.p_lin_rel, rows, 0, H, H, 1, EPI_REL, pix_per_map=1, oc_split=H,
                      x=tr["ctx"], map2img=rowid, out0=r_ctx, f16x3=f16)
        W = E + 2 * H
        # the lock-steps s = 0..T-1 (:1114-1134) in one native call: phase 0, the LSTM dense rule with map2img = idx[s], phase 1
        dense = ops.conv_desc(rs["A"], self.p_wg_h if f16 else self.p_wg, rows, 0, H, W, 1, EPI_REL, pix_per_map=1, oc_split=W,
                              x=tr["xh"], map2img=idx[0], out0=rs["rx"], f16x3=f16)
        fused = self.fused_rel and E == H == 512 and (f16 or self.fused_rel_exact)     # (exact modes: the same fusion in the fp32 K-split kernel, csrc/dense_small.hip)
        if fused:      # one launch per lock-step: the step's point-wise code in the GEMM's epilogue (lrpx_aoa_rel_steps_fused)
            a_alt, wpart, coef = e(rows, H), e(rows, T, 4), e(2 * rows * H + rows)
            check(lib.lrpx_aoa_rel_steps_fused(ctr, crs, C.byref(dense), ptr(idx), idx.shape[1], ptr(a_alt), ptr(wpart), ptr(coef), st))
        else:
            check(lib.lrpx_aoa_rel_steps(ctr, crs, T, C.byref(dense), ptr(idx), idx.shape[1], st))
        # :1136-1144  r_proj = eye rule on the mean (U) + v_proj dense rule; fused division for the projector rule
        U = e(rows, H)
        check(lib.lrpx_rel_avg_u(ptr(rs["r_glob"]), ptr(enc["glob"]), ptr(U), rows, T, H, P, st))
        if not fused:
            check(lib.lrpx_rel_words_norm(ptr(rs["r_words"]), rows, T, st))
        n, rowlist = rows, None
        if rg is not None and not rg.full and compact:     # unequal lengths: the (word, pixel) rules on the valid rows only
            n, rowlist, row2img = rg.n, rg.rows, rg.row2img
            if n == 0:
                return e(0, P, Cc), rs["r_words"], row2img
            U = ops.gather_rows(U, rowlist)
        a_proj = e(n, P, H)
        r_feat = e(n, P, Cc)
        f16_rules = self.p_v_rel_h is not None and P >= 32 and self._f16()
        b6_rules = not f16_rules and self.p_v_rel_6 is not None and self.dense_bf16x6           # (any P: a row's kernel never depends on the batch)
        head_only = self.head_only and ((f16_rules and self.p_v_rel_head is not None) or (b6_rules and self.p_v_rel_head6 is not None))
        if head_only:
            dk = H // self.NH
            a_val = e(n, P, dk)
            check(lib.lrpx_aoa_rel_value_head(ctr, crs, ptr(r_ctx), ptr(enc["value"]), int(head_idx), ptr(a_val), ptr(rowlist), n, st))
        else:
            a_val = e(n, P, H)
            check(lib.lrpx_aoa_rel_value_rows(ctr, crs, ptr(r_ctx), ptr(enc["value"]), int(head_idx), ptr(a_val), ptr(rowlist), n, st))
        amax2 = None
        if f16_rules:
            amax2 = ops.zeros(n, dtype=torch.int32, device=self.device)           # max|a_proj| per row: recorded by the first GEMM
            ops.conv_mfma(a_val, self.p_v_rel_head[int(head_idx)] if head_only else self.p_v_rel_h, n, 0, dk if head_only else H, H, 1,
                          EPI_REL, pix_per_map=P, oc_split=H, x=enc["Vp"], u=U,
                          zdiv=enc["proj_pre"], stab=STAB_EPS, map2img=row2img, out1=a_proj, f16x3=1,
                          in_amax=ops.amax_maps(a_val, n), out1_amax=amax2)
        elif b6_rules:
            ops.conv_mfma(a_val, self.p_v_rel_head6[int(head_idx)] if head_only else self.p_v_rel_6, n, 0, dk if head_only else H, H, 1,
                          EPI_REL, pix_per_map=P, oc_split=H, x=enc["Vp"], u=U, zdiv=enc["proj_pre"], stab=STAB_EPS, map2img=row2img,
                          out1=a_proj, bf16x6=1)
        else:
            ops.conv_mfma(a_val, self.p_v_rel, n, 0, H, H, 1, EPI_REL, pix_per_map=P, oc_split=H, x=enc["Vp"], u=U,
                          zdiv=enc["proj_pre"], stab=STAB_EPS, map2img=row2img, out1=a_proj)
        # :1145-1148, in the arithmetic of the v_proj rule
        self._proj_rule(a_proj, n, P, enc["feats"], row2img, r_feat, kind="f16" if f16_rules else "b6" if b6_rules else "f32", in_amax=amax2)
        return r_feat, rs["r_words"], row2img

    def explain_batch(self, captions, head_idx, images=None, features=None, lens=None, accumulate=False,
                      return_features=False, predictions=False):
        """Batched `explain_caption(img, head_idx)` (:1165-1181).  With images: maps (B,T,3,H,W), 224 x 224 for VGG16; with
        `features` (bottom-up): the region-feature relevance (B,T,P,C) is the result (no CNN stage).
        predictions=True keeps the (T,V) scores of the trace as the reference's explainer does (:1026).  The instance attribute
        `lrp_params` selects the encoder's Conv2d rule on the images path (explainers/engine_base.py: `_maps_stage`); with `features`
        there is no encoder stage and anything but None is a ValueError."""
        maps_of = self._features_stage("explain_batch") if features is not None else self._maps_stage("explain_batch")
        enc = self.encode(images, features)
        captions = captions.to(self.device, torch.int64).contiguous()
        B, T = captions.shape[0], captions.shape[1] - 1
        tr = self.trace(enc, captions, predictions=predictions)
        rg = ragged(lens, B, T, self.device)
        if features is not None:         # bottom-up: the region relevance IS the result; rows behind an image's last word are zero
            r_feat, r_words, _ = self.relevance(enc, tr, head_idx, rg, compact=False)
            return r_feat.view(B, T, enc["P"], self.C), r_words.view(B, T, T)
        r_feat, r_words, row2img = self.relevance(enc, tr, head_idx, rg)
        # unequal caption lengths (models/aoamodel.py:1171-1176 explains `caption_length` words): the VGG16 chain runs on the sum(lens)
        # valid maps; `_finish` takes the result back to the padded layout
        return self._finish(rg, B, T, r_feat, r_words, row2img, maps_of, tuple(images.shape[1:]), accumulate=accumulate,
                            features=(tr, enc) if return_features else None)

    def _static(self, graph, key, captions, head_idx, images, features, accumulate, predictions):
        name, src = ("features", features) if features is not None else ("images", images)
        return self._static_step(graph, key, src.to(self.device, torch.float32), captions.to(self.device, torch.int64),
                                 lambda s, c: self.explain_batch(c, head_idx, accumulate=accumulate, predictions=predictions, **{name: s}))

    def explain_batch_graph(self, captions, head_idx, images=None, features=None, accumulate=False, predictions=False):
        """`explain_batch` replayed from a captured HIP graph, one per input shape and head (explainers/engine_base.py: `_static_step`)."""
        self._features_stage("explain_batch_graph") if features is not None else self._preset_only("explain_batch_graph", self._NO_STATIC_AB)
        if features is None:
            self._refuse_resnet("explain_batch_graph", self._NO_GRAPH)
        src = features if features is not None else images
        key = (features is not None, tuple(src.shape), tuple(captions.shape), int(head_idx), bool(accumulate), bool(predictions), self._f16())
        return self._static(True, key, captions, head_idx, images, features, accumulate, predictions)

    def explain_batch_replay(self, captions, head_idx, images=None, features=None, accumulate=False, predictions=False):
        """`explain_batch` as a RECORDED step, one per input shape, head and stream (explainers/engine_base.py: `_static_step`)."""
        self._features_stage("explain_batch_replay") if features is not None else self._preset_only("explain_batch_replay", self._NO_STATIC_AB)
        if features is None:
            self._refuse_resnet("explain_batch_replay", self._NO_RECORDING)
        src = features if features is not None else images
        key = (tuple(src.shape), tuple(captions.shape), bool(accumulate), bool(predictions), _lib.stream_ptr().value,
               self.vgg.conv_mode if self.vgg is not None else None, int(head_idx), features is not None, self._f16())
        return self._static(False, key, captions, head_idx, images, features, accumulate, predictions)

    def explain_stream(self, batches, head_idx, depth=3, accumulate=False):
        """`explain_batch` over an iterable of (images, captions[, lens]) batches, `depth` in flight (explainers/engine_base.py)."""
        self._maps_stage("explain_stream")                # a refusal here, not inside the generator's first step
        return self._explain_stream(batches, depth, lambda eng, images, captions, lens: eng.explain_batch(
            captions, head_idx, images=images, lens=lens, accumulate=accumulate))


class AOAResNetEngine(AOAEngine):
    """`AOAEngine` with the encoder's two parameters of `GridTDEngine`: `encoder`, an nn.Module on the GPU that
    `ops.match_bottleneck_resnet` accepts (the model's own `img_encoder.encoder`; None: built from the state dict as `AOAEngine` does),
    and `encoder_conv_mode`, the ResNet encoder engine's arithmetic (0: fp32 MFMA, 1: the exact bf16 split).  A mode outside {0, 1}, a
    module that is not on the GPU and a BasicBlock / dilated / grouped net are refused before any device work.  (`AOAEngine` keeps the
    constructor it has always had; everything else is inherited.)"""

    def __init__(self, state, num_head=8, device="cuda", encoder=None, encoder_conv_mode=1):
        self._build(state, num_head, device, encoder, encoder_conv_mode)


class ExplainAOAAttention(ExplainerBase):
    """Drop-in for the reference's `ExplainAOAAttention` (models/aoamodel.py:748-1194), called as evaluation.py:637,702,767 call
    it: `explain_caption(img_filepath, head_idx)`, `explain_caption_wordt(t, head_idx)`, `explain_cnn(R)`,
    `explain_caption_words(img_filepath)`, `teacherforce_forward(img, beam_caption_encode)`, `get_hidden_parameters(img_filepath)`,
    `preprocess_img(img_filepath)`; attributes `.model .word_map .img .img_filepath .beam_caption .beam_caption_encode .predictions
    .alphas .args`.  Conventions: explainers/dropin.py; the caption the reference explains is its beam search with beam 3 over 20
    steps (:992).

    ResNet encoders (`args.encoder` 'resnet101' / 'renset50', models/aoamodel.py:34-39): an `AOAModel` hands over its
    `model.img_encoder.encoder` (used as it is when it lives on the GPU, rebuilt from the state dict otherwise); a state dict or
    `args.weight` with models/resnet.py key names is built by `ops.bottleneck_resnet_from_state`.  `args.height` / `args.width` size the
    images (any size the encoder accepts: the attention takes any number of pixels); `args.encoder_conv_mode` (optional, default 1)
    is the engine's.  The gradient-family subclasses run on such a model too, except `ExplainAOAGuidedGradCam` (NotImplementedError:
    the reference's own class fails at a stride of 32)."""

    _REFUSES_RESNET = False      # (True: Guided Grad-CAM, VGG16 only)

    def __init__(self, args, word_map, model=None):
        self.num_head = getattr(args, "num_head", 8)
        super().__init__(args, word_map, model)

    def _engine_key(self):
        from . import engine_cache
        extra = (self.num_head,)
        if self.model is None:
            resnet = getattr(self.args, "encoder", "vgg16") != "vgg16"            # ('resnet101' / 'renset50', models/aoamodel.py:34-39)
        else:
            resnet = resnet_encoder_keys(self.model.state_dict() if hasattr(self.model, "state_dict") else self.model)
        if resnet:                                                                # a ResNet engine is built in ITS conv mode
            extra += (("resnet", getattr(self.args, "encoder_conv_mode", 1)),)
        return engine_cache.fingerprint("aoa", self.args.weight if self.model is None else self.model, extra)

    def _refuse_resnet(self):
        raise NotImplementedError("{}: not built for a ResNet encoder - {}".format(type(self).__name__, AOAEngine._GUIDED_GRADCAM_MISSING))

    def _build_engine(self, state):
        encoder = None
        if hasattr(self.model, "state_dict"):
            enc = getattr(getattr(self.model, "img_encoder", None), "encoder", None)
            if resnet_encoder_keys(state) and isinstance(enc, torch.nn.Module) and all(
                    t.device.type == "cuda" for t in list(enc.parameters()) + list(enc.buffers())):
                encoder = enc                  # the model's own module (else: rebuilt from the same tensors by the engine)
        if self._REFUSES_RESNET and resnet_encoder_keys(state):
            self._refuse_resnet()              # before anything is uploaded
        if not resnet_encoder_keys(state):
            return AOAEngine(state, self.num_head)
        return AOAResNetEngine(state, self.num_head, encoder=encoder, encoder_conv_mode=getattr(self.args, "encoder_conv_mode", 1))

    def _accept_engine(self, engine):
        if self._REFUSES_RESNET and engine.resnet:
            self._refuse_resnet()

    def get_hidden_parameters(self, img, caption_encode=None):
        """Forward trace (:990-1062).  `img`: file path (the reference's argument) or a (1,3,H,W) tensor of the encoder's image size
        (224 x 224 for VGG16; `args.height` / `args.width` size a file's image)."""
        self._hidden_parameters(img, caption_encode, 3, 20)

    def _explain_rows(self, head_idx):
        return self.engine.relevance(self._enc, self._tr, head_idx)

    def explain_caption_wordt(self, t, head_idx):
        return self._explain_wordt(t, head_idx)

    def explain_caption(self, img_filepath, head_idx, t_list=None, caption_encode=None):
        """(:1165-1181; gradient family :1517-1534) -> ([T] x maps, [T] x (t+1,)).  The LRP maps are the reference's running sums
        (lrp_wrapper.py:64-82); the gradient family's image gradient is a fresh tensor per word."""
        return self._explain_caption(img_filepath, caption_encode, head_idx)

    def explain_caption_words(self, img_filepath, caption_encode=None):
        """(:1183-1194) linguistic relevance only, head 0."""
        self.img_filepath = img_filepath
        self.get_hidden_parameters(img_filepath, caption_encode)
        if self.caption_length == 0:
            return []
        _, r_words, _ = self._relevance(0)
        return [r_words[t, :t + 1] for t in range(self.caption_length)]


class ExplainAOAGradient(ExplainAOAAttention):
    """Drop-in for the reference's `ExplainAOAGradient` (models/aoamodel.py:1257-1592): hand-written BPTT through the
    language LSTM for one attention head (`explain_caption_wordt`, :1435-1499) and the autograd gradient through the
    encoder (`explain_cnn`, :1501-1515).  Same surface: `explain_caption(img, head_idx) -> (maps, word scores)`."""
    EX_TYPE = 'gradient'
    TF_MODEL_BIAS = True
    _RUNNING_SUMS = False

    def get_hidden_parameters(self, img, caption_encode=None):
        super().get_hidden_parameters(img, caption_encode)
        if self.caption_length:
            self._trace(grad=True)             # :1309-1376 (correct LSTM bias)

    def _explain_rows(self, head_idx):
        return self.engine.gradient(self._enc, self._tr, head_idx)

    def _cnn(self, d_feat_nhwc, row2img):
        return self.engine.cnn.gradient(d_feat_nhwc, row2img)

    def explain_cnn(self, d_img_feature):          # (the reference's argument name in this family)
        return super().explain_cnn(d_img_feature)


class ExplainAOAGuidedGradient(ExplainAOAGradient):
    """Drop-in for `ExplainAOAGuidedGradient` (models/aoamodel.py:1594-1667): same decoder gradient, guided backprop
    through the encoder (:1621-1640)."""
    EX_TYPE = 'GuidedBackpropagate'

    def _cnn(self, d_feat_nhwc, row2img):
        return self.engine._guided_backprop(d_feat_nhwc, row2img)


class ExplainAOAGuidedGradCam(ExplainAOAGuidedGradient):
    """Drop-in for `ExplainAOAGuidedGradCam` (models/aoamodel.py:1714-1751): the guided-backprop map of every word times
    the Grad-CAM heat map of the same decoder gradient, expanded 16x by `skimage.transform.pyramid_expand` (:1741; here
    one matrix product per axis, ops.pyramid_expand_matrix)."""
    EX_TYPE = 'GuidedGradCam'
    _REFUSES_RESNET = True

    def _cnn(self, d_feat_nhwc, row2img):
        guided = self.engine.vgg.guided_backprop(d_feat_nhwc, row2img)
        return ops.guided_gradcam(guided, self.engine.grad_cam(self._enc, d_feat_nhwc, row2img), int(round(d_feat_nhwc.shape[1] ** 0.5)))


class ExplainAOAGradCam(ExplainAOAGradient):
    """Drop-in for `ExplainAOAGradCam` (models/aoamodel.py:1669-1711): per word the (1, h*w) Grad-CAM heat map."""
    EX_TYPE = 'GradCam'

    def _cnn(self, d_feat_nhwc, row2img):
        return self.engine.grad_cam(self._enc, d_feat_nhwc, row2img)
