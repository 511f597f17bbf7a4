"""The gradient family of the single-LSTM adaptive-attention model: `AdaAttGradEngine` + the drop-ins `ExplainAdaptiveGradient`,
`ExplainiAdaptiveGuidedGradient` (the spelling is the reference's), `ExplainAdaptiveGradCam`, and `ExplainAdaptiveGuidedGradCam`, which
refuses.

Reference: models/adaptiveattention.py:851-1320.  Kernels: csrc/lrpx_adaatt_grad.hip behind the `lrpx_adaptive_grad_*` entries of the C
ABI; DESIGN.md 5.16.  The decoder back-pass (`explain_caption_wordt`, :965-1021) is a hand-derived partial gradient in which alpha, beta
and the sentinel gate are constants; three facts about it shape this module:

  1. the decoder part of the guided class (:1100-1157) is the same function: its mask :1130 tests ReLU outputs for < 0 and its mask :1148
     comes after `d_average_img_feature` has been formed - neither selects anything.  The two classes differ in `explain_cnn` only;
  2. only d_h = G_i W_hh is serial.  r_words[i] = G_i . wsum with wsum[k] = sum_{e < E} W_ih[k, e], d_glob = (sum_i G_i) W_ih[:, E:], and the
     pixel term alpha_t[k] (d_ctx W_proj) is rank-1 in the pixel index: one launch per lock-step and three GEMMs behind the loop;
  3. `ExplainAdaptiveGuidedGradCam` expands the heat map by 32 (:1289), which is the image only for a stride-32 encoder at 448 x 448
     (the model fixes P = 196, :118): refused.

The host logic below only sequences kernel launches; torch is used for device memory."""
import ctypes as C

import torch

from .. import _lib, ops
from .._lib import EPI_PLAIN, AdaGradState, PACK_DENSE_T, check, ptr, stream_ptr
from .adaatt import AdaAttEngine, ExplainAdaptiveAttention
from .ragged import ragged

GUIDED_GRADCAM_MISSING = ("ExplainAdaptiveGuidedGradCam expands the Grad-CAM heat map by a fixed factor of 32 "
                          "(models/adaptiveattention.py:1289): on VGG16's 14 x 14 map that is 448 against a 224 x 224 image, so the reference's "
                          "own class cannot run there; it fits a stride-32 encoder at 448 x 448 only, and that expansion is missing here")
GRADCAM_MAX_PIXELS = 256          # lrpx_gradcam's limit on the pixels of a heat map


class AdaAttGradEngine(AdaAttEngine):
    """`AdaAttEngine` + the gradient, guided-backprop and Grad-CAM explainers (`AdaAttEngine` itself keeps refusing them: the LRP engine
    carries none of the weights below).  Same constructor.  Added per engine, once: `w_hh_t` (H, 4H), the transposed copy of W_hh the
    lock-step kernel streams; `wsum` (4H,), the row sums of the embedding half of W_ih, formed in fp64 and rounded once; the packed glob
    half of W_ih."""

    def __init__(self, state, device="cuda", encoder=None, encoder_conv_mode=1):
        super().__init__(state, device=device, encoder=encoder, encoder_conv_mode=encoder_conv_mode)
        H, E, sd = self.H, self.E, self.sd
        w_ih, w_hh = sd["AdaLSTM.lstm_cell.weight_ih"], sd["AdaLSTM.lstm_cell.weight_hh"]
        self.w_hh_t = w_hh.t().contiguous()                                                  # row j = column j of W_hh (:1007)
        self.wsum = w_ih[:, :E].double().sum(1).float().contiguous()                         # :1008, :1010, :1016
        self.p_ih_glob = ops.pack_weights(w_ih[:, E:].contiguous(), 4 * H, E, 1, PACK_DENSE_T, ops.conv_kc(0, 1, 4 * H))     # :1008-1009
        torch.cuda.synchronize()

    # ------------------------------------------------------------------------------------------
    def trace(self, enc, captions, model_bias=True, predictions=True, grad=False):
        """`AdaAttEngine.trace`; grad=True: the same trace with the output gate `o` and the sentinel gate `sgate` kept
        (get_hidden_parameters of the gradient classes, :900-963: the LSTM bias is bias_ih + bias_hh in both, :883).  Both `decoupled`
        settings fill them."""
        return self._teacher_forced(enc, captions, predictions, bool(grad))

    def guided_gradient(self, enc, tr, lens=None, mask_features=True):
        """`explain_caption_wordt` of the gradient classes (:965-1021, :1100-1157) for every (image, word) row in lock-step.  `tr` must be
        a grad=True trace.  Returns d_feat (B*T, P, C), r_words (B*T, T), row2img.  With `lens` (explainers/ragged.py) d_feat holds the
        valid (image, word) rows only, compact, with the matching row -> image table.
        `mask_features` is accepted for the surface this entry shares with `GridTDEngine.guided_gradient` and changes nothing in this
        model: the guided class's feature mask (:1130) tests the ReLU outputs `image_feature_proj` for < 0 and its second mask (:1148)
        comes after the value it would have changed was used - the reference's two decoder functions return identical tensors.
        The state tensors of the last call stay in `self.last_grad` (d_ctx, gsum, d_glob, ...: what the tests read)."""
        if "o" not in tr or "sgate" not in tr:
            raise ValueError("{}.guided_gradient: the trace has no output gate / sentinel gate - take it with trace(..., grad=True)".format(
                type(self).__name__))
        lib, st = _lib.load(), stream_ptr()
        B, T, H, E, P, Cc = tr["B"], tr["T"], self.H, self.E, self.P, self.C
        rows, dev = B * T, self.device
        rg = ragged(lens, B, T, dev)
        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        gs = dict(d_ctx=e(rows, H), d_c=e(rows, H), g0=e(rows, 4 * H), g1=e(rows, 4 * H), gsum=e(rows, 4 * H), wpart=e(rows, T, H // 16),
                  r_words=e(rows, T))
        c = AdaGradState()
        c.lens = ptr(rg.lens) if rg is not None else None
        for k, v in gs.items():
            setattr(c, k, ptr(v))
        ctr, cgs = C.byref(tr["_c"]), C.byref(c)
        _, row2img, _ = self._row_index(B, T)
        check(lib.lrpx_adaptive_grad_init(ctr, cgs, ptr(self.sd["fc.weight"]), ptr(tr["captions"]), T + 1, ptr(self.wsum), st))
        check(lib.lrpx_adaptive_grad_steps(ctr, cgs, T, ptr(self.w_hh_t), ptr(self.wsum), st))      # lock-steps 1 .. T-1, then r_words
        check(lib.lrpx_rel_words_norm(ptr(gs["r_words"]), rows, T, st))                                # :1016-1019

        def dense(a, wp, n):      # (rows, K) @ packed (K, n) -> (rows, n), fp32 MFMA
            out = e(rows, n)
            ops.conv_mfma(a, wp, rows, 0, a.shape[1], -(-n // 32) * 32, 1, EPI_PLAIN, pix_per_map=1, oc_split=n, out0=out)
            return out
        gs["d_glob"] = dense(gs["gsum"], self.p_ih_glob, E)                                            # :1008-1009 out of the loop
        gs["d_avg"] = dense(gs["d_glob"], self.p_gp_rel, Cc)                                           # :1011
        gs["v1"] = dense(gs["d_ctx"], self.p_proj_rel, Cc)                                             # :1015 out of the pixel loop
        self.last_grad = gs
        n, rowlist = rows, None
        if rg is not None and not rg.full:
            n, rowlist, row2img = rg.n, rg.rows, rg.row2img
        d_feat = e(n, P, Cc)
        if n:
            check(lib.lrpx_adaptive_grad_pix_rows(ctr, cgs, ptr(gs["v1"]), ptr(gs["d_avg"]), ptr(d_feat), Cc, ptr(rowlist), n, st))
        return d_feat, gs["r_words"], row2img

    def _guided_backprop(self, d_feat, row2img):
        if self.resnet:      # the reference hooks the encoder's direct children (:1169-1173): the stem's ReLU alone
            return self.cnn.guided_backprop(d_feat, row2img, relus="stem")
        return self.cnn.guided_backprop(d_feat, row2img)

    def _decoder_gradient(self, enc, captions, lens):
        captions = captions.to(self.device, torch.int64).contiguous()
        B, T = captions.shape[0], captions.shape[1] - 1
        tr = self.trace(enc, captions, predictions=False, grad=True)
        rg = ragged(lens, B, T, self.device)
        d_feat, r_words, row2img = self.guided_gradient(enc, tr, rg)
        return B, T, tr, rg, d_feat, r_words, row2img

    def explain_batch_gradient(self, images, captions, lens=None, cam=False, return_features=False):
        """Batched `ExplainAdaptiveGradient.explain_caption` (:1038-1052): the decoder gradient + the gradient through the encoder
        (`explain_cnn`, :1023-1036) -> maps (B,T,3,H,W), word scores (B,T,T).  cam=True: `ExplainAdaptiveGradCam` (:1218-1236) - the
        per-word result is the Grad-CAM heat map (B,T,P).  (No running sums: the reference takes a fresh gradient per word.)"""
        self._preset_only("explain_batch_gradient", self._NO_GRAD_AB)
        self._check_sizes(images=images)                                  # before any launch
        if cam and self.P > GRADCAM_MAX_PIXELS:
            raise ValueError("{}: a feature map of {} pixels; Grad-CAM heat maps are built for at most {} (lrpx_gradcam)".format(
                type(self).__name__, self.P, GRADCAM_MAX_PIXELS))
        images = images.to(self.device, torch.float32).contiguous()
        enc = self.encode(images)
        B, T, tr, rg, d_feat, r_words, row2img = self._decoder_gradient(enc, captions, lens)
        return self._finish(rg, B, T, d_feat, r_words, row2img, (lambda d, m: self.grad_cam(enc, d, m)) if cam else self.cnn.gradient,
                            (self.P,) if cam else tuple(images.shape[1:]), features=(tr, enc) if return_features else None)

    def explain_batch_guided(self, images, captions, lens=None, return_features=False, gradcam=False):
        """Batched `ExplainiAdaptiveGuidedGradient.explain_caption`: the same decoder gradient, guided backprop through the encoder
        (`explain_cnn`, :1175-1189) -> maps (B,T,3,H,W), word scores (B,T,T).  gradcam=True (`ExplainAdaptiveGuidedGradCam`) is refused."""
        self._preset_only("explain_batch_guided", self._NO_GRAD_AB)
        if gradcam:
            raise NotImplementedError("{}.explain_batch_guided(gradcam=True): {}".format(type(self).__name__, GUIDED_GRADCAM_MISSING))
        self._check_sizes(images=images)                                  # before any launch
        images = images.to(self.device, torch.float32).contiguous()
        enc = self.encode(images)
        B, T, tr, rg, d_feat, r_words, row2img = self._decoder_gradient(enc, captions, lens)
        return self._finish(rg, B, T, d_feat, r_words, row2img, self._guided_backprop, tuple(images.shape[1:]),
                            features=(tr, enc) if return_features else None)

    def explain_features_gradient(self, features, captions, lens=None):
        """The decoder gradient of every word of B captions on (B, P, C) features in place of the encoder's (an engine without an
        encoder): d_feat (B, T, P, C) - zero in rows behind an image's last word (`lens`) - and r_words (B, T, T)."""
        self._features_stage("explain_features_gradient")
        enc = self.encode(features=features)
        B, T, _, rg, d_feat, r_words, row2img = self._decoder_gradient(enc, captions, lens)
        return self._finish(rg, B, T, d_feat, r_words, row2img, lambda feat, m: feat, (self.P, self.C))


# ------------------------------------------------------------------------------------------------
# drop-in explainers (models/adaptiveattention.py:851-1320)
# ------------------------------------------------------------------------------------------------
class ExplainAdaptiveGradient(ExplainAdaptiveAttention):
    """Drop-in for the reference's `ExplainAdaptiveGradient` (models/adaptiveattention.py:851-1095): the hand-written decoder back-pass
    (`explain_caption_wordt`, :965-1021) and the autograd gradient through the encoder (`explain_cnn`, :1023-1036).  Same surface as
    `ExplainAdaptiveAttention`: `explain_caption(img) -> (maps, word scores)`; the image gradient is a fresh tensor per word."""
    EX_TYPE = 'gradient'
    TF_MODEL_BIAS = True
    _RUNNING_SUMS = False

    _ENGINE, _ENGINE_KIND = AdaAttGradEngine, "adaatt_grad"          # (an engine-cache key of its own: never `ExplainAdaptiveAttention`'s engine)

    def get_hidden_parameters(self, img, caption_encode=None, max_cap_length=20):
        super().get_hidden_parameters(img, caption_encode, max_cap_length)
        if self.caption_length:
            self._trace(grad=True)             # :900-963 (output gate and sentinel gate kept)

    def _explain_rows(self, head_idx):
        return self.engine.guided_gradient(self._enc, self._tr)

    def _cnn(self, d_feat, row2img):
        return self.engine.cnn.gradient(d_feat, row2img)

    def explain_cnn(self, d_img_feature):          # (the reference's argument name in this family)
        return super().explain_cnn(d_img_feature)


class ExplainiAdaptiveGuidedGradient(ExplainAdaptiveGradient):
    """Drop-in for `ExplainiAdaptiveGuidedGradient` (models/adaptiveattention.py:1098-1215): the same decoder gradient (its two extra
    masks select nothing, see the module text), guided backprop through the encoder (`explain_cnn`, :1175-1189)."""
    EX_TYPE = 'GuidedBackpropagate'

    def _cnn(self, d_feat, row2img):
        return self.engine._guided_backprop(d_feat, row2img)


class ExplainAdaptiveGradCam(ExplainAdaptiveGradient):
    """Drop-in for `ExplainAdaptiveGradCam` (models/adaptiveattention.py:1218-1258): `explain_caption` returns per word the (1, P)
    Grad-CAM heat map of the decoder gradient."""
    EX_TYPE = 'GradCam'

    def grad_cam(self, img_feature, grads):
        """(1,C,h,w) features and gradients -> (h*w,) heat map, as the reference's method of the same name (:1225-1236)."""
        from .gridtd import _grad_cam_one
        return _grad_cam_one(img_feature, grads).view(-1)

    def explain_cnn(self, d_img_feature):
        return self.grad_cam(self.image_features, d_img_feature).unsqueeze(0)

    def _cnn(self, d_feat, row2img):
        return self.engine.grad_cam(self._enc, d_feat, row2img)


class ExplainAdaptiveGuidedGradCam(ExplainiAdaptiveGuidedGradient):
    """`ExplainAdaptiveGuidedGradCam` (models/adaptiveattention.py:1261-1318) exists under the reference's name and refuses: see
    `GUIDED_GRADCAM_MISSING`."""
    EX_TYPE = 'GuidedGradCam'

    def __init__(self, args, word_map, model=None):
        raise NotImplementedError(GUIDED_GRADCAM_MISSING)
