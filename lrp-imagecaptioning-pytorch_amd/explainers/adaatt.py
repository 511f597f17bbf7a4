"""Batched LRP engine for the single-LSTM adaptive-attention model + the drop-in `ExplainAdaptiveAttention` explainer.

Reference: models/adaptiveattention.py - `AdaptiveAttentionCaptioningModel` (:101-135, the original adaptive-attention model with a
visual sentinel) and `ExplainAdaptiveAttention` (:493-848).  Kernels: csrc/lrpx_adaatt.hip behind the `lrpx_adaatt_*` section of the C
ABI; DESIGN.md 5.15.  What differs from gridTD (explainers/gridtd.py), all of it in the reference's code:

  1. the input row is x_t = [emb | glob] (:656), one LSTM cell; the LSTM bias is bias_ih + bias_hh (:557: no doubled bias);
  2. sentinel and context take relevance at the explained word only (:714-724) - the context never feeds the LSTM;
  3. the gate rule divides by tanh OF the pre-activation (:737);
  4. the glob columns of the gate rule count at i == t only (:740-741);
  5. the rules of `global_img_feature_proj` and `img_projector` divide by BIAS-FREE pre-activations (`forward_output=False`, :536-537).

The host logic below only sequences kernel launches; torch is used for device memory."""
import ctypes as C

import torch

from .. import _lib, ops
from .._lib import (EPI_PLAIN, EPI_REL, AdaRelState, AdaStepArgs, AdaTrace, PACK_DENSE, PACK_DENSE_T, check, ptr, ptr_at, stream_ptr)
from .dropin import ExplainerBase
from .engine_base import EngineBase, resnet_encoder_keys
from .ragged import ragged

UNITS_PER_GROUP = 3          # hidden units per 16-row group of the interleaved gate rows (include/lrpx.h: lrpx_adaatt_fwd_recurrence)


def interleave_index(H):
    """(NR,) int64: interleaved gate row r -> row of the stacked (5H + 1)-row matrix [i ; f ; g ; o ; sentinel gate ; zero row]:
    row 16 j + 5 u + q = gate q of hidden unit 3 j + u; row 16 j + 15 and the rows of units >= H point at the zero row 5H"""
    ng = -(-H // UNITS_PER_GROUP)
    idx = torch.full((16 * ng,), 5 * H, dtype=torch.int64)
    for u in range(UNITS_PER_GROUP):
        unit = torch.arange(ng) * UNITS_PER_GROUP + u
        ok = unit < H
        for q in range(5):
            rows = torch.arange(ng) * 16 + 5 * u + q
            idx[rows[ok]] = q * H + unit[ok]
    return idx


class AdaAttEngine(EngineBase):
    """Device-resident single-LSTM adaptive-attention model + trace / relevance pipelines.  `state`: the reference model's `state_dict`
    (torch tensors or numpy arrays, names of models/adaptiveattention.py:112-120).  The encoder (:18-38) is chosen as for
    `GridTDEngine`: VGG16 from the keys under `img_encoder.encoder.`, a bottleneck ResNet from `encoder=` or from models/resnet.py key
    names, or none - a state without encoder keys explains (B, P, C) features (`explain_features`, `encode(features=)`).  The decoder's
    sizes C (`img_projector`) and P (`AdaAttention.W_v_proj`) must match what it is fed (`encode` checks).

    `cut_dead_columns` (default True): the gate rule of the lock-steps s >= 1 contracts N = H + E columns instead of H + 2E - the glob
    columns are read at s == 0 only (:740-741); every value that is read is bit-identical either way (A/B and tests).
    `decoupled` (default True): the teacher-forced trace with the recurrence apart from what hangs off it - one GEMM for the input
    half of the gate rows of all B*T rows, one launch per time step, the attention once over all rows; False: the per-step entries the
    decoding loops use (values equal to rounding)."""

    ENCODER_CONV_MODES = EngineBase._ENCODER_CONV_MODES
    GRADIENT_FOLLOW_UP = ("the gradient explainers of this model (ExplainAdaptiveAttentionGradient / GuidedGradient / GradCam / GuidedGradCam, "
                          "models/adaptiveattention.py:851-1320) live in the follow-up to this engine, AdaAttGradEngine "
                          "(explainers/adaatt_grad.py): AdaAttEngine has the LRP explainer only")
    NO_LRP_INFERENCE = "models/adaptiveattention.py defines no sample_lrp / forwardlrp_context for this model"

    def __init__(self, state, device="cuda", encoder=None, encoder_conv_mode=1):
        self._check_state(state)
        sd = self._init_encoder(state, device, encoder, encoder_conv_mode, need_encoder=False)
        self.sd = sd
        self.V, self.E = sd["embedding.weight"].shape
        self.H = sd["fc.weight"].shape[1]
        self.C = sd["img_projector.weight"].shape[1]
        self.P = sd["AdaAttention.W_v_proj.weight"].shape[0]
        H, E, Cc = self.H, self.E, self.C
        assert H == 512 and E == 512, "kernels are built for hidden=embed=512 (config.py:123-124; the reference's xt buffer needs E == H, :640)"
        a = "AdaLSTM.lstm_cell."
        w_ih, w_hh = sd[a + "weight_ih"], sd[a + "weight_hh"]
        wx, wh = torch.cat([w_ih, sd["AdaLSTM.x_gate.weight"]], 0), torch.cat([w_hh, sd["AdaLSTM.h_gate.weight"]], 0)     # (5H, 2E), (5H, H)
        bias = torch.cat([sd[a + "bias_ih"] + sd[a + "bias_hh"], sd["AdaLSTM.x_gate.bias"] + sd["AdaLSTM.h_gate.bias"]])      # :557, :51
        # per-step path: one dot product over the row [h | emb | glob]
        self.Wcat, self.bcat = torch.cat([wh, wx], 1).contiguous(), bias.contiguous()
        # decoupled trace: gate rows interleaved so that one workgroup of the recurrence owns the five rows of its hidden units
        il = interleave_index(H).to(self.device)
        z = lambda t: torch.cat([t, t.new_zeros((1,) + tuple(t.shape[1:]))], 0)
        self.Wx_il, self.Wh_il, self.b_il = z(wx)[il].contiguous(), z(wh)[il].contiguous(), z(bias)[il].contiguous()
        self.NR = il.shape[0]
        self.decoupled = True
        self.cut_dead_columns = True
        self.w_proj2d = sd["img_projector.weight"].reshape(H, Cc).contiguous()
        kc = ops.conv_kc(0, 1, Cc)
        self.p_proj_fwd = ops.pack_weights(self.w_proj2d, H, Cc, 1, PACK_DENSE, kc)
        self.p_attv_fwd = ops.pack_weights(sd["AdaAttention.W_v_proj.weight"], self.P, H, 1, PACK_DENSE, ops.conv_kc(0, 1, H))
        self.p_fc_fwd = ops.pack_weights(sd["fc.weight"], self.V, H, 1, PACK_DENSE, ops.conv_kc(0, 1, H))
        self.p_fc_fwd_h = None            # every contraction of this engine is fp32 arithmetic (no fp16 split products)
        self.force_f16 = False
        # relevance: the g-gate rows [W_hh^g | W_ih^g] - the columns of xh (:685-688 with the h columns first)
        wg = torch.cat([w_hh[2 * H:3 * H], w_ih[2 * H:3 * H]], 1).contiguous()
        self.p_wg = ops.pack_weights(wg, H, H + 2 * E, 1, PACK_DENSE_T, ops.conv_kc(0, 1, H))
        self.p_gp_rel = ops.pack_weights(sd["global_img_feature_proj.weight"], E, Cc, 1, PACK_DENSE_T, ops.conv_kc(0, 1, E))
        self.p_proj_rel = ops.pack_weights(self.w_proj2d, H, Cc, 1, PACK_DENSE_T, ops.conv_kc(0, 1, H))
        self.p_proj_rel_h = None
        self.p_proj_rel_6 = ops.pack_weights_bf16x3(self.w_proj2d, H, Cc, _lib.PACK_BWD_PLAIN, taps=1) if (H % 32 == 0 and Cc % 4 == 0) else None
        self.dense_bf16x6 = True         # False: the projector rule on the fp32 MFMA kernel (A/B and tests)
        torch.cuda.synchronize()
        self._idx_cache = {}

    @staticmethod
    def _check_state(state):
        """host logic: the three ways a state is not `AdaptiveAttentionCaptioningModel`'s"""
        for k in state:
            if k.startswith("LanguageLSTM."):
                raise ValueError("AdaAttEngine: the state holds {!r}: a gridTD state (two LSTMs; GridTDEngine explains it) - the "
                                 "adaptive-attention model has the AdaLSTM cell only".format(k))
        w_ih, emb = state["AdaLSTM.lstm_cell.weight_ih"], state["embedding.weight"]
        if len(w_ih.shape) != 2 or w_ih.shape[1] != 2 * emb.shape[1]:
            raise ValueError("AdaAttEngine: 'AdaLSTM.lstm_cell.weight_ih' is {}; this model's cell reads x_t = [emb | glob], 2E = {} "
                             "columns (gridTD's reads 2E + H)".format(tuple(w_ih.shape), 2 * emb.shape[1]))
        wp = state["img_projector.weight"]
        if len(wp.shape) != 4:
            raise ValueError("AdaAttEngine: 'img_projector.weight' is {}-D {}; this model's projector is a 1 x 1 Conv2d, (H, C, 1, 1) "
                             "(a 2-D weight is a bottom-up model's Linear)".format(len(wp.shape), tuple(wp.shape)))

    # ------------------------------------------------------------------------------------------
    def _alloc_trace(self, B, T, grad=False):
        dev, H, E, P = self.device, self.H, self.E, self.P
        shapes = {"xh": (B, T, H + 2 * E), "h": (B, T + 1, H), "c": (B, T + 1, H), "alpha": (B, T, P), "beta": (B, T)}
        names = ["xh", "h", "c", "g", "i", "f", "s", "ctx", "ctx_hat", "hc", "alpha", "beta"]
        for k in names[3:10]:
            shapes[k] = (B, T, H)
        if grad:                                           # the gradient explainers' trace: output gate and sentinel gate kept
            names += ["o", "sgate"]
            shapes["o"] = shapes["sgate"] = (B, T, H)
        tr = dict(B=B, T=T)
        tr.update(ops.zeros_arena(dev, shapes))            # one allocation, one fill (h[0] = c[0] = 0: init_hidden_state, :123-126)
        c = AdaTrace()
        c.B, c.T, c.H, c.E, c.P = B, T, H, E, P
        for k in names:
            setattr(c, k, ptr(tr[k]))
        tr["_c"] = c
        return tr

    def feature_shape(self, images):
        """(h, w, C) of the encoder's feature map for these images (host arithmetic)"""
        if self.cnn is None:
            raise ValueError("AdaAttEngine: this engine was built from a state without encoder keys: it takes (B, P, C) features "
                             "(encode(features=...), explain_features), not images")
        if images.dim() != 4:
            raise ValueError("AdaAttEngine: images must be (B, 3, H, W), got {}".format(tuple(images.shape)))
        if self.resnet:
            return self.cnn.feature_shape(int(images.shape[2]), int(images.shape[3]))
        return self.cnn.feat_hw + (512,)

    def _check_sizes(self, images=None, features=None):
        """the decoder is built for P pixels of C channels: refuse anything else here, before any kernel runs"""
        if (images is None) == (features is None):
            raise ValueError("AdaAttEngine: give images or features (one of them)")
        if features is not None:
            if features.dim() != 3:
                raise ValueError("AdaAttEngine: features must be (B, P, C), NHWC rows, got {}".format(tuple(features.shape)))
            p, c, what = int(features.shape[1]), int(features.shape[2]), "features of"
        else:
            h, w, c = self.feature_shape(images)
            p, what = h * w, "{}x{} images give a {}x{} feature map =".format(int(images.shape[2]), int(images.shape[3]), h, w)
        if p != self.P or c != self.C:
            raise ValueError("AdaAttEngine: {} {} pixels of {} channels; the decoder is built for {} pixels (AdaAttention.W_v_proj) of {} "
                             "channels (img_projector)".format(what, p, c, self.P, self.C))

    def encode(self, images=None, features=None):
        """Encoder forward (or `features`, (B, P, C) NHWC, in its place) + the image-side constants of get_hidden_parameters (:632-637):
        avg, proj_pre / Vp, glob_pre / glob, att_img - and the BIAS-FREE pre-activations proj_nb, glob_nb the two image-side rules
        divide by (:536-537), each formed by the GEMM that forms the biased one, without its bias."""
        self._check_sizes(images, features)                                # before any launch
        lib = _lib.load()
        st = stream_ptr()
        H, E, Cc, P = self.H, self.E, self.C, self.P
        if features is not None:
            feats = features.to(self.device, torch.float32).contiguous()
        else:
            feats = self.cnn.forward(images.to(self.device, torch.float32).contiguous())         # (B,P,C) NHWC view into the trace
        B = feats.shape[0]
        e = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)
        enc = dict(B=B, feats=feats)
        enc["avg"] = e(B, Cc)
        check(lib.lrpx_mean_pixels(ptr(feats), ptr(enc["avg"]), B, P, Cc, st))
        for name, bias in (("proj_pre", self.sd["img_projector.bias"]), ("proj_nb", None)):
            enc[name] = e(B, P, H)
            ops.conv_mfma(feats, self.p_proj_fwd, B, 0, Cc, H, 1, EPI_PLAIN, pix_per_map=P, oc_split=H, bias=bias, out0=enc[name])
        enc["Vp"] = e(B, P, H)
        check(lib.lrpx_relu(ptr(enc["proj_pre"]), ptr(enc["Vp"]), enc["Vp"].numel(), st))
        wgp = self.sd["global_img_feature_proj.weight"]
        for name, bias in (("glob_pre", self.sd["global_img_feature_proj.bias"]), ("glob_nb", None)):
            enc[name] = e(B, E)
            for b0 in range(0, B, 64):      # (slices of <= 64 rows: the same kernel whatever the batch size)
                check(lib.lrpx_linear_small(ptr_at(enc["avg"], b0 * Cc), Cc, ptr(wgp), ptr(bias), ptr_at(enc[name], b0 * E), E,
                                            min(64, B - b0), Cc, E, 0, st))
        enc["glob"] = e(B, E)
        check(lib.lrpx_relu(ptr(enc["glob_pre"]), ptr(enc["glob"]), enc["glob"].numel(), st))
        # time-invariant part of the attention scores: W_v_proj(V) + b  (:74)
        enc["att_img"] = e(B, P, P)
        ops.conv_mfma(enc["Vp"], self.p_attv_fwd, B, 0, H, -(-P // 32) * 32, 1, EPI_PLAIN, pix_per_map=P, oc_split=P,
                      bias=self.sd["AdaAttention.W_v_proj.bias"], out0=enc["att_img"])
        return enc

    def _step_args(self, tr, enc, B):
        sa, sd, aa = AdaStepArgs(), self.sd, "AdaAttention."
        if "_zz" not in tr:
            tr["_zz"], tr["_att_scr"] = torch.empty(B, 5 * self.H, device=self.device), torch.empty(B, 3 * self.P, device=self.device)
        sa.w_cat, sa.b_cat, sa.Vp, sa.att_img = ptr(self.Wcat), ptr(self.bcat), ptr(enc["Vp"]), ptr(enc["att_img"])
        sa.Wg, sa.Ws, sa.bs, sa.wh = ptr(sd[aa + "W_g_proj.weight"]), ptr(sd[aa + "W_s_proj.weight"]), ptr(sd[aa + "W_s_proj.bias"]), ptr(sd[aa + "w_h.weight"])
        sa.zz, sa.att_scratch = ptr(tr["_zz"]), ptr(tr["_att_scr"])
        tr["_sa"] = sa
        return sa

    def _step(self, tr, enc, t, tokens):
        """decoder step t (predict_next_word, :128-135) for all rows: column t of `tokens` is its input"""
        lib, st = _lib.load(), stream_ptr()
        sa = tr.get("_sa") or self._step_args(tr, enc, tr["B"])
        c = C.byref(tr["_c"])
        check(lib.lrpx_adaatt_fwd_pre(c, t, ptr(enc["glob"]), ptr(self.sd["embedding.weight"]), ptr(tokens), tokens.shape[1], st))
        check(lib.lrpx_adaatt_fwd_step(c, t, C.byref(sa), st))

    def trace(self, enc, captions, model_bias=True, predictions=True, grad=False):
        """get_hidden_parameters (:651-677) for B images under teacher forcing.  captions: (B,T+1) int64, column 0 = <start>.
        (`model_bias`: accepted for the drop-in base; this explainer's forward IS the model's, :557.)"""
        if grad:
            raise NotImplementedError("AdaAttEngine.trace(grad=True): " + self.GRADIENT_FOLLOW_UP)
        return self._teacher_forced(enc, captions, predictions, False)

    def _teacher_forced(self, enc, captions, predictions, grad):
        """the body of `trace`; grad=True keeps the output gate and the sentinel gate (explainers/adaatt_grad.py)"""
        lib, st = _lib.load(), stream_ptr()
        B, T = captions.shape[0], captions.shape[1] - 1
        H, E, P, dev, sd = self.H, self.E, self.P, self.device, self.sd
        captions = captions.to(dev, torch.int64).contiguous()      # (token ids index the embedding table: never another width)
        tr = self._alloc_trace(B, T, grad)
        c = C.byref(tr["_c"])
        if self.decoupled and T > 0:
            W, R, NR, aa = H + 2 * E, B * T, self.NR, "AdaAttention."
            check(lib.lrpx_adaatt_fwd_inputs(c, ptr(enc["glob"]), ptr(sd["embedding.weight"]), ptr(captions), captions.shape[1], st))
            zin = torch.empty(R, NR, device=dev)
            for r0 in range(0, R, 64):      # slices of <= 64 rows: the same (MFMA) kernel whatever the batch size - an image's trace never depends on its batch
                check(lib.lrpx_linear_small(ptr_at(tr["xh"], r0 * W + H), W, ptr(self.Wx_il), ptr(self.b_il), ptr_at(zin, r0 * NR), NR,
                                            min(64, R - r0), 2 * E, NR, 0, st))
            check(lib.lrpx_adaatt_fwd_recurrence(c, ptr(self.Wh_il), ptr(zin), st))
            tr["_att_scr"] = torch.empty(R, 3 * P, device=dev)
            check(lib.lrpx_adaatt_fwd_attention_all(c, ptr(enc["Vp"]), ptr(enc["att_img"]), ptr(sd[aa + "W_g_proj.weight"]),
                                                    ptr(sd[aa + "W_s_proj.weight"]), ptr(sd[aa + "W_s_proj.bias"]), ptr(sd[aa + "w_h.weight"]),
                                                    ptr(tr["_att_scr"]), st))
        else:
            for t in range(T):
                self._step(tr, enc, t, captions)
        tr["captions"] = captions
        tr["logit"] = torch.empty(B * T, device=dev)
        check(lib.lrpx_target_logit(ptr(tr["hc"]), ptr(sd["fc.weight"]), ptr(sd["fc.bias"]), ptr(captions), T + 1, ptr(tr["logit"]), B, T, H, st))
        if predictions:
            tr["pred"] = self.logits(tr["hc"].view(B * T, H)).view(B, T, self.V)
        return tr

    def greedy(self, enc, max_cap_length, start_id, end_id):
        """`greedy_search` (:442-490): argmax per step; after the first <end> the sequence is padded with 0.  Returns int64
        (B, max_cap_length) incl. <start>."""
        lib = _lib.load()
        B, T = enc["B"], max_cap_length - 1
        toks = torch.zeros(B, T + 1, dtype=torch.int64, device=self.device)
        toks[:, 0] = start_id
        tr = self._alloc_trace(B, T)
        nxt = torch.empty(B, dtype=torch.int64, device=self.device)
        unfinished = torch.ones(B, dtype=torch.bool, device=self.device)
        for t in range(T):
            self._step(tr, enc, t, toks)
            lg = self.logits(tr["hc"][:, t].contiguous())
            check(lib.lrpx_argmax_rows(ptr(lg), self.V, B, self.V, ptr(nxt), stream_ptr()))
            unfinished = unfinished & (nxt != end_id)          # token bookkeeping (integers), :471-477
            toks[:, t + 1] = nxt * unfinished
        return toks

    # the beam search of explainers/engine_base.py on this model's step (`beam_search`, :370-440: gridTD's algorithm on one state pair)
    _BEAM_STATE = ("h", "c")

    def _decode_trace(self, enc, B, T, lrp=False):
        if lrp:
            raise NotImplementedError("AdaAttEngine: " + self.NO_LRP_INFERENCE)
        return self._alloc_trace(B, T)

    def _decode_step(self, tr, enc, t, toks):
        self._step(tr, enc, t, toks)

    def sample_lrp(self, *a, **k):
        raise NotImplementedError("AdaAttEngine.sample_lrp: " + self.NO_LRP_INFERENCE)

    def forwardlrp_context(self, *a, **k):
        raise NotImplementedError("AdaAttEngine.forwardlrp_context: " + self.NO_LRP_INFERENCE)

    # ------------------------------------------------------------------------------------------
    def relevance(self, enc, tr, lens=None):
        """explain_caption_wordt (:679-771) for every (image, word) row at once.  Returns r_feat (B*T, P, C) relevance of the encoder
        output (NHWC), r_words (B*T, T) and the row -> image table.  lens (explainers/ragged.py): words past an image's length are
        skipped by the lock-step kernels (their r_words rows stay zero), and the (word, pixel) rules run on the valid rows only - r_feat is
        then COMPACT, (sum(lens), P, C) in image-major order, with the matching row -> image table.  The state tensors of the last call
        stay in `self.last_rel` (r_glob, r_ctx, ...: what the tests read)."""
        lib, st = _lib.load(), stream_ptr()
        B, T, H, E, P, Cc = tr["B"], tr["T"], self.H, self.E, self.P, self.C
        rows, W, dev = B * T, self.H + 2 * self.E, self.device
        rg = ragged(lens, B, T, dev)
        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        rs = dict(r_h=e(rows, H), r_c=e(rows, H), r_ctx=e(rows, H), r_glob=e(rows, E), A=e(rows, H), rx=e(rows, W), r_words=e(rows, T))
        c = AdaRelState()
        c.lens = ptr(rg.lens) if rg is not None else None
        for k, v in rs.items():
            setattr(c, k, ptr(v))
        ctr, crs = C.byref(tr["_c"]), C.byref(c)
        idx, row2img, _ = self._row_index(B, T)
        check(lib.lrpx_adaatt_rel_init(ctr, crs, ptr(self.sd["fc.weight"]), ptr(tr["logit"]), ptr(tr["captions"]), T + 1, st))
        d = ops.conv_desc(rs["A"], self.p_wg, rows, 0, H, W, 1, EPI_REL, pix_per_map=1, oc_split=W, x=tr["xh"], map2img=idx[0], out0=rs["rx"])
        check(lib.lrpx_adaatt_rel_steps(ctr, crs, T, C.byref(d), ptr(idx), idx.shape[1], 1 if self.cut_dead_columns else 0, st))
        # global feature path (:743-755) and projector (:756-763)
        a_glob = e(rows, E)
        check(lib.lrpx_adaatt_rel_glob(ctr, crs, ptr(enc["glob_nb"]), ptr(a_glob), st))
        r_avg = e(rows, Cc)
        ops.conv_mfma(a_glob, self.p_gp_rel, rows, 0, E, -(-Cc // 32) * 32, 1, EPI_REL, pix_per_map=1, oc_split=Cc, x=enc["avg"],
                      map2img=row2img, out0=r_avg)
        U = e(rows, Cc)
        check(lib.lrpx_rel_avg_u(ptr(r_avg), ptr(enc["avg"]), ptr(U), rows, T, Cc, P, st))
        check(lib.lrpx_rel_words_norm(ptr(rs["r_words"]), rows, T, st))
        self.last_rel = rs
        n, rowlist = rows, None
        if rg is not None and not rg.full:       # unequal lengths: the (word, pixel) rule on the valid rows only, compact
            n, rowlist, row2img = rg.n, rg.rows, rg.row2img
            if n == 0:
                return e(0, P, Cc), rs["r_words"], row2img
            U = ops.gather_rows(U, rowlist)
        a_proj = e(n, P, H)
        check(lib.lrpx_adaatt_rel_pix_rows(ctr, crs, ptr(enc["Vp"]), ptr(enc["proj_nb"]), ptr(a_proj), ptr(rowlist), n, st))
        rs["a_proj"] = a_proj
        r_feat = e(n, P, Cc)
        self._proj_rule(a_proj, n, P, enc["feats"], row2img, r_feat, u=U)
        return r_feat, rs["r_words"], row2img

    def explain_features(self, features, captions, lens=None, predictions=False):
        """Every word of B captions explained on (B, P, C) features in place of the encoder's; captions (B, T+1) int64, column 0 =
        <start>.  Returns r_feat (B, T, P, C) - zero in rows behind an image's last word (`lens`) - and r_words (B, T, T) (row t holds
        t + 1 valid entries); then the (B, T, V) scores with predictions=True.  No encoder stage: `lrp_params` must be None."""
        self._features_stage("explain_features")
        enc = self.encode(features=features)
        captions = captions.to(self.device, torch.int64).contiguous()
        B, T = captions.shape[0], captions.shape[1] - 1
        tr = self.trace(enc, captions, predictions=predictions)
        rg = ragged(lens, B, T, self.device)
        r_feat, r_words, row2img = self.relevance(enc, tr, rg)
        return self._finish(rg, B, T, r_feat, r_words, row2img, lambda feat, m: feat, (self.P, self.C), extra=(tr["pred"],) if predictions else ())

    def explain_batch(self, images, captions, lens=None, accumulate=False, return_features=False, predictions=False):
        """Batched `explain_caption` (:779-794): images (B,3,H,W) of the encoder's size, captions (B,T+1) int64.  Returns maps
        (B,T,3,H,W) and r_words (B,T,T); accumulate=True: the running sums the reference returns (lrp_wrapper.py:64-82 quirk);
        predictions=True: then the (B,T,V) scores; return_features=True: then r_feat (B,T,P,C), the trace and `encode`'s dict.
        The instance attribute `lrp_params` selects the encoder's Conv2d rule (explainers/engine_base.py: `_maps_stage`)."""
        maps_of = self._maps_stage("explain_batch")
        self._check_sizes(images=images)
        images = images.to(self.device, torch.float32).contiguous()
        captions = captions.to(self.device, torch.int64).contiguous()
        B, T = captions.shape[0], captions.shape[1] - 1
        enc = self.encode(images)
        tr = self.trace(enc, captions, predictions=predictions)
        rg = ragged(lens, B, T, self.device)
        r_feat, r_words, row2img = self.relevance(enc, tr, rg)
        return self._finish(rg, B, T, r_feat, r_words, row2img, maps_of, tuple(images.shape[1:]), accumulate=accumulate,
                            extra=(tr["pred"],) if predictions else (), features=(tr, enc) if return_features else None)

    def explain_stream(self, batches, depth=3, accumulate=False):
        """`explain_batch` over an iterable of (images, captions[, lens]) batches, `depth` in flight (explainers/engine_base.py); an
        engine without an encoder streams `explain_features` over (features, captions[, lens]) batches."""
        if self.cnn is None:
            self._features_stage("explain_stream")
            return self._explain_stream(batches, depth, lambda eng, f, c, lens: eng.explain_features(f, c, lens=lens))
        self._maps_stage("explain_stream")                # a refusal here, not inside the generator's first step
        return self._explain_stream(batches, depth, lambda eng, i, c, lens: eng.explain_batch(i, c, lens=lens, accumulate=accumulate))

    def _static(self, graph, src, captions, accumulate, predictions, *key):
        src, captions = src.to(self.device, torch.float32), captions.to(self.device, torch.int64)
        feats = src.dim() == 3
        self._check_sizes(features=src) if feats else self._check_sizes(images=src)
        key = (tuple(src.shape), tuple(captions.shape), bool(accumulate), bool(predictions)) + key
        step = (lambda f, c: self.explain_features(f, c, predictions=predictions)) if feats else \
            (lambda i, c: self.explain_batch(i, c, accumulate=accumulate, predictions=predictions))
        return self._static_step(graph, key, src, captions, step)

    def explain_batch_graph(self, images, captions, accumulate=False, predictions=False):
        """`explain_batch` (images) or `explain_features` ((B, P, C) features) replayed from a captured HIP graph, one per input shape
        (explainers/engine_base.py: `_static_step`)."""
        self._preset_only("explain_batch_graph", self._NO_STATIC_AB)
        self._refuse_resnet("explain_batch_graph", self._NO_GRAPH)
        return self._static(True, images, captions, accumulate, predictions)

    def explain_batch_replay(self, images, captions, accumulate=False, predictions=False):
        """the same as a RECORDED step, one per input shape and stream (explainers/engine_base.py: `_static_step`)."""
        self._preset_only("explain_batch_replay", self._NO_STATIC_AB)
        self._refuse_resnet("explain_batch_replay", self._NO_RECORDING)
        return self._static(False, images, captions, accumulate, predictions, _lib.stream_ptr().value,
                            self.vgg.conv_mode if self.vgg is not None else None)

    def _no_gradient(self, entry):
        raise NotImplementedError("AdaAttEngine.{}: {}".format(entry, self.GRADIENT_FOLLOW_UP))

    def guided_gradient(self, enc, tr, lens=None, mask_features=True):
        self._no_gradient("guided_gradient")

    def explain_batch_guided(self, images, captions, lens=None, return_features=False, gradcam=False):
        self._no_gradient("explain_batch_guided")

    def explain_batch_gradient(self, images, captions, lens=None, cam=False, return_features=False):
        self._no_gradient("explain_batch_gradient")


# ------------------------------------------------------------------------------------------------
# drop-in explainer (models/adaptiveattention.py:493-848)
# ------------------------------------------------------------------------------------------------
class ExplainAdaptiveAttention(ExplainerBase):
    """Same constructor, attributes and methods as the reference's `ExplainAdaptiveAttention` (models/adaptiveattention.py:493-794):
    `explain_caption(img_filepath, t_list=None) -> (relevance_imgs, relevance_preceeding_words)`, `get_hidden_parameters`,
    `explain_caption_wordt(t)`, `explain_cnn(R)`, `preprocess_img`, `teacherforce_forward(img, ids)`; attributes `.model .word_map
    .img .beam_caption .beam_caption_encode .predictions .alphas .betas .args`.  Conventions: explainers/dropin.py; the caption the
    reference explains is `beam_search(beam_size=3, max_cap_length=20)` (:628).  `t_list` selects what the reference draws
    (`visualize_explanations`); nothing is drawn here, every word is explained.  A ResNet encoder is handed over as for
    `ExplainGridTDAttention`."""
    _ENGINE, _ENGINE_KIND = AdaAttEngine, "adaatt"          # the engine class and its engine-cache kind (the gradient family has its own)

    def _engine_key(self):
        from . import engine_cache
        mode = getattr(self.args, "encoder_conv_mode", 1)
        return engine_cache.fingerprint(self._ENGINE_KIND, self.args.weight if self.model is None else self.model,
                                        extra=() if mode == 1 else (("encoder_conv_mode", mode),))

    def _build_engine(self, state):
        encoder = None
        if hasattr(self.model, "state_dict"):
            enc = getattr(getattr(self.model, "img_encoder", None), "encoder", None)
            if resnet_encoder_keys(state) and isinstance(enc, torch.nn.Module) and all(
                    t.device.type == "cuda" for t in list(enc.parameters()) + list(enc.buffers())):
                encoder = enc                  # the model's own module (else: rebuilt from the same tensors by the engine)
        return self._ENGINE(state, encoder=encoder, encoder_conv_mode=getattr(self.args, "encoder_conv_mode", 1))

    def get_hidden_parameters(self, img, caption_encode=None, max_cap_length=20):
        """Forward trace (:626-677).  `img`: file path or a (1,3,H,W) tensor of the encoder's image size."""
        self._hidden_parameters(img, caption_encode, 3, max_cap_length)

    def _explain_rows(self, head_idx):
        return self.engine.relevance(self._enc, self._tr)

    def explain_caption_wordt(self, t):
        """(:679-771) -> (r_img_feature (1,C,h,w), r_words (t+1,))"""
        return self._explain_wordt(t)

    def explain_caption(self, img_filepath, t_list=None, caption_encode=None):
        """(:779-794) -> ([T] x (1,3,H,W), [T] x (t+1,)); the LRP maps are the reference's running sums."""
        return self._explain_caption(img_filepath, caption_encode)
