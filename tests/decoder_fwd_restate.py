"""The decoder FORWARD traces of csrc/decoder_gridtd.hip, csrc/decoder_aoa.hip and csrc/lrpx_adaatt.hip restated time step by time step in plain torch, from the formulae
of the reference (models/gridTDmodel.py, models/aoamodel.py, models/adaptiveattention.py: line numbers at each step, as in the .hip comments and
oracle/lrp_oracle.py), from ANY initial state - and the planted models and drawn inputs the kernel tests run them on.  A helper module, not a
conftest.

    gridtd_fwd(sd, enc, tok, dtype, order, model_bias, gate_h_new=False, h0=None)   get_hidden_parameters, gridTDmodel.py:933-1012, :71-103
    aoa_fwd(sd, enc, tok, num_head, dtype, order, model_bias, h0=None)              get_hidden_parameters, aoamodel.py:1019-1052, :77-108
    adaatt_fwd(sd, enc, tok, dtype, order, h0=None)                                 forward_greedy, adaptiveattention.py:554-604, :56-134
    lrp_reweight(pred, h, ctx, fcw, skip, log_softmax, dtype, order)                get_lrp_weight_step, gridTDmodel.py:548-577, :687; aoamodel.py:597-626
    linear, mean_pixels, target_logit, argmax_logprob                               the building blocks

`sd`: the model's UN-interleaved state dict (CPU tensors), `enc` the image-side constants (`glob`, `Vp`, `att_img` / `glob`, `key`, `value`),
`tok` (B, >= T + 1) token ids (the columns behind T + 1 are never read), `dtype` torch.float64 / float32, `order` the summation order of every
matrix product and softmax denominator (decoder_restate.ORDERS), `h0` the state of slot 0 (None: zeros, `init_hidden_state`).  Each returns every
tensor the C trace struct exposes, batched as the engines keep them ([B][T][..], [B][T+1][..], g = gate PRE-activation), and the attention
scores.  The reference's quirks are kept: h_proj[k] broadcast along the ROW of img_proj (gridTDmodel.py:82), LanguageLSTM's bias_ih added twice
(:789, aoamodel.py:873), the sentinel gate on h_{t-1} (:982) unless `gate_h_new` (:672)."""
import functools
import math

import torch

from decoder_restate import ORDERS, _chunks, mm, tot, worst_of  # noqa: F401  (ORDERS, worst_of: for the tests that import this module)

H = E = 512
EPS = 0.01
NH_DRAW = 8


def stab(z):
    """z + eps sign(z); exact zeros (of either sign) -> eps   (gridTDmodel.py:757-759)"""
    zt = z + EPS * torch.sign(z)
    return torch.where(zt == 0, torch.full_like(zt, EPS), zt)


def tot_last(x, order):
    """sum over the last dimension in `order` (decoder_restate.tot for a batch of rows)"""
    if order == "torch":
        return x.sum(-1)
    out = None
    for k0 in _chunks(x.shape[-1], order):
        p = x[..., k0:k0 + 128].sum(-1)
        out = p if out is None else out + p
    return out


def lin(x, w, b, order):
    """nn.Linear: x (.., K) @ w (N, K)^T + b"""
    out = mm(x, w.t(), order)
    return out if b is None else out + b


def softmax_last(z, order):
    if order == "torch":
        return torch.softmax(z, -1)
    e = torch.exp(z - z.max(-1, keepdim=True).values)
    return e / tot_last(e, order)[..., None]


def _cast(d, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


def _zeros(dtype, *s):
    return torch.zeros(*s, dtype=dtype)


# ---- the building blocks ---------------------------------------------------------------------------------------------------------------------
def linear(x, w, bias, act, dtype, order):
    """lrpx_linear_small: act(x @ w^T + bias), act 1 = relu"""
    out = lin(x.to(dtype), w.to(dtype), None if bias is None else bias.to(dtype), order)
    return torch.relu(out) if act == 1 else out


def mean_pixels(f, dtype, order):
    """(B, P, C) -> (B, C): the mean over the pixels (gridTDmodel.py:941, aoamodel.py:1003), the P terms summed in `order`"""
    f = f.to(dtype)
    P = f.shape[1]
    if order == "torch":
        return f.mean(1)
    seq = list(range(P))[::-1] if order == "rev128" else list(range(0, P, 2)) + list(range(1, P, 2))
    out = f[:, seq[0]]
    for p in seq[1:]:
        out = out + f[:, p]
    return out / P


def target_logit(hc, fcw, fcb, tok, dtype, order):
    """logit[b * T + t] = fc.weight[k] . hc[b, t] + fc.bias[k], k = tok[b, t + 1]   (gridTDmodel.py:1033-1036)"""
    B, T, _ = hc.shape
    k = tok[:, 1:T + 1]
    return (tot_last(fcw.to(dtype)[k] * hc.to(dtype), order) + fcb.to(dtype)[k]).reshape(B * T)


def argmax_logprob(x, dtype, order):
    """(index of the first maximum of every row, log_softmax(row)[index])   (gridTDmodel.py:522-526)"""
    idx = torch.argmax(x, -1)          # (torch.argmax: the first of several maxima)
    xd = x.to(dtype)
    m = xd.max(-1, keepdim=True).values
    lp = torch.stack([-torch.log(tot(torch.exp(r - mi), order)) for r, mi in zip(xd, m[:, 0])])          # x[k] - max = 0
    return idx, lp


# ---- AdaptiveAttention.forward ---------------------------------------------------------------------------------------------------------------
def _adaptive_attention(w, Vp, att_img, h, s, order):
    """gridTDmodel.py:71-103 = adaptiveattention.py:56-98 for a batch of rows.  Vp (B, P, H), att_img = W_v_proj(Vp) + b (B, P, P), h, s (B, H)
    -> ctx_hat, ctx, alpha, beta, zsc (B, P + 1) = [pixel scores | sentinel score]"""
    a = "AdaAttention."
    wh = w[a + "w_h.weight"][0]                                                                     # (P,)
    h_proj = lin(h, w[a + "W_g_proj.weight"], None, order)                                          # :80  (B, P)
    z = tot_last(wh * torch.tanh(att_img + h_proj[:, :, None]), order)                              # :82-86: h_proj[k] along the ROW of img_proj
    alpha = softmax_last(z, order)                                                                  # :88
    ctx = _pix_sum(Vp * alpha[:, :, None], order)                                                   # :90
    s_proj = lin(s, w[a + "W_s_proj.weight"], w[a + "W_s_proj.bias"], order)
    zs = tot_last(wh * torch.tanh(s_proj + h_proj), order)                                          # :92-94
    zsc = torch.cat([z, zs[:, None]], 1)
    beta = softmax_last(zsc, order)[:, -1]                                                          # :96-100
    ctx_hat = beta[:, None] * s + (1 - beta[:, None]) * ctx                                         # :102
    return ctx_hat, ctx, alpha, beta, zsc


def _pix_sum(x, order):
    """sum over the pixel dimension (B, P, C) -> (B, C) in `order`"""
    return tot_last(x.transpose(1, 2), order)


def _cell(z, c_old):
    """gridTDmodel.py:777-784 (nn.LSTMCell's order of the gates: i, f, g, o) -> h', c', g pre-activation, i, f, o"""
    zi, zf, zg, zo = z.chunk(4, -1)
    i, f, o = torch.sigmoid(zi), torch.sigmoid(zf), torch.sigmoid(zo)
    c = f * c_old + i * torch.tanh(zg)
    return o * torch.tanh(c), c, zg, i, f, o


# ---- gridTD ------------------------------------------------------------------------------------------------------------------------------------
def gridtd_fwd(sd, enc, tok, dtype, order, model_bias, gate_h_new=False, h0=None, T=None):
    """-> xh1 (B, T, 2E + 2H) = [h2 | glob | emb | h1], xh2 (B, T, 3H) = [ctx_hat | h1' | h2], h1, c1, h2, c2 (B, T + 1, H), g1, i1, f1, o1, g2, i2,
    f2, o2, sgate, s, ctx, ctx_hat, hc (B, T, H), alpha (B, T, P), beta (B, T), zsc (B, T, P + 1)"""
    w, e = _cast(sd, dtype), _cast(enc, dtype)
    B = e["glob"].shape[0]
    T = tok.shape[1] - 1 if T is None else T
    P = e["Vp"].shape[1]
    a, l = "AdaLSTM.lstm_cell.", "LanguageLSTM."
    w1 = torch.cat([w[a + "weight_ih"], w[a + "weight_hh"]], 1)                                     # on [h2 | glob | emb | h1]
    b1 = w[a + "bias_ih"] + w[a + "bias_hh"]
    w2 = torch.cat([w[l + "weight_ih"], w[l + "weight_hh"]], 1)                                     # on [ctx_hat | h1' | h2]
    b2 = w[l + "bias_ih"] + (w[l + "bias_hh"] if model_bias else w[l + "bias_ih"])                  # :789: bias_ih twice
    wxg, whg = w["AdaLSTM.x_gate.weight"], w["AdaLSTM.h_gate.weight"]
    bg = w["AdaLSTM.x_gate.bias"] + w["AdaLSTM.h_gate.bias"]
    z = functools.partial(_zeros, dtype)
    o = dict(xh1=z(B, T, 2 * E + 2 * H), xh2=z(B, T, 3 * H), alpha=z(B, T, P), beta=z(B, T), zsc=z(B, T, P + 1))
    for k in ("h1", "c1", "h2", "c2"):
        o[k] = z(B, T + 1, H)
        if h0 is not None:
            o[k][:, 0] = h0[k].to(dtype)
    for k in ("g1", "i1", "f1", "o1", "g2", "i2", "f2", "o2", "sgate", "s", "ctx", "ctx_hat", "hc"):
        o[k] = z(B, T, H)
    for t in range(T):
        emb = w["embedding.weight"][tok[:, t]]                                                      # :955
        x1 = torch.cat([o["h2"][:, t], e["glob"], emb], 1)                                          # :957
        xh1 = torch.cat([x1, o["h1"][:, t]], 1)
        h1, c1, g1, i1, f1, o1 = _cell(lin(xh1, w1, b1, order), o["c1"][:, t])                      # :959, :777-784
        hg = h1 if gate_h_new else o["h1"][:, t]                                                    # :982 (h_{t-1}) / :672 (the new h1)
        sgate = torch.sigmoid(lin(torch.cat([x1, hg], 1), torch.cat([wxg, whg], 1), bg, order))
        s = sgate * torch.tanh(c1)                                                                  # :983
        ctx_hat, ctx, alpha, beta, zsc = _adaptive_attention(w, e["Vp"], e["att_img"], h1, s, order)          # :985
        xh2 = torch.cat([ctx_hat, h1, o["h2"][:, t]], 1)                                            # :987
        h2, c2, g2, i2, f2, o2 = _cell(lin(xh2, w2, b2, order), o["c2"][:, t])                      # :988
        o["xh1"][:, t], o["xh2"][:, t] = xh1, xh2
        o["h1"][:, t + 1], o["c1"][:, t + 1], o["h2"][:, t + 1], o["c2"][:, t + 1] = h1, c1, h2, c2
        for k, v in (("g1", g1), ("i1", i1), ("f1", f1), ("o1", o1), ("g2", g2), ("i2", i2), ("f2", f2), ("o2", o2), ("sgate", sgate), ("s", s),
                     ("ctx", ctx), ("ctx_hat", ctx_hat), ("alpha", alpha), ("beta", beta), ("zsc", zsc)):
            o[k][:, t] = v
        o["hc"][:, t] = h2 + ctx_hat                                                                # :990, the fc input
    return o


# ---- AoA ---------------------------------------------------------------------------------------------------------------------------------------
def aoa_fwd(sd, enc, tok, num_head, dtype, order, model_bias, h0=None, T=None):
    """-> xh (B, T, E + 2H) = [emb | glob | h], h, c (B, T + 1, H), g, i, f, o, ctx, lin, c_aoa, sg, hc (B, T, H), alpha (B, T, NH, P), q, gate
    (B, T, H) = q_proj(h'), decoder_aoa_linear_gate(h'), scores (B, T, NH, P)"""
    w, e = _cast(sd, dtype), _cast(enc, dtype)
    B, P, _ = e["key"].shape
    T = tok.shape[1] - 1 if T is None else T
    dk = H // num_head
    l = "LanguageLSTM."
    wc = torch.cat([w[l + "weight_ih"], w[l + "weight_hh"]], 1)                                     # on [emb | glob | h]
    bc = w[l + "bias_ih"] + (w[l + "bias_hh"] if model_bias else w[l + "bias_ih"])                  # :873: bias_ih twice
    kh = e["key"].view(B, P, num_head, dk).transpose(1, 2)                                          # (B, NH, P, dk)
    vh = e["value"].view(B, P, num_head, dk).transpose(1, 2)
    z = functools.partial(_zeros, dtype)
    o = dict(xh=z(B, T, E + 2 * H), h=z(B, T + 1, H), c=z(B, T + 1, H), alpha=z(B, T, num_head, P), scores=z(B, T, num_head, P))
    if h0 is not None:
        o["h"][:, 0], o["c"][:, 0] = h0["h"].to(dtype), h0["c"].to(dtype)
    for k in ("g", "i", "f", "o", "ctx", "lin", "c_aoa", "sg", "hc", "q", "gate"):
        o[k] = z(B, T, H)
    for t in range(T):
        emb = w["embedding.weight"][tok[:, t]]                                                      # :1027
        xh = torch.cat([emb, e["glob"], o["h"][:, t]], 1)                                           # :1030, :1075
        h, c, g, i, f, og = _cell(lin(xh, wc, bc, order), o["c"][:, t])                             # :1033, :861-880
        q = lin(h, w["decoder_multihead_attention.q_proj.weight"], w["decoder_multihead_attention.q_proj.bias"], order)   # :77-85
        qh = q.view(B, num_head, dk)
        scores = tot_last(qh[:, :, None, :] * kh, order) / math.sqrt(dk)                            # (B, NH, P)
        alpha = softmax_last(scores, order)                                                         # :86
        ctx = torch.stack([_pix_sum(vh[:, hd] * alpha[:, hd, :, None], order) for hd in range(num_head)], 1).reshape(B, H)   # :88-90
        gate = lin(h, w["decoder_aoa_linear_gate.weight"], w["decoder_aoa_linear_gate.bias"], order)                         # :1034
        ln = lin(ctx, w["decoder_aoa_linear.weight"], w["decoder_aoa_linear.bias"], order)                                   # :1035
        sg = torch.sigmoid(gate)
        c_aoa = sg * ln                                                                             # :1036
        o["xh"][:, t], o["h"][:, t + 1], o["c"][:, t + 1] = xh, h, c
        for k, v in (("g", g), ("i", i), ("f", f), ("o", og), ("ctx", ctx), ("lin", ln), ("c_aoa", c_aoa), ("sg", sg), ("q", q), ("gate", gate),
                     ("alpha", alpha), ("scores", scores)):
            o[k][:, t] = v
        o["hc"][:, t] = c_aoa + h                                                                   # :1038, the fc input
    return o


# ---- the single-LSTM adaptive-attention model --------------------------------------------------------------------------------------------------
def adaatt_fwd(sd, enc, tok, dtype, order, h0=None, T=None):
    """-> xh (B, T, H + 2E) = [h | emb | glob] (the engine's column order), h, c (B, T + 1, H), g, i, f, o, sgate, s, ctx, ctx_hat, hc (B, T, H),
    alpha (B, T, P), beta (B, T), zsc (B, T, P + 1)"""
    w, e = _cast(sd, dtype), _cast(enc, dtype)
    B = e["glob"].shape[0]
    T = tok.shape[1] - 1 if T is None else T
    P = e["Vp"].shape[1]
    a = "AdaLSTM.lstm_cell."
    wc = torch.cat([w[a + "weight_hh"], w[a + "weight_ih"]], 1)                                     # on [h | emb | glob]
    bc = w[a + "bias_hh"] + w[a + "bias_ih"]                                                        # :557
    wg = torch.cat([w["AdaLSTM.h_gate.weight"], w["AdaLSTM.x_gate.weight"]], 1)
    bg = w["AdaLSTM.x_gate.bias"] + w["AdaLSTM.h_gate.bias"]
    z = functools.partial(_zeros, dtype)
    o = dict(xh=z(B, T, H + 2 * E), h=z(B, T + 1, H), c=z(B, T + 1, H), alpha=z(B, T, P), beta=z(B, T), zsc=z(B, T, P + 1))
    if h0 is not None:
        o["h"][:, 0], o["c"][:, 0] = h0["h"].to(dtype), h0["c"].to(dtype)
    for k in ("g", "i", "f", "o", "sgate", "s", "ctx", "ctx_hat", "hc"):
        o[k] = z(B, T, H)
    for t in range(T):
        emb = w["embedding.weight"][tok[:, t]]                                                      # :594-595
        xh = torch.cat([o["h"][:, t], emb, e["glob"]], 1)                                           # :598 x_t = [emb | glob], and h_{t-1}
        h, c, g, i, f, og = _cell(lin(xh, wc, bc, order), o["c"][:, t])                             # :601, :554-565
        sgate = torch.sigmoid(lin(xh, wg, bg, order))                                               # :602: x_gate(x_t) + h_gate(h_{t-1})
        s = sgate * torch.tanh(c)                                                                   # :603
        ctx_hat, ctx, alpha, beta, zsc = _adaptive_attention(w, e["Vp"], e["att_img"], h, s, order)          # :604, :56-98
        o["xh"][:, t], o["h"][:, t + 1], o["c"][:, t + 1] = xh, h, c
        for k, v in (("g", g), ("i", i), ("f", f), ("o", og), ("sgate", sgate), ("s", s), ("ctx", ctx), ("ctx_hat", ctx_hat), ("alpha", alpha),
                     ("beta", beta), ("zsc", zsc)):
            o[k][:, t] = v
        o["hc"][:, t] = ctx_hat + h                                                                 # :134, the fc input
    return o


# ---- LRP-inference re-weighting ----------------------------------------------------------------------------------------------------------------
def lrp_reweight(pred, h, ctx, fcw, skip, log_softmax, dtype, order="torch"):
    """get_lrp_weight_step (gridTDmodel.py:548-577; aoamodel.py:597-626 hands it log_softmax(pred), :721-723) + the re-weighted fc input (:687),
    row by row.  pred (R, V) fp32 (the arg-max is taken on it, whatever `dtype`), h, ctx (R, H) the two fc summands, skip (V,) bool.
    -> hcw (R, H) = ctx * w_ctx + w_h * h, k (R,), w_h, w_ctx (R, H)"""
    R = pred.shape[0]
    fcw = fcw.to(dtype)
    hcw, wh_, wc_, ks = _zeros(dtype, R, H), _zeros(dtype, R, H), _zeros(dtype, R, H), []
    for r in range(R):
        k = int(torch.argmax(pred[r]))                                                              # :553 (first maximum)
        ks.append(k)
        hr, cr, p = h[r].to(dtype), ctx[r].to(dtype), pred[r].to(dtype)
        if bool(skip[k]):                                                                           # :557-558 stop words and specials: weights of 1
            wh_[r], wc_[r] = 1, 1
        else:
            pk = p[k]
            if log_softmax:
                pk = -torch.log(tot(torch.exp(p - p[k]), order))                                    # log_softmax(pred)[k], p[k] the maximum
            hc = hr + cr
            r_hc = fcw[k] * hc / stab(pk) * pk                                                      # :560-566 one-hot epsilon rule through fc
            r_h, r_c = hr / stab(hc) * r_hc, cr / stab(hc) * r_hc                                   # :567-572
            mh, mc = r_h.abs().max(), r_c.abs().max()
            wh_[r] = r_h / (mh if mh != 0 else 1) + 1                                               # LRPtools/utils.py:55-64
            wc_[r] = r_c / (mc if mc != 0 else 1) + 1
        hcw[r] = cr * wc_[r] + wh_[r] * hr                                                          # :687
    return hcw, torch.tensor(ks), wh_, wc_


# ---- the planted models -------------------------------------------------------------------------------------------------------------------------
V_DRAW = 203
FEAT_DRAW = 64
# (hidden unit, gate, pre-activation): gates 0 - 3 = i, f, g, o of every LSTM cell, 4 = the sentinel gate (AdaAtt's fifth gate row) and AoA's
# decoder_aoa_linear_gate.  +-100 under a sigmoid, +-50 under the tanh of g, and an exact 0 (weight rows and biases zeroed).  Units 3 and 7
# close a four-unit interleave group (gridTD, AoA), 2 and 5 a three-unit one (AdaAtt); 511 = H - 1 (in AdaAtt's last, two-unit, group).
PLANTS = [(3, 0, 100.), (7, 0, -100.), (2, 0, 0.), (5, 1, 100.), (511, 1, -100.), (510, 1, 0.), (100, 2, 50.), (257, 2, -50.), (258, 2, 0.),
          (259, 3, 100.), (260, 3, -100.), (263, 3, 0.), (261, 4, 100.), (262, 4, -100.), (11, 4, 0.), (509, 4, 100.)]
C0_PLANTS = {8: 0.0, 9: -0.0, 10: 50.0, 12: -50.0, 13: 0.004, 14: -0.004}          # c[0] of every image
ATT_VARIANTS = ("hi", "lo", "over")          # peaked (+-40) with the sentinel score above / below every pixel score; scores past +-89
ATT_TOTAL, ATT_AMP, OVER_WH, OVER_AMP = 44.0, 1.2, 4.0, 6.0


def _plant_rows(sd, w_names, b_names, row, val):
    """the pre-activation of `row` becomes val (+- what the weights add), or exactly 0: weight rows zeroed"""
    for n in b_names:
        sd[n][row] = val / len(b_names)
    if val == 0:
        for n in w_names:
            sd[n][row] = 0.0


def _plant_gates(sd, cells, gate5):
    for unit, q, val in PLANTS:
        if q < 4:
            for c in cells:
                _plant_rows(sd, (c + ".weight_ih", c + ".weight_hh"), (c + ".bias_ih", c + ".bias_hh"), q * H + unit, val)
        else:
            _plant_rows(sd, [n + ".weight" for n in gate5], [n + ".bias" for n in gate5], unit, val)


def _plant_attention(sd, variant):
    """w_h scaled so that sum |w_h| = 44 (peaked: the scores of `draw`'s att_img span about +-40) or |w_h| = 4 (over: +-4 P with saturated
    tanh); W_s_proj.bias = +-3 sign(w_h): the sentinel score is +-0.995 x 44, above / below every pixel score"""
    import numpy as np
    wh = sd["AdaAttention.w_h.weight"]
    sign = np.where(wh < 0, -1.0, 1.0).astype(np.float32)
    if variant == "over":
        sd["AdaAttention.w_h.weight"] = sign * OVER_WH
    else:
        sd["AdaAttention.w_h.weight"] = (wh * (ATT_TOTAL / np.abs(wh).sum())).astype(np.float32)
        sd["AdaAttention.W_s_proj.bias"] = (3.0 if variant == "hi" else -3.0) * sign[0]


@functools.lru_cache(maxsize=None)
def np_state(model, P, variant):
    """the planted small-V model (numpy, as lrp_amd.weights makes it) the kernel tests build their engine from.  model: gridtd (bottom-up: no
    encoder), aoa, adaatt; P: pixels (the attention's width; AoA: any); variant: ATT_VARIANTS (AoA: ignored, `draw` scales the keys)"""
    from lrp_amd import weights
    if model == "gridtd":
        sd = weights.make_gridtd_bu_state(seed=5, vocab_size=V_DRAW, feat_dim=FEAT_DRAW, num_pixels=P)
        _plant_gates(sd, ("AdaLSTM.lstm_cell", "LanguageLSTM"), ("AdaLSTM.x_gate", "AdaLSTM.h_gate"))
        _plant_attention(sd, variant)
    elif model == "adaatt":
        sd = weights.make_adaatt_state(seed=5, vocab_size=V_DRAW, feat_dim=FEAT_DRAW, num_pixels=P, encoder=None)
        _plant_gates(sd, ("AdaLSTM.lstm_cell",), ("AdaLSTM.x_gate", "AdaLSTM.h_gate"))
        _plant_attention(sd, variant)
    else:
        sd = weights.make_aoa_state(seed=5, vocab_size=V_DRAW, feat_dim=FEAT_DRAW, with_encoder=False)
        _plant_gates(sd, ("LanguageLSTM",), ("decoder_aoa_linear_gate",))
    return sd


@functools.lru_cache(maxsize=None)
def state(model, P, variant):
    return {k: torch.from_numpy(v) for k, v in np_state(model, P if model != "aoa" else 0, variant if model != "aoa" else "").items()}


def engine_state(model, P, variant):
    return np_state(model, P if model != "aoa" else 0, variant if model != "aoa" else "")


# ---- the drawn inputs ---------------------------------------------------------------------------------------------------------------------------
# draws that missed the yardstick condition (tests/test_decoder_fwd_restate_host.py) and were drawn again: (model, P, variant, B, T) -> how often
RESEED = {}
AOA_SPAN = {0: 40.0, 4: 100.0, 7: 1e-3}          # max |scaled score| of the heads whose keys `draw` scales (the others: as drawn, below 1)


def draw_tokens(B, T, gen):
    """(B, T + 3) ids: `tok_ld` != T + 1; ids 0 and V - 1 as inputs and as targets, one id repeated"""
    tok = torch.randint(1, V_DRAW - 3, (B, T + 3), generator=gen)
    tok[0, 0] = 0
    tok[0, 1] = V_DRAW - 1
    if T >= 2:
        tok[0, 2] = 0
    tok[B - 1, 1] = tok[B - 1, 0]
    return tok


def draw_state(B, names, gen):
    """h: 0.5 randn, c: randn with the C0_PLANTS entries"""
    h0 = {}
    for k in names:
        x = torch.randn(B, H, generator=gen)
        if k.startswith("h"):
            x = 0.5 * x
        else:
            for u, v in C0_PLANTS.items():
                x[:, u] = v
        h0[k] = x
    return h0


@functools.lru_cache(maxsize=None)
def draw(model, P, variant, B, T, zero_state=False):
    """(enc, tok, h0) of a case: the image-side constants the decoder kernels read (encoder GEMMs stay out of these tests), token ids, and a
    drawn initial state.  gridtd / adaatt: att_img[b, k, :] = amp u_k sign(w_h) + 0.3 randn, u a permutation of linspace(-1, 1, P): pixel score
    k is about tanh(amp u_k) sum |w_h|.  aoa: key = randn, the heads of AOA_SPAN scaled to that largest |score| (of the trace from h0, or from
    zeros: zero_state); value >= 0 in image 0, <= 0 in the others."""
    seed = 2000 + 101 * P + 7 * B + 13 * T + 1000 * (ATT_VARIANTS + ("",)).index(variant if model != "aoa" else "") \
        + 50000 * ("gridtd", "aoa", "adaatt").index(model) + 1000000 * RESEED.get((model, P, variant, B, T), 0)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    tok = draw_tokens(B, T, gen)
    if model == "aoa":
        key = rnd(B, P, H)
        dk = H // NH_DRAW
        value = torch.relu(rnd(B, P, H)) + 0.01
        value[1:] = -value[1:]
        enc = dict(glob=torch.relu(rnd(B, H)), key=key, value=value)
        h0 = draw_state(B, ("h", "c"), gen)
        # the attention feeds nothing back into the recurrence: the queries are those of the unit keys, whatever the scale of a head
        unit = aoa_fwd(state("aoa", 0, ""), enc, tok, NH_DRAW, torch.float64, "torch", False, None if zero_state else h0, T)["scores"]
        unit = unit.abs().amax(dim=(0, 1, 3))
        for hd, target in AOA_SPAN.items():
            key[:, :, hd * dk:(hd + 1) * dk] *= float(target * (2.0 if variant == "over" else 1.0) / unit[hd])
        return enc, tok, h0
    sign = torch.sign(state(model, P, variant)["AdaAttention.w_h.weight"][0])
    amp = OVER_AMP if variant == "over" else ATT_AMP
    u = torch.stack([torch.linspace(-1, 1, P)[torch.randperm(P, generator=gen)] for _ in range(B)])          # (B, P)
    att_img = amp * u[:, :, None] * sign[None, None, :] + 0.3 * rnd(B, P, P)
    enc = dict(glob=torch.relu(rnd(B, E)), Vp=torch.relu(rnd(B, P, H)), att_img=att_img)
    return enc, tok, draw_state(B, ("h1", "c1", "h2", "c2") if model == "gridtd" else ("h", "c"), gen)


def run(model, sd, enc, tok, dtype, order, T=None, h0=None, model_bias=False, gate_h_new=False):
    if model == "gridtd":
        return gridtd_fwd(sd, enc, tok, dtype, order, model_bias, gate_h_new, h0, T)
    if model == "aoa":
        return aoa_fwd(sd, enc, tok, NH_DRAW, dtype, order, model_bias, h0, T)
    return adaatt_fwd(sd, enc, tok, dtype, order, h0, T)


@functools.lru_cache(maxsize=None)
def references(model, P, variant, B, T, model_bias=False, gate_h_new=False, zero_state=False):
    """(fp64 evaluation, [fp32 evaluation per order in ORDERS]) of a case - computed once per process.  zero_state: from h = c = 0, as the
    engines' `trace` starts"""
    enc, tok, h0 = draw(model, P, variant, B, T, zero_state)
    sd = state(model, P, variant)
    f = lambda dtype, order: run(model, sd, enc, tok, dtype, order, T, None if zero_state else h0, model_bias, gate_h_new)
    return f(torch.float64, "torch"), [f(torch.float32, o) for o in ORDERS]


# every case the kernel tests run: (model, P, variant, B, T, model_bias, gate_h_new, zero_state)
MODELS = ("gridtd", "aoa", "adaatt")
STEP_P = (5, 36, 67, 196)
STEP_VARIANT = {5: "hi", 36: "lo", 67: "hi", 196: "lo"}
B_SWEEP = (1, 17, 33, 49, 64, 65)


def step_cases():
    """one step from a drawn state: B = 2, a T = 1 reference (the kernels run it as step t = 2 of a T = 4 trace)"""
    out = []
    for m in MODELS:
        for P in STEP_P:
            out.append((m, P, STEP_VARIANT[P], 2, 1, False, False, False))
            if m == "gridtd":
                out.append((m, P, STEP_VARIANT[P], 2, 1, True, True, False))
    return out


def trace_cases():
    out = []
    for m in MODELS:
        out += [(m, 36, "hi", 2, 3, False, False, False), (m, 36, "lo", 2, 11, False, False, False), (m, 36, "over", 2, 3, False, False, False),
                (m, 36, "hi", max(B_SWEEP), 2, False, False, False)]
    return out


def engine_cases():
    out = []
    for m in MODELS:
        for mb in ((False, True) if m != "adaatt" else (False,)):
            out.append((m, 36, "hi", 2, 3, mb, False, True))
    return out


def all_cases():
    return step_cases() + trace_cases() + engine_cases()
