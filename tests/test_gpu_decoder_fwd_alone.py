"""The decoder FORWARD kernels of csrc/decoder_blocks.hip, csrc/decoder_gridtd.hip, csrc/decoder_aoa.hip and csrc/lrpx_adaatt.hip ALONE, through the C ABI, against the fp64 restatements of
tests/decoder_fwd_restate.py: the building blocks (`lrpx_linear_small` at every row tile and on both kernels, `lrpx_mean_pixels`, `lrpx_relu`,
`lrpx_target_logit`, the two arg-max kernels), one decoder step of each model from a drawn state, whole traces through every path (per-step,
fused, decoupled), the recorded row maxima, the engines' `trace`, and the LRP-inference re-weighting.  The kernels receive the engine's OWN packed
and interleaved tensors (`Wcat1_il`, `W_hh_il`, `tok_table`, AdaAtt's 16-row groups); the restatement receives the raw state dict.  The models
are planted (decoder_fwd_restate.py): peaked attention (+-40), a draw whose scores pass +-89, the sentinel above / below every pixel score,
AoA heads spanning +-40, +-100 and 0, gate pre-activations of +-100, +-50 and exact 0 (interleave-group ends and unit H - 1 among them), token
ids 0 and V - 1, `tok_ld` = T + 3, a drawn initial state with +-0, +-50, +-0.004 in c.  Every trace buffer starts as NaN (but `_amax[1]`, which
the API has the caller zero); flat outputs carry a 4096-float guard.

Bounds.  Integer outputs and copies are exact.  Everything else: `fp64_anchor.fp32_grade` with the project's C = 6 and FLOOR = 1e-7 against the
WORST of three plain fp32 evaluations in different summation orders (tests/test_decoder_fwd_restate_host.py holds every draw to the condition that
makes this a fair yardstick).  alpha rows and the [alpha, beta] softmax sum to 1 within 4 P 2^-24 and hold no NaN / inf.  The fp16-split GEMMs
of the decoupled AoA engine trace (`force_f16`): 1e-4 of the maximum, as tests/test_gpu_t20.py holds that arithmetic.

Worst e / max(e32, FLOOR) per family and kernel group over all cases and tensors, first MI355X run (the bound is 6):
  building blocks   linear_small 1.02, mean_pixels 0.59, target_logit 1.29, argmax_logprob 1.01, lrp_reweight 1.00
  gridTD            one step 1.11; whole traces, interleaved rows and rows left null alike 1.67 (scores past +-89: 1.05); engine trace 1.83
  AoA               one step 1.58 (the decoupled path's kernels on it 2.17); lrpx_aoa_fwd_steps fused and not fused 1.29 (past +-89: 0.64);
                    decoupled from a host zin 1.48 (0.71), from the token table 2.08 (0.67); engine trace 2.03
  AdaAtt            one step 2.98; step loop 1.73, decoupled 1.44 (past +-89: 1.00 both); engine trace 1.51
  f16 split GEMMs of the decoupled AoA engine trace: at worst 1.3e-6 of the maximum (logit; alpha 1.1e-6) against the 1e-4 bound - 2.2 x
                    the fp32 yardstick (ctx), every other tensor below 2.0 x
No kernel missed a check: no defect found.  The ten mutations of the issue, each built into a library of its own and not committed; every
one turned tests red:
   1 `- m` dropped from the expf of att_context_block: test_whole_trace_vs_fp64[gridtd-over-3] and [adaatt-over-3] (NaN) - the draws whose
     scores pass +-89, and no other test
   2 m2 -> m in beta, 3 `k <= P` -> `k < P` in denom2: the same 28 tests each - wherever the sentinel score is above every pixel score
     (variant hi): test_one_step_from_a_drawn_state at P = 5 and 67 (gridTD, both sentinel gates, and AdaAtt), test_whole_trace_vs_fp64
     [gridtd-hi-3] and [adaatt-hi-3], test_every_row_tile_vs_fp64 (gridTD, AdaAtt: every B), test_gridtd_engine_trace, test_adaatt_engine_trace
   4 (1 - beta) -> beta in ctx_hat, 5 sv and hv swapped in the call of att_scores_block: every gridTD and AdaAtt case of
     test_one_step_from_a_drawn_state, test_whole_trace_vs_fp64, test_every_row_tile_vs_fp64 and both engine-trace tests (38 tests each)
   6 `* inv` dropped in aoa_fwd_attention_all_kernel only, 8 z[1] and z[0] swapped in aoa_rec_lstm_kernel only, 9 `+ gi[col]` dropped:
     the same 18 tests each, all on the decoupled path - test_one_step_from_a_drawn_state[aoa-*] (its decoupled-kernels part), every AoA case of
     test_whole_trace_vs_fp64 and test_every_row_tile_vs_fp64, test_aoa_engine_trace[decoupled-*], test_aoa_engine_trace_f16_split_gemms
   7 fabsf dropped from ctx_amax: test_row_maxima_are_recorded, the AoA cases of test_whole_trace_vs_fp64 and of test_every_row_tile_vs_fp64
     with more than one image (B = 1 holds image 0 alone, whose value rows are positive)
  10 `if (mh == 0.f)` dropped in lrp_reweight_kernel: all four test_lrp_reweight_vs_fp64 cases (NaN in the zero-logit row and the h = 0 row)
What the path through `lrpx_adaatt_fwd_inputs` does not write: xh[b, 0][:H] (the engine's trace is zero there, as h[0] is); it stays NaN here.
Every deviation is printed before it is asserted."""
import ctypes as C
import math

import pytest
import torch

import lrp_amd  # noqa: F401
import decoder_fwd_restate as F
from conftest import rel_err
from fp64_anchor import FLOOR, fp32_grade

pytestmark = pytest.mark.gpu

H = E = F.H
NH = F.NH_DRAW
V = F.V_DRAW
GUARD = 4096
NAN = float("nan")
_ENGINES = {}
WORST = {}


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------
def _engine(model, P=36, variant="hi"):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    key = (model, P if model != "aoa" else 0, variant if model != "aoa" else "")
    if key not in _ENGINES:
        sd = F.engine_state(model, P, variant)
        if model == "gridtd":
            from lrp_amd.explainers.gridtd import GridTDBUEngine
            eng = GridTDBUEngine(sd)
            assert eng.fused_steps and eng.P == P
        elif model == "aoa":
            from lrp_amd.explainers.aoa import AOAEngine
            eng = AOAEngine(sd, num_head=NH)
            assert eng.cnn is None and eng.decoupled and eng.tok_table is not None
        else:
            from lrp_amd.explainers.adaatt import AdaAttEngine
            eng = AdaAttEngine(sd)
            assert eng.P == P
        _ENGINES[key] = eng
    return _ENGINES[key]


def _lib():
    from lrp_amd import _lib
    return _lib.load(), _lib.stream_ptr()


def _ptr(t):
    from lrp_amd._lib import ptr
    return ptr(t)


def _ptr_at(t, off):
    from lrp_amd._lib import ptr_at
    return ptr_at(t, off)


def _check(rc):
    from lrp_amd._lib import check
    check(rc)


def _nan(*s):
    return torch.full(s, NAN, device="cuda")


def _guarded(n, fill=777.0):
    return torch.full((n + GUARD,), fill, device="cuda")


def _guard_ok(buf, n, what):
    assert bool((buf[n:] == 777.0).all()), what + ": written behind the output"
    return buf[:n]


def _bits(a, b):
    """bit for bit, NaN left by nobody included"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _note(group, ratio):
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    print("WORST %s so far: %.2f" % (group, WORST[group]))


def _grade(group, what, got, ref64, refs32, keys, sel=lambda k, v: v):
    """every tensor of `keys` against fp64: fp32 grade against the worst fp32 order.  sel(key, tensor): the part of a reference tensor that is
    compared (the kernels' tensor `got[k]` has that shape)"""
    worst = 0.0
    for k in keys:
        g = got[k].detach().cpu()
        r64 = sel(k, ref64[k])
        assert tuple(g.shape) == tuple(r64.shape), (what, k, tuple(g.shape), tuple(r64.shape))
        assert not torch.isnan(g).any() and not torch.isinf(g).any(), (what, k, "NaN / inf")
        errs = [rel_err(sel(k, r[k]), r64) for r in refs32]
        r32 = sel(k, refs32[errs.index(max(errs))][k])
        e, e32, _, _ = fp32_grade(g, r64, r32, r32, "%s %s" % (what, k), margin_min=0)
        worst = max(worst, e / max(e32, FLOOR))
    _note(group, worst)
    return worst


def _softmax_sums(what, alpha, beta, P):
    """each alpha row, and the [alpha (1 - beta), beta] softmax it stands for, sums to 1 within 4 P 2^-24; no NaN / inf"""
    a = alpha.detach().cpu().double()
    assert torch.isfinite(a).all() and (a >= 0).all(), what
    d = float((a.sum(-1) - 1).abs().max())
    bound = 4 * P * 2.0 ** -24
    print("%s: alpha rows sum to 1 within %.2e (bound %.2e)" % (what, d, bound))
    assert d <= bound, (what, d)
    if beta is not None:
        b = beta.detach().cpu().double()
        assert torch.isfinite(b).all() and (b >= 0).all() and (b <= 1).all(), what
        d2 = float((a.sum(-1) * (1 - b) + b - 1).abs().max())
        print("%s: [alpha, beta] sums to 1 within %.2e" % (what, d2))
        assert d2 <= bound, (what, d2)


def _dev(enc, B):
    return {k: v[:B].cuda().contiguous() for k, v in enc.items()}


STATE = {"gridtd": ("h1", "c1", "h2", "c2"), "aoa": ("h", "c"), "adaatt": ("h", "c")}
STEPWISE = {"gridtd": ("g1", "i1", "f1", "o1", "g2", "i2", "f2", "o2", "sgate", "s", "ctx", "ctx_hat", "hc", "alpha", "beta"),
            "aoa": ("g", "i", "f", "o", "ctx", "lin", "c_aoa", "sg", "hc", "alpha"),
            "adaatt": ("g", "i", "f", "o", "sgate", "s", "ctx", "ctx_hat", "hc", "alpha", "beta")}
INPUT_ROWS = {"gridtd": ("xh1", "xh2"), "aoa": ("xh",), "adaatt": ("xh",)}


def _trace(model, eng, B, T, P, state=None, slot=0):
    """a trace of NaN (the gradient explainers' tensors included), the state `state` in slot `slot`"""
    if model == "gridtd":
        tr = eng._alloc_trace(B, T, grad=True)
    elif model == "aoa":
        tr = eng._alloc_trace(B, T, P, grad=True)
    else:
        tr = eng._alloc_trace(B, T)
        tr["o"], tr["sgate"] = torch.empty(B, T, H, device="cuda"), torch.empty(B, T, H, device="cuda")
        tr["_c"].o, tr["_c"].sgate = _ptr(tr["o"]), _ptr(tr["sgate"])
    for k, v in tr.items():
        if torch.is_tensor(v) and v.is_floating_point():
            v.fill_(NAN)
    if model == "aoa":
        tr["_amax"][1].zero_()          # ctx_amax: an atomicMax over the heads into a buffer the caller zeroes
    if state is not None:
        for k in STATE[model]:
            tr[k][:, slot] = state[k][:B].cuda()
    return tr


def _tensors(model, tr):
    return {k: tr[k] for k in STATE[model] + STEPWISE[model] + INPUT_ROWS[model]}


def _copies_exact(model, tr, enc, tok, emb, T, first_h_row=True):
    """the input rows are copies: bit for bit the state, the global feature and the embedding row they were gathered from"""
    B = tok.shape[0]
    e = emb[tok[:, :T]]
    glob = enc["glob"][:, None].expand(B, T, enc["glob"].shape[1])
    if model == "gridtd":
        want1 = torch.cat([tr["h2"][:, :T], glob, e, tr["h1"][:, :T]], 2)
        want2 = torch.cat([tr["ctx_hat"], tr["h1"][:, 1:], tr["h2"][:, :T]], 2)
        assert _bits(tr["xh1"], want1), "xh1 is not [h2 | glob | emb | h1]"
        assert _bits(tr["xh2"], want2), "xh2 is not [ctx_hat | h1' | h2]"
    elif model == "aoa":
        assert _bits(tr["xh"], torch.cat([e, glob, tr["h"][:, :T]], 2)), "xh is not [emb | glob | h]"
    else:
        want = torch.cat([tr["h"][:, :T], e, glob], 2)
        t0 = 0 if first_h_row else 1
        assert _bits(tr["xh"][:, :, H:], want[:, :, H:]) and _bits(tr["xh"][:, t0:, :H], want[:, t0:, :H]), "xh is not [h | emb | glob]"


# ---- a. the building blocks ------------------------------------------------------------------------------------------------------------------
LINEAR = [(1, 4, 1), (3, 20, 5), (16, 36, 19), (16, 512, 16), (17, 512, 33), (33, 1536, 49), (48, 2048, 80), (64, 512, 2560), (65, 512, 35)]


@pytest.mark.parametrize("B, K, N", LINEAR, ids=lambda v: str(v))
def test_linear_small_vs_fp64(B, K, N):
    """K % 16 != 0 and B > 64 take the VALU kernel (B = 65: a last row chunk of one), the others the matrix-core kernel at RT = 1, 2, 3, 4"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib, st = _lib()
    gen = torch.Generator().manual_seed(100 * B + K + N)
    ldx, ldo = K + 4, N + 3
    x = torch.randn(B, ldx, generator=gen)
    w, bias = torch.randn(N, K, generator=gen) / math.sqrt(K), torch.randn(N, generator=gen)
    xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
    for use_bias in (True, False):
        for act in (0, 1):
            buf = _guarded(B * ldo)
            _check(lib.lrpx_linear_small(_ptr(xd), ldx, _ptr(wd), _ptr(bd) if use_bias else None, _ptr(buf), ldo, B, K, N, act, st))
            torch.cuda.synchronize()
            out = _guard_ok(buf, B * ldo, "linear_small").view(B, ldo)
            assert bool((out[:, N:] == 777.0).all()), "linear_small wrote the padding columns of out"
            b_ = bias if use_bias else None
            ref64 = F.linear(x[:, :K], w, b_, act, torch.float64, "torch")
            refs32 = [F.linear(x[:, :K], w, b_, act, torch.float32, o) for o in F.ORDERS]
            _grade("linear_small", "linear_small (%d, %d, %d) bias %s act %d" % (B, K, N, use_bias, act), dict(out=out[:, :N]), dict(out=ref64),
                   [dict(out=r) for r in refs32], ("out",))


@pytest.mark.parametrize("P, Cc", [(1, 64), (3, 100), (36, 2048), (197, 192)], ids=lambda v: str(v))
def test_mean_pixels_vs_fp64(P, Cc):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib, st = _lib()
    B = 2
    f = torch.relu(torch.randn(B, P, Cc, generator=torch.Generator().manual_seed(P + Cc)))
    buf = _guarded(B * Cc)
    fd = f.cuda()
    _check(lib.lrpx_mean_pixels(_ptr(fd), _ptr(buf), B, P, Cc, st))
    torch.cuda.synchronize()
    out = _guard_ok(buf, B * Cc, "mean_pixels").view(B, Cc)
    _grade("mean_pixels", "mean_pixels (%d, %d)" % (P, Cc), dict(avg=out), dict(avg=F.mean_pixels(f, torch.float64, "torch")),
           [dict(avg=F.mean_pixels(f, torch.float32, o)) for o in F.ORDERS], ("avg",))


def test_relu_is_exact():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib, st = _lib()
    n = 257
    x = torch.randn(n, generator=torch.Generator().manual_seed(1))
    x[0], x[1], x[255], x[256] = -0.0, 0.0, -3.0, 2.5
    buf = _guarded(n)
    xd = x.cuda()
    _check(lib.lrpx_relu(_ptr(xd), _ptr(buf), n, st))
    torch.cuda.synchronize()
    y = _guard_ok(buf, n, "relu").cpu()
    assert torch.equal(y, torch.relu(x)) and float(y[0]) == 0.0 and float(y[256]) == 2.5


@pytest.mark.parametrize("B, T", [(1, 1), (5, 1), (2, 4)], ids=lambda v: str(v))
def test_target_logit_vs_fp64(B, T):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib, st = _lib()
    gen = torch.Generator().manual_seed(7 * B + T)
    hc, fcw, fcb = torch.randn(B, T, H, generator=gen), torch.randn(V, H, generator=gen) / math.sqrt(H), torch.randn(V, generator=gen)
    tok = torch.randint(1, V - 1, (B, T + 3), generator=gen)
    tok[0, 1] = 0                       # the first row's target: id 0 ...
    tok[B - 1, T] = V - 1               # ... the last row's: id V - 1
    if B * T == 1:
        tok[0, 1] = V - 1
    buf = _guarded(B * T)
    dev = [x.cuda() for x in (hc, fcw, fcb, tok)]          # (kept alive until the kernel has run)
    _check(lib.lrpx_target_logit(_ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), T + 3, _ptr(buf), B, T, H, st))
    torch.cuda.synchronize()
    out = _guard_ok(buf, B * T, "target_logit")
    _grade("target_logit", "target_logit B T = %d" % (B * T), dict(logit=out), dict(logit=F.target_logit(hc, fcw, fcb, tok, torch.float64, "torch")),
           [dict(logit=F.target_logit(hc, fcw, fcb, tok, torch.float32, o)) for o in F.ORDERS], ("logit",))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 10004])
def test_argmax_rows_and_logprob(n):
    """rows: a tie between the first and the last column (the first wins), the maximum in the last column, one repeated value, a row with
    -inf, a plain row.  `ld` > n, the padding above every value: a read past n would win"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib, st = _lib()
    gen = torch.Generator().manual_seed(n)
    rows, ld = 5, n + 5
    x = torch.full((rows, ld), 1e30)
    x[:, :n] = torch.randn(rows, n, generator=gen)
    x[0, 0] = x[0, n - 1] = 9.0
    x[1, n - 1] = 11.0
    x[2, :n] = -1.25
    if n > 1:
        x[3, n // 2] = float("-inf")
    want = torch.argmax(x[:, :n], -1)
    assert want.tolist()[:3] == [0, n - 1, 0]
    xd = x.cuda()
    idx1, idx2 = (torch.full((rows + 8,), -7, dtype=torch.int64, device="cuda") for _ in range(2))
    lp = _guarded(rows)
    _check(lib.lrpx_argmax_rows(_ptr(xd), ld, rows, n, _ptr(idx1), st))
    _check(lib.lrpx_argmax_logprob_rows(_ptr(xd), ld, rows, n, _ptr(idx2), _ptr(lp), st))
    torch.cuda.synchronize()
    for idx in (idx1, idx2):
        assert idx[:rows].cpu().tolist() == want.tolist() and bool((idx[rows:] == -7).all()), (idx.tolist(), want.tolist())
    got = _guard_ok(lp, rows, "argmax_logprob_rows")
    ref64 = F.argmax_logprob(x[:, :n], torch.float64, "torch")[1]
    if n == 1:          # log_softmax of one score: exactly 0
        assert torch.count_nonzero(got) == 0 and torch.count_nonzero(ref64) == 0
        return
    _grade("argmax_logprob", "argmax_logprob_rows n = %d" % n, dict(lp=got), dict(lp=ref64),
           [dict(lp=F.argmax_logprob(x[:, :n], torch.float32, o)[1]) for o in F.ORDERS], ("lp",))


# ---- the steps of the three decoders through the C ABI ----------------------------------------------------------------------------------------
def _att_args(eng):
    sd, aa = eng.sd, "AdaAttention."
    return [sd[aa + "W_g_proj.weight"], sd[aa + "W_s_proj.weight"], sd[aa + "W_s_proj.bias"], sd[aa + "w_h.weight"]]


def _gridtd_step(eng, tr, enc, t, tok, model_bias, gate_h_new, scr):
    """`GridTDEngine._step`: the seven launches of a decoder step (+ the three of the sentinel gate on the new h1)"""
    lib, st = _lib()
    B, T = tr["B"], tr["T"]
    c = C.byref(tr["_c"])
    W1 = 2 * E + 2 * H
    zz1, zz2 = _nan(B, 5 * H), _nan(B, 4 * H)
    _check(lib.lrpx_gridtd_fwd_pre(c, t, _ptr(enc["glob"]), _ptr(eng.sd["embedding.weight"]), _ptr(tok), tok.shape[1], st))
    _check(lib.lrpx_linear_small(_ptr_at(tr["xh1"], t * W1), T * W1, _ptr(eng.Wcat1), _ptr(eng.bcat1), _ptr(zz1), 5 * H, B, W1, 5 * H, 0, st))
    _check(lib.lrpx_gridtd_fwd_lstm(c, t, _ptr(zz1), 5 * H, 1, st))
    if gate_h_new:
        xg, zg = _nan(B, W1), _nan(B, H)
        w_gate, b_gate = eng.Wcat1[4 * H:], eng.bcat1[4 * H:]
        _check(lib.lrpx_gridtd_fwd_gate_input(c, t, _ptr(xg), st))
        _check(lib.lrpx_linear_small(_ptr(xg), W1, _ptr(w_gate), _ptr(b_gate), _ptr(zg), H, B, W1, H, 0, st))
        _check(lib.lrpx_gridtd_fwd_sentinel(c, t, _ptr(zg), H, st))
    wg, ws, bs, wh = _att_args(eng)
    _check(lib.lrpx_gridtd_fwd_attention(c, t, _ptr(enc["Vp"]), _ptr(enc["att_img"]), _ptr(wg), _ptr(ws), _ptr(bs), _ptr(wh), _ptr(scr), st))
    b2 = eng.bcat2_model if model_bias else eng.bcat2_explainer
    _check(lib.lrpx_linear_small(_ptr_at(tr["xh2"], t * 3 * H), T * 3 * H, _ptr(eng.Wcat2), _ptr(b2), _ptr(zz2), 4 * H, B, 3 * H, 4 * H, 0, st))
    _check(lib.lrpx_gridtd_fwd_lstm(c, t, _ptr(zz2), 4 * H, 2, st))


def _aoa_step(eng, tr, enc, t, tok, model_bias):
    """`AOAEngine._step`: the seven launches of a decoder step (the 256-thread attention kernel)"""
    lib, st = _lib()
    B, T = tr["B"], tr["T"]
    c = C.byref(tr["_c"])
    W = E + 2 * H
    zz, qg, ln = _nan(B, 4 * H), _nan(B, 2 * H), _nan(B, H)
    bias = eng.bcat_model if model_bias else eng.bcat_explainer
    _check(lib.lrpx_aoa_fwd_pre(c, t, _ptr(enc["glob"]), _ptr(eng.sd["embedding.weight"]), _ptr(tok), tok.shape[1], st))
    _check(lib.lrpx_linear_small(_ptr_at(tr["xh"], t * W), T * W, _ptr(eng.Wcat), _ptr(bias), _ptr(zz), 4 * H, B, W, 4 * H, 0, st))
    _check(lib.lrpx_aoa_fwd_lstm(c, t, _ptr(zz), 4 * H, st))
    _check(lib.lrpx_linear_small(_ptr_at(tr["h"], (t + 1) * H), (T + 1) * H, _ptr(eng.Wqg), _ptr(eng.bqg), _ptr(qg), 2 * H, B, H, 2 * H, 0, st))
    _check(lib.lrpx_aoa_fwd_attention(c, t, _ptr(qg), 2 * H, _ptr(enc["key"]), _ptr(enc["value"]), st))
    _check(lib.lrpx_linear_small(_ptr_at(tr["ctx"], t * H), T * H, _ptr(eng.sd["decoder_aoa_linear.weight"]), _ptr(eng.sd["decoder_aoa_linear.bias"]),
                                 _ptr(ln), H, B, H, H, 0, st))
    _check(lib.lrpx_aoa_fwd_post(c, t, _ptr(qg), 2 * H, _ptr(ln), st))


def _rows_linear(x, w, bias, n):
    """x (R, K) @ w^T + bias through lrpx_linear_small (exact fp32 products), any R"""
    lib, st = _lib()
    R, K = x.shape
    out = _nan(R, n)
    _check(lib.lrpx_linear_small(_ptr(x), K, _ptr(w), _ptr(bias), _ptr(out), n, R, K, n, 0, st))
    return out


def _il4():
    """interleaved gate row r = 16 j + 4 gate + u -> row gate * H + 4 j + u of the un-interleaved matrix (gridTD, AoA)"""
    jj, qq, uu = torch.meshgrid(torch.arange(H // 4), torch.arange(4), torch.arange(4), indexing="ij")
    return (qq * H + 4 * jj + uu).reshape(-1)


def _aoa_decoupled(eng, tr, enc, tok, model_bias, sd_raw, use_tab):
    """the decoupled trace (`AOAEngine._trace_decoupled`) with every GEMM on lrpx_linear_small: inputs, recurrence (from a `zin` formed on the host
    in fp64 from the RAW state dict and rounded, or from the engine's token table and the image part), gather, q / gate linear, attention over
    all rows, decoder_aoa_linear, gated sum.  -> (hn, the three recorded row maxima as int32 bits)"""
    lib, st = _lib()
    B, T = tr["B"], tr["T"]
    R = B * T
    c = C.byref(tr["_c"])
    _check(lib.lrpx_aoa_fwd_inputs(c, _ptr(enc["glob"]), _ptr(eng.sd["embedding.weight"]), _ptr(tok), tok.shape[1], None, st))
    if use_tab:
        bias_il = eng.bcat_model_il if model_bias else eng.bcat_explainer_il
        gimg = _nan(B, 4 * H)
        for b0 in range(0, B, 64):
            nb = min(64, B - b0)
            _check(lib.lrpx_linear_small(_ptr_at(enc["glob"], b0 * H), H, _ptr(eng.W_ig_il), _ptr(bias_il), _ptr_at(gimg, b0 * 4 * H), 4 * H, nb, H,
                                         4 * H, 0, st))
        _check(lib.lrpx_aoa_fwd_recurrence_tab(c, _ptr(eng.W_hh_il), _ptr(eng.tok_table), _ptr(gimg), _ptr(tok), tok.shape[1], st))
    else:
        l, il = "LanguageLSTM.", _il4()
        w_ih = sd_raw[l + "weight_ih"].double()[il]
        b = (sd_raw[l + "bias_ih"] + (sd_raw[l + "bias_hh"] if model_bias else sd_raw[l + "bias_ih"])).double()[il]
        xin = torch.cat([sd_raw["embedding.weight"][tok[:, :T].cpu()], enc["glob"].cpu()[:, None].expand(B, T, H)], 2).double()
        zin = (xin @ w_ih.t() + b).float().reshape(R, 4 * H).cuda()
        _check(lib.lrpx_aoa_fwd_recurrence(c, _ptr(eng.W_hh_il), _ptr(zin), st))
    hn = _nan(R, H)
    am = tr["_amax"].view(torch.int32)
    _check(lib.lrpx_aoa_fwd_gather_h(c, _ptr(hn), _ptr(am[0]), st))
    qg = _rows_linear(hn, eng.Wqg, eng.bqg, 2 * H)
    _check(lib.lrpx_aoa_fwd_attention_all(c, _ptr(qg), 2 * H, _ptr(enc["key"]), _ptr(enc["value"]), _ptr(am[1]), st))
    ln = _rows_linear(tr["ctx"].view(R, H), eng.sd["decoder_aoa_linear.weight"], eng.sd["decoder_aoa_linear.bias"], H)
    _check(lib.lrpx_aoa_fwd_post_all(c, _ptr(qg), 2 * H, _ptr(ln), _ptr(am[2]), st))
    torch.cuda.synchronize()
    return hn, am


def _ada_args(eng, tr, enc, rows):
    from lrp_amd._lib import AdaStepArgs
    sa = AdaStepArgs()
    wg, ws, bs, wh = _att_args(eng)
    keep = dict(zz=_nan(tr["B"], 5 * H), scr=_nan(rows, 3 * eng.P))
    sa.w_cat, sa.b_cat, sa.Vp, sa.att_img = _ptr(eng.Wcat), _ptr(eng.bcat), _ptr(enc["Vp"]), _ptr(enc["att_img"])
    sa.Wg, sa.Ws, sa.bs, sa.wh = _ptr(wg), _ptr(ws), _ptr(bs), _ptr(wh)
    sa.zz, sa.att_scratch = _ptr(keep["zz"]), _ptr(keep["scr"])
    return sa, keep


def _ada_step(eng, tr, enc, t, tok, sa):
    lib, st = _lib()
    c = C.byref(tr["_c"])
    _check(lib.lrpx_adaatt_fwd_pre(c, t, _ptr(enc["glob"]), _ptr(eng.sd["embedding.weight"]), _ptr(tok), tok.shape[1], st))
    _check(lib.lrpx_adaatt_fwd_step(c, t, C.byref(sa), st))


def _ada_decoupled(eng, tr, enc, tok):
    """`AdaAttEngine.trace`, decoupled: inputs, the input half of the five gate rows (interleaved 16-row groups), recurrence, attention over all rows"""
    lib, st = _lib()
    B, T, P = tr["B"], tr["T"], eng.P
    R, W, NR = B * T, H + 2 * E, eng.NR
    c = C.byref(tr["_c"])
    _check(lib.lrpx_adaatt_fwd_inputs(c, _ptr(enc["glob"]), _ptr(eng.sd["embedding.weight"]), _ptr(tok), tok.shape[1], st))
    zin = _nan(R, NR)
    for r0 in range(0, R, 64):
        _check(lib.lrpx_linear_small(_ptr_at(tr["xh"], r0 * W + H), W, _ptr(eng.Wx_il), _ptr(eng.b_il), _ptr_at(zin, r0 * NR), NR, min(64, R - r0), 2 * E,
                                     NR, 0, st))
    _check(lib.lrpx_adaatt_fwd_recurrence(c, _ptr(eng.Wh_il), _ptr(zin), st))
    scr = _nan(R, 3 * P)
    wg, ws, bs, wh = _att_args(eng)
    _check(lib.lrpx_adaatt_fwd_attention_all(c, _ptr(enc["Vp"]), _ptr(enc["att_img"]), _ptr(wg), _ptr(ws), _ptr(bs), _ptr(wh), _ptr(scr), st))
    torch.cuda.synchronize()
    return scr


# ---- b. one step from a drawn state -----------------------------------------------------------------------------------------------------------
def _step_sel(model):
    """the reference is a T = 1 trace: its step 0 is the kernels' step t"""
    return lambda k, v: v[:, 1] if k in STATE[model] else v[:, 0]


@pytest.mark.parametrize("case", F.step_cases(), ids=lambda c: "-".join(str(v) for v in c[:3] + c[5:7]))
def test_one_step_from_a_drawn_state(case):
    model, P, variant, B, _, model_bias, gate_h_new, _ = case
    eng = _engine(model, P, variant)
    ref64, refs32 = F.references(*case)
    enc_c, tok_c, h0 = F.draw(model, P, variant, B, 1)
    T, t = 4, 2
    enc = _dev(enc_c, B)
    tok = torch.randint(1, V - 3, (B, T + 3), generator=torch.Generator().manual_seed(P))
    tok[:, t], tok[:, t + 1] = tok_c[:, 0], tok_c[:, 1]
    tok = tok.cuda()
    tr = _trace(model, eng, B, T, P, h0, slot=t)
    before = {k: v.clone() for k, v in _tensors(model, tr).items()}
    scr = _nan(B, 3 * P)
    if model == "gridtd":
        _gridtd_step(eng, tr, enc, t, tok, model_bias, gate_h_new, scr)
    elif model == "aoa":
        _aoa_step(eng, tr, enc, t, tok, model_bias)
    else:
        sa, keep = _ada_args(eng, tr, enc, B)
        _ada_step(eng, tr, enc, t, tok, sa)
        scr = keep["scr"]
    torch.cuda.synchronize()
    got = _tensors(model, tr)
    # every slot the step does not own is what it was (NaN, or the drawn state): bit for bit
    for k, v in got.items():
        own = t + 1 if k in STATE[model] else t
        for j in range(v.shape[1]):
            if j == own:
                continue
            if model == "adaatt" and k == "xh" and j == t + 1:          # the cell leaves the next step's h columns
                assert _bits(v[:, j, H:], before[k][:, j, H:]) and _bits(v[:, j, :H], got["h"][:, t + 1]), k
                continue
            assert _bits(v[:, j], before[k][:, j]), "%s: slot %d is not the step's and was written" % (k, j)
    own = {k: (v[:, t + 1] if k in STATE[model] else v[:, t]) for k, v in got.items()}
    # the input rows are copies
    emb = eng.sd["embedding.weight"][tok[:, t]]
    if model == "gridtd":
        assert _bits(own["xh1"], torch.cat([h0["h2"].cuda(), enc["glob"], emb, h0["h1"].cuda()], 1))
        assert _bits(own["xh2"], torch.cat([own["ctx_hat"], own["h1"], h0["h2"].cuda()], 1))
    elif model == "aoa":
        assert _bits(own["xh"], torch.cat([emb, enc["glob"], h0["h"].cuda()], 1))
    else:
        assert _bits(own["xh"], torch.cat([h0["h"].cuda(), emb, enc["glob"]], 1))
    keys = STATE[model] + STEPWISE[model]
    what = "%s step P %d %s%s" % (model, P, variant, " gate on the new h1" if gate_h_new else "")
    _grade(model + " step", what, own, ref64, refs32, keys, _step_sel(model))
    if model == "aoa":
        _softmax_sums(what, own["alpha"], None, P)
        # the 64-thread attention kernel (and the other kernels of the decoupled path) on the same step: a T = 1 trace
        tr1 = _trace(model, eng, B, 1, P, h0, slot=0)
        tok1 = tok[:, t:t + 4].contiguous()
        for use_tab in (False, True):
            _aoa_decoupled(eng, tr1, enc, tok1, model_bias, F.state("aoa", 0, ""), use_tab)
            got1 = _tensors(model, tr1)
            own1 = {k: (v[:, 1] if k in STATE[model] else v[:, 0]) for k, v in got1.items()}
            assert _bits(own1["xh"], own["xh"])
            _grade("aoa step, decoupled kernels", what + (" (token table)" if use_tab else " (host zin)"), own1, ref64, refs32, keys, _step_sel(model))
            _softmax_sums(what + " 64-thread kernel", own1["alpha"], None, P)
            tr1 = _trace(model, eng, B, 1, P, h0, slot=0)
    else:
        _softmax_sums(what, own["alpha"], own["beta"], P)
        # the scores the attention kernels left: [z | h_proj | s_proj]; beta is the last entry of the softmax over [z, sentinel score]
        z = scr.view(B, 3, P).cpu().double()
        wh = F.state(model, P, variant)["AdaAttention.w_h.weight"][0].double()
        zs = (wh * torch.tanh(z[:, 2] + z[:, 1])).sum(-1)
        beta = torch.softmax(torch.cat([z[:, 0], zs[:, None]], 1), -1)[:, -1]
        d = float((beta - own["beta"].cpu().double()).abs().max())
        print("%s: beta against the fp64 softmax of the kernel's own scores: %.2e" % (what, d))
        # (the sentinel score is a sum of P terms |w_h[j] tanh| <= |w_h[j]|, each within 2^-24 of itself at every step of the sum and after
        # tanhf: |dz| <= (P + 3) 2^-24 sum |w_h|; d beta = beta (1 - beta) dz <= dz / 4; and the softmax's own rounding as above)
        assert d <= 0.25 * (P + 3) * 2.0 ** -24 * float(wh.abs().sum()) + 4 * P * 2.0 ** -24
        sel = _step_sel(model)
        e = rel_err(z[:, 0], sel("zsc", ref64["zsc"])[:, :P])
        e32 = max(rel_err(sel("zsc", r["zsc"])[:, :P], sel("zsc", ref64["zsc"])[:, :P]) for r in refs32)
        print("%s: pixel scores %.2e from fp64 (fp32: %.2e)" % (what, e, e32))
        assert e <= 6 * max(e32, FLOOR)


# ---- c. whole traces ---------------------------------------------------------------------------------------------------------------------------
def _grid_args(eng, tr, enc, tok, model_bias, interleaved):
    from lrp_amd._lib import GridStepArgs
    B = tr["B"]
    sa = GridStepArgs()
    keep = dict(zz1=_nan(B, 5 * H), zz2=_nan(B, 4 * H), scr=_nan(B, 3 * eng.P))
    wg, ws, bs, wh = _att_args(eng)
    sa.glob, sa.emb, sa.tok, sa.tok_ld = _ptr(enc["glob"]), _ptr(eng.sd["embedding.weight"]), _ptr(tok), tok.shape[1]
    sa.w_cat1, sa.b_cat1, sa.w_cat2 = _ptr(eng.Wcat1), _ptr(eng.bcat1), _ptr(eng.Wcat2)
    sa.b_cat2 = _ptr(eng.bcat2_model if model_bias else eng.bcat2_explainer)
    if interleaved:
        sa.w_il1, sa.b_il1, sa.w_il2 = _ptr(eng.Wcat1_il), _ptr(eng.bcat1_il), _ptr(eng.Wcat2_il)
        sa.b_il2 = _ptr(eng.bcat2_model_il if model_bias else eng.bcat2_explainer_il)
    sa.Vp, sa.att_img = _ptr(enc["Vp"]), _ptr(enc["att_img"])
    sa.Wg, sa.Ws, sa.bs, sa.wh = _ptr(wg), _ptr(ws), _ptr(bs), _ptr(wh)
    sa.zz1, sa.zz2, sa.att_scratch = _ptr(keep["zz1"]), _ptr(keep["zz2"]), _ptr(keep["scr"])
    return sa, keep


def _aoa_args(eng, tr, enc, tok, model_bias, fused):
    from lrp_amd._lib import AoaStepArgs
    B = tr["B"]
    sa = AoaStepArgs()
    keep = dict(zz=_nan(B, 4 * H), qg=_nan(B, 2 * H), lin=_nan(B, H))
    sa.glob, sa.emb, sa.tok, sa.tok_ld = _ptr(enc["glob"]), _ptr(eng.sd["embedding.weight"]), _ptr(tok), tok.shape[1]
    sa.w_cat, sa.b_cat = _ptr(eng.Wcat), _ptr(eng.bcat_model if model_bias else eng.bcat_explainer)
    sa.w_qg, sa.b_qg = _ptr(eng.Wqg), _ptr(eng.bqg)
    if fused:
        sa.w_cat_il, sa.b_cat_il = _ptr(eng.Wcat_il), _ptr(eng.bcat_model_il if model_bias else eng.bcat_explainer_il)
    sa.w_lin, sa.b_lin = _ptr(eng.sd["decoder_aoa_linear.weight"]), _ptr(eng.sd["decoder_aoa_linear.bias"])
    sa.key, sa.value, sa.zz, sa.qg, sa.lin = _ptr(enc["key"]), _ptr(enc["value"]), _ptr(keep["zz"]), _ptr(keep["qg"]), _ptr(keep["lin"])
    return sa, keep


def _paths(model):
    return {"gridtd": ("steps, interleaved rows", "steps, rows left null"), "aoa": ("steps, fused", "steps, not fused", "decoupled, host zin",
            "decoupled, token table"), "adaatt": ("step loop", "decoupled")}[model]


def _run_trace(model, path, eng, B, T, P, enc, tok, h0, model_bias, sd_raw):
    """one whole trace from NaN buffers and the drawn state, through `path` -> the trace"""
    lib, st = _lib()
    tr = _trace(model, eng, B, T, P, h0, slot=0)
    c = C.byref(tr["_c"])
    if model == "gridtd":
        sa, keep = _grid_args(eng, tr, enc, tok, model_bias, path.startswith("steps, interleaved"))
        _check(lib.lrpx_gridtd_fwd_steps(c, 0, T, C.byref(sa), st))
    elif model == "aoa" and path.startswith("steps"):
        sa, keep = _aoa_args(eng, tr, enc, tok, model_bias, path == "steps, fused")
        _check(lib.lrpx_aoa_fwd_steps(c, 0, T, C.byref(sa), st))
    elif model == "aoa":
        hn, am = _aoa_decoupled(eng, tr, enc, tok, model_bias, sd_raw, path.endswith("token table"))
        tr["_hn"], tr["_am"] = hn, am
    elif path == "step loop":
        sa, keep = _ada_args(eng, tr, enc, B)
        for t in range(T):
            _ada_step(eng, tr, enc, t, tok, sa)
    else:
        _ada_decoupled(eng, tr, enc, tok)
    torch.cuda.synchronize()
    return tr


def _whole(case, B=None):
    model, P, variant, Bmax, T, model_bias, gate_h_new, _ = case
    B = Bmax if B is None else B
    eng = _engine(model, P, variant)
    ref64, refs32 = F.references(*case)
    enc_c, tok_c, h0 = F.draw(model, P, variant, Bmax, T)
    enc, tok = _dev(enc_c, B), tok_c[:B].cuda()
    sd_raw = F.state(model, P, variant)
    keys = STATE[model] + STEPWISE[model]
    sel = lambda k, v: v[:B]
    for path in _paths(model):
        tr = _run_trace(model, path, eng, B, T, P, enc, tok, h0, model_bias, sd_raw)
        got = _tensors(model, tr)
        what = "%s %s P %d %s B %d T %d" % (model, path, P, variant, B, T)
        for k in STATE[model]:
            assert _bits(got[k][:, 0], h0[k][:B].cuda()), k
        _copies_exact(model, got, enc, tok, eng.sd["embedding.weight"], T, first_h_row=(path != "decoupled"))
        group = "%s %s%s" % (model, path, " (scores past +-89)" if variant == "over" else "")
        _grade(group, what, got, ref64, refs32, keys, sel)
        if model == "aoa":
            _softmax_sums(what, got["alpha"], None, P)
            if "_am" in tr:
                _row_maxima(what, tr, B, T)
        else:
            _softmax_sums(what, got["alpha"], got["beta"], P)
        if variant == "over":
            assert float(got["alpha"].min()) == 0.0          # exp underflows for the pixels far below the maximum, and never overflows


def _row_maxima(what, tr, B, T):
    """d. hn_amax, ctx_amax, hc_amax, read as float bits, are max |.| of the rows the kernels wrote, bit for bit"""
    R = B * T
    am = tr["_am"]
    for j, (name, rows) in enumerate((("hn_amax", tr["_hn"]), ("ctx_amax", tr["ctx"].view(R, H)), ("hc_amax", tr["hc"].view(R, H)))):
        want = rows.abs().amax(-1)
        assert _bits(am[j].view(torch.float32), want), "%s %s: not max |.| of the row (worst %.3e)" % (
            what, name, float((am[j].view(torch.float32) - want).abs().max()))
    assert bool((tr["ctx"][0] > 0).all()) and (B == 1 or bool((tr["ctx"][1:] < 0).all()))          # (image 1's value rows are negated)
    print("%s: hn_amax, ctx_amax, hc_amax equal max |.| of their rows bit for bit" % what)


TRACES = [c for c in F.trace_cases() if c[3] == 2]


@pytest.mark.parametrize("case", TRACES, ids=lambda c: "-".join(str(v) for v in (c[0], c[2], c[4])))
def test_whole_trace_vs_fp64(case):
    """T = 3 (sentinel above every pixel score), T = 11 (below), and the draw whose scores pass +-89, through every path of each model"""
    _whole(case)


@pytest.mark.parametrize("B", F.B_SWEEP)
@pytest.mark.parametrize("model", F.MODELS)
def test_every_row_tile_vs_fp64(model, B):
    """B = 1, 17, 33, 49 and 64: RT = 1, 2, 3, 4, 4 of the fused and recurrence kernels; B = 65: the 64-image slices and the fall-back to the
    unfused step"""
    _whole((model, 36, "hi", max(F.B_SWEEP), 2, False, False, False), B)


def test_row_maxima_are_recorded():
    """d. on its own: the decoupled AoA path at B = 2, T = 3, one image's value rows negated (a signed maximum would record 0 there)"""
    case = ("aoa", 36, "hi", 2, 3, False, False, False)
    eng = _engine("aoa")
    enc_c, tok_c, h0 = F.draw("aoa", 36, "hi", 2, 3)
    enc, tok = _dev(enc_c, 2), tok_c.cuda()
    for path in ("decoupled, host zin", "decoupled, token table"):
        tr = _run_trace("aoa", path, eng, 2, 3, 36, enc, tok, h0, False, F.state("aoa", 0, ""))
        _row_maxima(path, tr, 2, 3)
        assert bool((tr["_am"][1].view(torch.float32)[3:] > 0).all())
    assert F.references(*case)[0]["ctx"][1].max() < 0


# ---- e. the engines' trace ----------------------------------------------------------------------------------------------------------------------
def _engine_trace(model, model_bias, grad, setup, f16=False):
    P, variant, B, T = 36, "hi", 2, 3
    mb = model_bias or grad
    case = (model, P, variant, B, T, mb, False, True)
    eng = _engine(model, P, variant)
    ref64, refs32 = F.references(*case)
    enc_c, tok_c, _ = F.draw(model, P, variant, B, T, True)
    enc = dict(_dev(enc_c, B), B=B, P=P)
    caps = tok_c[:, :T + 1].contiguous().cuda()
    saved = {k: getattr(eng, k) for k in setup}
    try:
        for k, v in setup.items():
            setattr(eng, k, v)
        tr = eng.trace(enc, caps, model_bias=model_bias, predictions=False, grad=grad) if model != "adaatt" else eng.trace(enc, caps, predictions=False)
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            setattr(eng, k, v)
    keep = ("o1", "o2", "sgate", "o", "sg")
    keys = tuple(k for k in STATE[model] + STEPWISE[model] if k in tr and (grad or k not in keep))
    if grad:
        assert all(k in tr for k in (("o1", "o2", "sgate") if model == "gridtd" else ("o", "sg")))
    fcw, fcb = F.state(model, P, variant)["fc.weight"], F.state(model, P, variant)["fc.bias"]
    for r, (dt, o) in zip([ref64] + refs32, [(torch.float64, "torch")] + [(torch.float32, o) for o in F.ORDERS]):
        if "logit" not in r:
            r["logit"] = F.target_logit(r["hc"], fcw, fcb, tok_c, dt, o)
    keys = keys + ("logit",)
    what = "%s engine trace %s model_bias %s grad %s" % (model, setup, model_bias, grad)
    if not f16:
        _grade("%s engine trace" % model, what, tr, ref64, refs32, keys)
    else:          # the fp16-split GEMMs: 1e-4 of the maximum (tests/test_gpu_t20.py); their ratio to the fp32 yardstick is printed
        worst = 0.0
        for k in keys:
            g = tr[k].cpu()
            assert torch.isfinite(g).all(), k
            e = rel_err(g, ref64[k])
            e32 = max(rel_err(r[k], ref64[k]) for r in refs32)
            print("%s %s (f16): %.2e of the maximum (bound 1e-4); %.1f x the fp32 yardstick" % (what, k, e, e / max(e32, FLOOR)))
            worst = max(worst, e / max(e32, FLOOR))
            assert e <= 1e-4, (what, k, e)
        _note("aoa engine trace, f16 split GEMMs (ratio to the fp32 yardstick, bound 1e-4 of the maximum)", worst)
    _copies_exact(model, tr, enc, caps, eng.sd["embedding.weight"], T)
    _softmax_sums(what, tr["alpha"], tr.get("beta"), P)


@pytest.mark.parametrize("model_bias, grad", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("fused", [True, False])
def test_gridtd_engine_trace(fused, model_bias, grad):
    _engine_trace("gridtd", model_bias, grad, dict(fused_steps=fused))


@pytest.mark.parametrize("model_bias, grad", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("mode", ["decoupled", "fused", "unfused"])
def test_aoa_engine_trace(mode, model_bias, grad):
    _engine_trace("aoa", model_bias, grad, dict(decoupled=(mode == "decoupled"), fused_steps=(mode != "unfused"), force_f16=False))


@pytest.mark.parametrize("model_bias, grad", [(False, False), (True, True)])
def test_aoa_engine_trace_f16_split_gemms(model_bias, grad):
    _engine_trace("aoa", model_bias, grad, dict(decoupled=True, force_f16=True), f16=True)


@pytest.mark.parametrize("decoupled", [True, False])
def test_adaatt_engine_trace(decoupled):
    _engine_trace("adaatt", False, False, dict(decoupled=decoupled))


# ---- f. the LRP-inference re-weighting ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Vn", [203, 10004])
@pytest.mark.parametrize("rows", [3, 5])
def test_lrp_reweight_vs_fp64(rows, Vn):
    """rows: a skipped arg-max word (hcw = ctx + h bit for bit), a zero logit (all relevance zero: both `== 0` guards), h = 0 with the arg-max in
    the last column (`mh == 0`), ctx = 0 (`mc == 0`), a plain row; raw scores and log-softmax; the flat entry and gridTD's trace entry"""
    eng = _engine("gridtd")
    lib, st = _lib()
    gen = torch.Generator().manual_seed(rows + Vn)
    ld = Vn + 7
    pred = torch.full((rows, ld), 1e30)
    pred[:, :Vn] = torch.randn(rows, Vn, generator=gen)
    h, ctx = 0.5 * torch.randn(rows, H, generator=gen), torch.relu(torch.randn(rows, H, generator=gen))
    fcw = torch.randn(Vn, H, generator=gen) / math.sqrt(H)
    skip = torch.zeros(Vn, dtype=torch.bool)
    pred[0, 17] = 9.0
    skip[17] = True                                        # row 0: skipped
    pred[1, :Vn] = -pred[1, :Vn].abs() - 0.1
    pred[1, 5] = 0.0                                       # row 1: the arg-max logit is exactly 0
    pred[2, Vn - 1] = 8.0
    h[2] = 0.0                                             # row 2: last column, h = 0
    if rows > 3:
        pred[3, 0] = 7.5
        ctx[3] = 0.0                                       # row 3: first column, ctx = 0
    skip[1:4] = True                                       # (skipped words that are no arg-max)
    skip[5] = False
    pd, hd, cd, fd, sk = pred.cuda(), h.cuda(), ctx.cuda(), fcw.cuda(), skip.to(torch.uint8).cuda()
    T, t = 2, 1
    tr = _trace("gridtd", eng, rows, T, 36)
    tr["h2"][:, t + 1], tr["ctx_hat"][:, t] = hd, cd
    for lsm in (0, 1):
        ref64 = F.lrp_reweight(pred[:, :Vn], h, ctx, fcw, skip, lsm, torch.float64)
        refs32 = [F.lrp_reweight(pred[:, :Vn], h, ctx, fcw, skip, lsm, torch.float32, o) for o in F.ORDERS]
        assert ref64[1].tolist()[:3] == [17, 5, Vn - 1]
        runs = [("rows", lambda buf: lib.lrpx_lrp_reweight_rows(_ptr(pd), ld, Vn, _ptr(hd), H, _ptr(cd), H, _ptr(fd), _ptr(sk), _ptr(buf), rows, H,
                                                                lsm, st))]
        if lsm == 0:
            runs.append(("gridtd trace", lambda buf: lib.lrpx_gridtd_lrp_reweight(C.byref(tr["_c"]), t, _ptr(pd), ld, Vn, _ptr(fd), _ptr(sk),
                                                                                  _ptr(buf), st)))
        for name, run in runs:
            buf = _guarded(rows * H)
            _check(run(buf))
            torch.cuda.synchronize()
            hcw = _guard_ok(buf, rows * H, "lrp_reweight").view(rows, H)
            what = "lrp_reweight (%s) rows %d V %d log_softmax %d" % (name, rows, Vn, lsm)
            assert _bits(hcw[0], cd[0] + hd[0]), what + ": the skipped row is not ctx + h"
            if lsm == 0:
                assert _bits(hcw[1], cd[1] + hd[1]), what + ": a zero logit leaves weights of 1"
            _grade("lrp_reweight", what, dict(hcw=hcw), dict(hcw=ref64[0]), [dict(hcw=r[0]) for r in refs32], ("hcw",))
