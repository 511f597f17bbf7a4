"""The four decoder back-passes of csrc/decoder_gridtd.hip and csrc/decoder_aoa.hip ALONE, through the C ABI, on traces of drawn values (tests/decoder_restate.py:
planted exact zeros of both signs and +-0.004 under every stabiliser, a zero logit, an all-zero row), against the fp64 restatement of the
same file: gridTD relevance (`gridtd_rel_*`), AoA relevance (`aoa_rel_*`, the fused lock-steps of csrc/dense_small.hip and
csrc/dense_f16x3.hip, `rel_words_norm_parts`), gridTD gradient / guided (`gridtd_grad_*`, `lstm_cell_bwd`, `spread_pixels`) and AoA
gradient (`aoa_grad_*`, `keep_cols`).  Every state buffer starts as NaN, so a stale read by an inactive row shows; every intermediate
tensor of the C state structs is compared, not only what a projector GEMM has mixed.  B = 2 with T in {3, 26}, one B = 3, T = 11 AoA
case (33 rows: one over the fused step's 32-row tile), P = 36 (two pixel chunks, 28 + 8), `lens` in {None, [T, 2], [2, 0]}.

Bounds.  Default (exact) decoder arithmetic: `fp64_anchor.fp32_grade` with the project's C = 6 and FLOOR = 1e-7, against the WORST of
three plain fp32 evaluations in different summation orders (tests/test_decoder_restate_host.py holds every draw to the condition that
makes this a fair yardstick).  `f16` variants (the lock-step GEMMs on the fp16 split products, a 22-bit operand path: T = 3 only): what
tests/test_gpu_t20.py holds that arithmetic to - 1e-4 of the maximum, normalised r_words 2e-5.

Conditioning.  The gridTD relevance chain on unfloored randn is fine at T = 3; at T = 26 it grows to 1e19 and plain fp32 is 1e-4 off
fp64, so the T = 26 gridTD relevance draw floors |c1|, |c2|, |g1|, |g2| at 0.2 outside the planted entries (plain fp32 then stays within
2e-5 of fp64).  The AoA chain assigns r_h and needs no floor; the gradient decoders divide by nothing.

`lrpx_aoa_grad_pix` takes no `lens` (it is a function of v1, v2 and alpha alone), so rows behind an image's last word are zero only in
the compact call the engine makes; the test holds the row-list call to the live rows of the full one.

Worst e / max(e32, FLOOR) per family over all cases and outputs, first MI355X run (the bound is 6):
  gridTD relevance  2.32 (T 3, r_words)       f16 lock-steps: 0.05 of the 1e-4 / 2e-5 bounds
  AoA relevance     1.71 two-launch steps, 0.75 r_words of the fused steps        f16 lock-steps: 0.05 of their bounds, fused and not
  gridTD gradient   1.19
  AoA gradient      1.66
No kernel missed a check: no defect found.  The six mutations of the issue, each built into a library of its own and not committed:
the zero branch of z~ dropped in the fused steps' copy (`aoa_rel_coef_kernel`'s dg) - both AoA relevance tests, every case; `s == 0 ?
r_ch0 : 0` dropped - both gridTD relevance tests (every case with a word behind the first that is not the zero-logit row); `+=` -> `=`
on r_glob - the gridTD and AoA relevance tests; `dc = dc * f` dropped - the gridTD gradient test, every case; the head offset dropped
in `head_only` - the AoA relevance tests at heads 4 and 7.  The `s + 1 >= T` exit of `aoa_rel_ca_kernel` cannot turn a test red: the
kernel has one caller, `lrpx_aoa_rel_steps`, which launches it for s + 1 < n_steps <= T only - the line is unreachable.
Every deviation is printed before it is asserted."""
import ctypes as C

import pytest
import torch

import lrp_amd  # noqa: F401
import decoder_restate as R
from conftest import rel_err
from fp64_anchor import fp32_grade

pytestmark = pytest.mark.gpu

H = E = R.H
P, NH = R.P_DRAW, R.NH_DRAW
GUARD = 4096
T3 = [c for c in R.T_CASES if c[0] == 3]
IDS = lambda v: str(v).replace(" ", "")


@pytest.fixture(scope="module")
def grid():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd.explainers.gridtd import GridTDBUEngine
    return GridTDBUEngine(R.np_state("gridtd"))


@pytest.fixture(scope="module")
def aoa():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from lrp_amd.explainers.aoa import AOAEngine
    eng = AOAEngine(R.np_state("aoa"))
    assert eng.cnn is None and eng.NH == NH
    return eng


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------
def _nan(*s):
    return torch.full(s, float("nan"), device="cuda")


def _guarded(n):
    """a flat buffer of n floats + a guard region behind it (as tests/test_gpu_dense.py)"""
    return torch.full((n + GUARD,), 777.0, device="cuda")


def _guard_ok(buf, n, what):
    assert bool((buf[n:] == 777.0).all()), what + ": written behind the compact output"
    return buf[:n]


def _bits(a, b):
    """bit for bit, NaN left by nobody included"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same(x, y, what, keys=None):
    for k in (keys or x):
        assert _bits(x[k], y[k]), "%s: %s differs in %d of %d elements" % (what, k, int((x[k] != y[k]).sum()), x[k].numel())


def _lens_t(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda") if lens is not None else None


def _rows(lens, B, T):
    active = [b * T + t for b in range(B) for t in range(T) if lens is None or t < lens[b]]
    return active, torch.tensor(active, dtype=torch.int32, device="cuda")


def _state(cls, rs, lens_t):
    from lrp_amd._lib import ptr
    c = cls()
    c.lens = ptr(lens_t)
    for k, v in rs.items():
        setattr(c, k, ptr(v))
    return c


def _grade(family, T, lens, got, keys, live, f16=False):
    """every output of `keys` on the live rows against fp64: fp32 grade against the worst fp32 order, or the f16 variant's flat bounds"""
    ref64, refs32, _ = R.references(family, T, lens)
    worst = 0.0
    for k in keys:
        g = got[k].cpu()
        assert not torch.isnan(g[live]).any() and not torch.isinf(g[live]).any(), (k, "NaN / inf in a live row")
        what = "%s T %d lens %s %s%s" % (family, T, lens, k, " (f16)" if f16 else "")
        if f16:
            e = rel_err(g[live], ref64[k][live])
            if k == "r_words_norm":
                e = float((g[live].double() - ref64[k][live]).abs().max())
            bound = 2e-5 if k == "r_words_norm" else 1e-4
            print("%s: %.2e (bound %.0e)" % (what, e, bound))
            worst = max(worst, e / bound)
            assert e <= bound, (what, e)
        else:
            ref32, _ = R.worst_of(refs32, ref64, k, live)
            e, e32, _, _ = fp32_grade(g[live], ref64[k][live], ref32[live], ref32[live], what, margin_min=0)
            worst = max(worst, e / max(e32, 1e-7))
    print("WORST %s%s T %d lens %s: %.2f" % (family, " f16" if f16 else "", T, lens, worst))


def _upto(x, T):
    """(rows, T, ..) with everything behind word t of row (b, t) set to zero (what nobody writes stays NaN there)"""
    rows = x.shape[0]
    keep = (torch.arange(T)[None, :] <= (torch.arange(rows) % T)[:, None]).to(x.device)
    return torch.where(keep.view(rows, T, *([1] * (x.dim() - 2))), x, torch.zeros((), device=x.device))


# ---- 1. gridTD relevance ---------------------------------------------------------------------------------------------------------------------
def _gridtd_rel(eng, T, lens, f16):
    from lrp_amd import _lib, ops
    from lrp_amd._lib import GridRelState, EPI_REL, check, ptr, stream_ptr
    lib, st = _lib.load(), stream_ptr()
    d, sd, B = R.case("gridtd_rel", T, lens)
    rows, W1 = B * T, 2 * E + 2 * H
    tr = eng._alloc_trace(B, T)
    for k in ("xh1", "xh2", "h2", "c1", "c2", "g1", "i1", "f1", "g2", "i2", "f2", "s", "ctx", "ctx_hat", "hc", "alpha", "beta"):
        tr[k].copy_(d[k])
    dv = {k: d[k].cuda() for k in ("logit", "tok", "Vp", "proj_pre", "glob_pre", "avg")}
    lens_t = _lens_t(lens)
    idx, row2img, _ = eng._row_index(B, T)
    active, rl = _rows(lens, B, T)
    wg2, wg1, wgp = (eng.p_wg2_h, eng.p_wg1_h, eng.p_gp_rel_h) if f16 else (eng.p_wg2, eng.p_wg1, eng.p_gp_rel)
    fcw = eng.sd["fc.weight"]

    def run(mode):
        rs = dict(r_h2n=_nan(rows, H), r_c2=_nan(rows, H), r_c1=_nan(rows, H), r_ch0=_nan(rows, H), r_h2p=_nan(rows, H), r_glob=_nan(rows, E),
                  A=_nan(rows, H), rx=_nan(rows, W1), wacc=_nan(rows, T, H), r_words=_nan(rows, T))
        c = _state(GridRelState, rs, lens_t)
        ctr, crs = C.byref(tr["_c"]), C.byref(c)
        check(lib.lrpx_gridtd_rel_init(ctr, crs, ptr(fcw), ptr(dv["logit"]), ptr(dv["tok"]), T + 1, st))
        kw2 = dict(pix_per_map=1, oc_split=3 * H, x=tr["xh2"], out0=rs["rx"], f16x3=f16)
        kw1 = dict(pix_per_map=1, oc_split=W1, x=tr["xh1"], out0=rs["rx"], f16x3=f16)
        if mode == "steps":
            d2 = ops.conv_desc(rs["A"], wg2, rows, 0, H, 3 * H, 1, EPI_REL, map2img=idx[0], **kw2)
            d1 = ops.conv_desc(rs["A"], wg1, rows, 0, H, W1, 1, EPI_REL, map2img=idx[0], **kw1)
            check(lib.lrpx_gridtd_rel_steps(ctr, crs, T, C.byref(d2), C.byref(d1), ptr(idx), idx.shape[1], st))
        else:
            for s in range(T):
                if s == 0 or mode == "phases":
                    check(lib.lrpx_gridtd_rel_step(ctr, crs, s, 0, st))
                ops.conv_mfma(rs["A"], wg2, rows, 0, H, 3 * H, 1, EPI_REL, map2img=idx[s], **kw2)
                check(lib.lrpx_gridtd_rel_step(ctr, crs, s, 1, st))
                ops.conv_mfma(rs["A"], wg1, rows, 0, H, W1, 1, EPI_REL, map2img=idx[s], **kw1)
                check(lib.lrpx_gridtd_rel_step(ctr, crs, s, 3 if (mode == "phase3" and s + 1 < T) else 2, st))
        rs["a_glob"] = _nan(rows, E)
        check(lib.lrpx_gridtd_rel_glob(ctr, crs, ptr(dv["glob_pre"]), ptr(rs["a_glob"]), st))
        rs["r_avg"] = _nan(rows, H)                  # (the bottom-up model: the global feature is a Linear(H, E) of the mean of Vp)
        ops.conv_mfma(rs["a_glob"], wgp, rows, 0, E, H, 1, EPI_REL, pix_per_map=1, oc_split=H, x=dv["avg"], map2img=row2img, out0=rs["r_avg"], f16x3=f16)
        rs["U"] = _nan(rows, H)
        check(lib.lrpx_rel_avg_u(ptr(rs["r_avg"]), ptr(dv["avg"]), ptr(rs["U"]), rows, T, H, P, st))
        rs["r_words_norm"] = rs["r_words"].clone()
        check(lib.lrpx_rel_words_norm(ptr(rs["r_words_norm"]), rows, T, st))
        rs["a_proj"] = _nan(rows, P, H)
        check(lib.lrpx_gridtd_rel_pix_rows(ctr, crs, ptr(dv["Vp"]), ptr(dv["proj_pre"]), ptr(rs["a_proj"]), None, rows, st))
        if mode == "steps":
            full = _nan(rows, P, H)
            check(lib.lrpx_gridtd_rel_pix(ctr, crs, ptr(dv["Vp"]), ptr(dv["proj_pre"]), ptr(full), st))
            buf = _guarded(len(active) * P * H)
            check(lib.lrpx_gridtd_rel_pix_rows(ctr, crs, ptr(dv["Vp"]), ptr(dv["proj_pre"]), ptr(buf), ptr(rl), len(active), st))
            torch.cuda.synchronize()
            assert _bits(full, rs["a_proj"])
            assert _bits(_guard_ok(buf, len(active) * P * H, "gridtd_rel_pix_rows").view(-1, P, H), rs["a_proj"][rl.long()])
        torch.cuda.synchronize()
        return rs

    got = run("steps")
    _same(got, run("phases"), "lrpx_gridtd_rel_steps against the per-phase calls")
    _same(got, run("phase3"), "rel_step phase 3 against phase 2 of s + phase 0 of s + 1")
    live = torch.zeros(rows, dtype=torch.bool)
    live[active] = True
    # exactness: no NaN in what a kernel writes; inactive rows and everything behind word t exact zeros
    for k in ("r_h2n", "r_c2", "r_c1", "r_ch0", "r_glob", "A", "rx", "r_words", "r_words_norm", "a_glob", "r_avg", "U", "a_proj"):
        assert not torch.isnan(got[k]).any(), k
    for k in ("A", "rx", "r_glob", "r_c2", "r_c1", "r_words", "r_words_norm", "a_glob", "r_avg", "U", "a_proj"):
        assert torch.count_nonzero(got[k][~live.cuda()]) == 0, k
    assert not torch.isnan(got["r_h2p"][live.cuda()]).any()
    wacc = _upto(got["wacc"], T)
    assert not torch.isnan(wacc[live.cuda()]).any()
    assert torch.count_nonzero(_upto(got["r_words"], T) - got["r_words"]) == 0          # zero behind word t
    if live[2]:          # the all-zero row (its target's fc row is zero) stays zero through the normalisation
        assert torch.count_nonzero(got["r_words"][2]) == 0 and torch.count_nonzero(got["r_words_norm"][2]) == 0
    got = dict(got, wacc=wacc)
    # U: the mean path's GEMM evaluated in each arithmetic from that arithmetic's a_glob
    ref64, refs32, _ = R.references("gridtd_rel", T, lens)
    wgp_cpu = sd["global_img_feature_proj.weight"]
    for r, order in [(ref64, "torch")] + list(zip(refs32, R.ORDERS)):
        if "U" not in r:
            dt = r["a_glob"].dtype
            r["r_avg"] = d["avg"].to(dt).repeat_interleave(T, 0) * R.mm(r["a_glob"], wgp_cpu.to(dt), order)          # :1116-1119
            r["U"] = R.gridtd_u(r["r_avg"], d["avg"], T, P)
    _grade("gridtd_rel", T, lens, got, ("r_ch0", "r_h2n", "r_h2p", "r_c2", "r_c1", "r_glob", "A", "rx", "wacc", "r_words", "r_words_norm", "a_glob",
                                        "r_avg", "U", "a_proj"), live, f16=bool(f16))


@pytest.mark.parametrize("T, lens", R.T_CASES, ids=IDS)
def test_gridtd_relevance_alone_vs_fp64(grid, T, lens):
    _gridtd_rel(grid, T, lens, 0)


@pytest.mark.parametrize("T, lens", T3, ids=IDS)
def test_gridtd_relevance_alone_f16_lockstep(grid, T, lens):
    assert grid.lockstep_f16 and grid.p_wg1_h is not None
    _gridtd_rel(grid, T, lens, 1)


# ---- 2. AoA relevance ------------------------------------------------------------------------------------------------------------------------
def _aoa_rel(eng, T, lens, f16):
    from lrp_amd import _lib, ops
    from lrp_amd._lib import AoaRelState, EPI_REL, check, ptr, stream_ptr
    lib, st = _lib.load(), stream_ptr()
    d, sd, B = R.case("aoa_rel", T, lens)
    head = R.head_of(T, lens)
    rows, W, dk = B * T, E + 2 * H, H // NH
    tr = eng._alloc_trace(B, T, P)
    for k in ("xh", "h", "c", "g", "i", "f", "ctx", "lin", "c_aoa", "hc", "alpha"):
        tr[k].copy_(d[k])
    dv = {k: d[k].cuda() for k in ("logit", "tok", "value", "glob")}
    lens_t = _lens_t(lens)
    idx, row2img, rowid = eng._row_index(B, T)
    active, rl = _rows(lens, B, T)
    wg, wlin = (eng.p_wg_h, eng.p_lin_rel_h) if f16 else (eng.p_wg, eng.p_lin_rel)
    fcw = eng.sd["fc.weight"]

    def run(mode):
        rs = dict(r_hn=_nan(rows, H), r_glob=_nan(rows, H), A=_nan(rows, H), rx=_nan(rows, W), r_words=_nan(rows, T))
        c = _state(AoaRelState, rs, lens_t)
        ctr, crs = C.byref(tr["_c"]), C.byref(c)
        check(lib.lrpx_aoa_rel_init(ctr, crs, ptr(fcw), ptr(dv["logit"]), ptr(dv["tok"]), T + 1, st))
        rs["A0"] = rs["A"].clone()
        rs["r_ctx"] = _nan(rows, H)
        ops.conv_mfma(rs["A"], wlin, rows, 0, H, H, 1, EPI_REL, pix_per_map=1, oc_split=H, x=tr["ctx"], map2img=rowid, out0=rs["r_ctx"], f16x3=f16)
        kw = dict(pix_per_map=1, oc_split=W, x=tr["xh"], out0=rs["rx"], f16x3=f16)
        if mode == "fused":
            dense = ops.conv_desc(rs["A"], wg, rows, 0, H, W, 1, EPI_REL, map2img=idx[0], **kw)
            assert dense.f16x3 == f16 and not dense.bf16x6
            a_alt, wpart, coef = _nan(rows, H), _nan(rows, T, 4), _nan(2 * rows * H + rows)
            check(lib.lrpx_aoa_rel_steps_fused(ctr, crs, C.byref(dense), ptr(idx), idx.shape[1], ptr(a_alt), ptr(wpart), ptr(coef), st))
            torch.cuda.synchronize()
            assert torch.isnan(rs["rx"]).all() and not torch.isnan(wpart[rl.long(), 0]).any()          # the fused steps really ran: r_xh is never stored
            rs["A"] = a_alt if (T - 1) & 1 else rs["A"]                                    # where lock-step T - 1 read its A from
            rs["r_words_norm"] = rs["r_words"]
        else:
            if mode == "steps":
                dense = ops.conv_desc(rs["A"], wg, rows, 0, H, W, 1, EPI_REL, map2img=idx[0], **kw)
                check(lib.lrpx_aoa_rel_steps(ctr, crs, T, C.byref(dense), ptr(idx), idx.shape[1], st))
            else:
                for s in range(T):
                    check(lib.lrpx_aoa_rel_step(ctr, crs, s, 0, st))
                    ops.conv_mfma(rs["A"], wg, rows, 0, H, W, 1, EPI_REL, map2img=idx[s], **kw)
                    check(lib.lrpx_aoa_rel_step(ctr, crs, s, 1, st))
            rs["r_words_norm"] = rs["r_words"].clone()
            check(lib.lrpx_rel_words_norm(ptr(rs["r_words_norm"]), rows, T, st))
        rs["U"] = _nan(rows, H)
        check(lib.lrpx_rel_avg_u(ptr(rs["r_glob"]), ptr(dv["glob"]), ptr(rs["U"]), rows, T, H, P, st))
        rs["a_val"] = _nan(rows, P, H)
        check(lib.lrpx_aoa_rel_value(ctr, crs, ptr(rs["r_ctx"]), ptr(dv["value"]), head, ptr(rs["a_val"]), st))
        if mode == "steps":
            n = len(active)
            b_rows, b_head, b_head_rows = _guarded(n * P * H), _guarded(rows * P * dk), _guarded(n * P * dk)
            check(lib.lrpx_aoa_rel_value_rows(ctr, crs, ptr(rs["r_ctx"]), ptr(dv["value"]), head, ptr(b_rows), ptr(rl), n, st))
            check(lib.lrpx_aoa_rel_value_head(ctr, crs, ptr(rs["r_ctx"]), ptr(dv["value"]), head, ptr(b_head), None, rows, st))
            check(lib.lrpx_aoa_rel_value_head(ctr, crs, ptr(rs["r_ctx"]), ptr(dv["value"]), head, ptr(b_head_rows), ptr(rl), n, st))
            torch.cuda.synchronize()
            sl = slice(head * dk, (head + 1) * dk)
            a_val = rs["a_val"]
            assert _bits(_guard_ok(b_rows, n * P * H, "aoa_rel_value_rows").view(n, P, H), a_val[rl.long()])
            assert _bits(_guard_ok(b_head, rows * P * dk, "aoa_rel_value_head").view(rows, P, dk), a_val[:, :, sl])
            assert _bits(_guard_ok(b_head_rows, n * P * dk, "aoa_rel_value_head, row list").view(n, P, dk), a_val[rl.long()][:, :, sl])
            other = torch.ones(H, dtype=torch.bool, device="cuda")
            other[sl] = False
            assert torch.count_nonzero(a_val[:, :, other]) == 0          # the other 448 columns
        torch.cuda.synchronize()
        return rs

    got = run("steps")
    _same(got, run("phases"), "lrpx_aoa_rel_steps against the per-phase calls")
    live = torch.zeros(rows, dtype=torch.bool)
    live[active] = True
    lv = live.cuda()
    for k in ("r_hn", "r_glob", "A", "rx", "r_words", "r_words_norm", "A0", "r_ctx", "U", "a_val"):
        assert not torch.isnan(got[k]).any(), k
    for k in ("A", "rx", "r_glob", "r_words", "r_words_norm", "U", "a_val"):
        assert torch.count_nonzero(got[k][~lv]) == 0, k
    assert torch.count_nonzero(_upto(got["r_words"], T) - got["r_words"]) == 0
    if live[2]:
        assert torch.count_nonzero(got["r_words"][2]) == 0 and torch.count_nonzero(got["r_words_norm"][2]) == 0
    keys = ("A0", "r_ctx", "r_hn", "r_glob", "A", "rx", "r_words", "r_words_norm", "U", "a_val")
    _grade("aoa_rel", T, lens, got, keys, live, f16=bool(f16))
    # the fused lock-steps (one launch per step, the point-wise code in the GEMM's epilogue) against the two-launch steps
    assert eng.fused_rel and eng.fused_rel_exact and E == H == 512
    fz = run("fused")
    for k in ("r_glob", "A", "U", "a_val", "A0", "r_ctx"):
        assert not torch.isnan(fz[k][lv]).any() and torch.equal(fz[k][lv], got[k][lv]), "fused lock-steps: %s differs from the two-launch steps" % k
    for k in ("r_glob", "r_words_norm"):
        assert not torch.isnan(fz[k]).any() and torch.count_nonzero(fz[k][~lv]) == 0, k
    assert torch.count_nonzero(_upto(fz["r_words_norm"], T) - fz["r_words_norm"]) == 0
    if live[2]:
        assert torch.count_nonzero(fz["r_words_norm"][2]) == 0          # rel_words_norm_parts on an all-zero row
    dw = float((fz["r_words_norm"] - got["r_words_norm"]).abs().max())
    print("fused against two-launch r_words (normalised): %.2e" % dw)
    _grade("aoa_rel", T, lens, fz, ("r_words_norm",), live, f16=bool(f16))


@pytest.mark.parametrize("T, lens", R.T_CASES + [R.AOA_B3], ids=IDS)
def test_aoa_relevance_alone_vs_fp64(aoa, T, lens):
    _aoa_rel(aoa, T, lens, 0)


@pytest.mark.parametrize("T, lens", T3, ids=IDS)
def test_aoa_relevance_alone_f16_lockstep(aoa, T, lens):
    assert aoa.lockstep_f16 and aoa.p_wg_h is not None
    _aoa_rel(aoa, T, lens, 1)


# ---- 3. gridTD gradient / guided -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, lens", R.T_CASES, ids=IDS)
def test_gridtd_gradient_alone_vs_fp64(grid, T, lens):
    from lrp_amd import _lib, ops
    from lrp_amd._lib import GridGradState, EPI_PLAIN, check, ptr, stream_ptr
    eng, lib, st = grid, _lib.load(), stream_ptr()
    d, sd, B = R.case("gridtd_grad", T, lens)
    rows = B * T
    tr = eng._alloc_trace(B, T, grad=True)
    for k in ("c1", "c2", "g1", "i1", "f1", "o1", "g2", "i2", "f2", "o2", "sgate", "beta", "alpha"):
        tr[k].copy_(d[k])
    tok, lens_t = d["tok"].cuda(), _lens_t(lens)
    active, rl = _rows(lens, B, T)
    gs = dict(d_h2n=_nan(rows, H), d_c2=_nan(rows, H), d_c1=_nan(rows, H), d_ch0=_nan(rows, H), d_h2p=_nan(rows, H), d_glob=_nan(rows, E),
              gates=_nan(rows, 4 * H), dx=_nan(rows, 3 * H), wacc=_nan(rows, T, H), r_words=_nan(rows, T))
    c = _state(GridGradState, gs, lens_t)
    ctr, cgs = C.byref(tr["_c"]), C.byref(c)
    check(lib.lrpx_gridtd_grad_init(ctr, cgs, ptr(eng.sd["fc.weight"]), ptr(tok), T + 1, st))
    for s in range(T):
        check(lib.lrpx_gridtd_grad_step(ctr, cgs, s, 0, st))
        ops.conv_mfma(gs["gates"], eng.p_g2, rows, 0, 4 * H, 3 * H, 1, EPI_PLAIN, pix_per_map=1, oc_split=3 * H, out0=gs["dx"])
        check(lib.lrpx_gridtd_grad_step(ctr, cgs, s, 1, st))
        ops.conv_mfma(gs["gates"], eng.p_g1, rows, 0, 4 * H, 2 * E + H, 1, EPI_PLAIN, pix_per_map=1, oc_split=2 * E + H, out0=gs["dx"])
        check(lib.lrpx_gridtd_grad_step(ctr, cgs, s, 2, st))
    gs["r_words_norm"] = gs["r_words"].clone()
    check(lib.lrpx_rel_words_norm(ptr(gs["r_words_norm"]), rows, T, st))
    gs["a_proj"] = _nan(rows, P, H)
    check(lib.lrpx_spread_pixels(ptr(gs["wacc"]), ptr(tr["alpha"]), ptr(lens_t), ptr(gs["a_proj"]), B, T, H, P, st))
    n = len(active)
    buf = _guarded(n * P * H)
    check(lib.lrpx_spread_pixels_rows(ptr(gs["wacc"]), ptr(tr["alpha"]), ptr(lens_t), ptr(buf), B, T, H, P, ptr(rl), n, st))
    torch.cuda.synchronize()
    assert _bits(_guard_ok(buf, n * P * H, "spread_pixels_rows").view(n, P, H), gs["a_proj"][rl.long()])
    live = torch.zeros(rows, dtype=torch.bool)
    live[active] = True
    lv = live.cuda()
    for k in ("d_h2n", "d_c2", "d_c1", "d_ch0", "d_glob", "gates", "dx", "r_words", "r_words_norm", "a_proj"):
        assert not torch.isnan(gs[k]).any(), k
    for k in ("gates", "dx", "d_glob", "d_c2", "d_c1", "r_words", "r_words_norm", "a_proj"):
        assert torch.count_nonzero(gs[k][~lv]) == 0, k
    assert not torch.isnan(gs["d_h2p"][lv]).any()
    assert torch.count_nonzero(_upto(gs["r_words"], T) - gs["r_words"]) == 0
    got = dict(gs, wacc=_upto(gs["wacc"], T))
    _grade("gridtd_grad", T, lens, got, ("d_ch0", "d_h2n", "d_h2p", "d_c2", "d_c1", "d_glob", "gates", "dx", "wacc", "r_words", "r_words_norm", "a_proj"),
           live)


# ---- 4. AoA gradient -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, lens", R.T_CASES + [R.AOA_B3], ids=IDS)
def test_aoa_gradient_alone_vs_fp64(aoa, T, lens):
    from lrp_amd import _lib, ops
    from lrp_amd._lib import AoaGradState, EPI_PLAIN, check, ptr, stream_ptr
    eng, lib, st = aoa, _lib.load(), stream_ptr()
    d, sd, B = R.case("aoa_grad", T, lens)
    head = R.head_of(T, lens)
    rows, W, dk, Cc = B * T, E + 2 * H, H // NH, eng.C
    tr = eng._alloc_trace(B, T, P, grad=True)
    for k in ("c", "g", "i", "f", "o", "sg", "lin", "alpha"):
        tr[k].copy_(d[k])
    tok, lens_t = d["tok"].cuda(), _lens_t(lens)
    active, rl = _rows(lens, B, T)
    gs = dict(d_h=_nan(rows, H), d_c=_nan(rows, H), dA=_nan(rows, H), dB=_nan(rows, H), gates=_nan(rows, 4 * H), dx=_nan(rows, W),
              d_glob=_nan(rows, H), r_words=_nan(rows, T))
    c = _state(AoaGradState, gs, lens_t)
    ctr, cgs = C.byref(tr["_c"]), C.byref(c)
    check(lib.lrpx_aoa_grad_init(ctr, cgs, ptr(eng.sd["fc.weight"]), ptr(tok), T + 1, st))

    def dense(a, wp, n):          # as `AOAEngine.gradient`
        out = _nan(rows, n)
        ops.conv_mfma(a, wp, rows, 0, a.shape[1], -(-n // 32) * 32, 1, EPI_PLAIN, pix_per_map=1, oc_split=n, out0=out)
        return out
    d_ctx = dense(gs["dA"], eng.p_lin_rel, H)
    check(lib.lrpx_accumulate(ptr(gs["d_h"]), ptr(dense(gs["dB"], eng.p_gate_grad, H)), rows * H, st))
    check(lib.lrpx_keep_cols(ptr(d_ctx), rows, H, head * dk, (head + 1) * dk, st))
    for s in range(T):
        check(lib.lrpx_aoa_grad_step(ctr, cgs, s, 0, st))
        ops.conv_mfma(gs["gates"], eng.p_gates_grad, rows, 0, 4 * H, W, 1, EPI_PLAIN, pix_per_map=1, oc_split=W, out0=gs["dx"])
        check(lib.lrpx_aoa_grad_step(ctr, cgs, s, 1, st))
    v1 = dense(dense(d_ctx, eng.p_v_rel, H), eng.p_proj_rel, Cc)
    v2 = dense(gs["d_glob"], eng.p_proj_rel, Cc)
    check(lib.lrpx_scale(ptr(v2), ptr(v2), v2.numel(), 1.0 / P, st))
    gs["r_words_norm"] = gs["r_words"].clone()
    check(lib.lrpx_rel_words_norm(ptr(gs["r_words_norm"]), rows, T, st))
    gs["d_feat"] = _nan(rows, P, Cc)
    check(lib.lrpx_aoa_grad_pix(ctr, head, ptr(v1), ptr(v2), ptr(gs["d_feat"]), Cc, st))
    n = len(active)
    buf = _guarded(n * P * Cc)
    check(lib.lrpx_aoa_grad_pix_rows(ctr, head, ptr(v1), ptr(v2), ptr(buf), Cc, ptr(rl), n, st))
    torch.cuda.synchronize()
    assert _bits(_guard_ok(buf, n * P * Cc, "aoa_grad_pix_rows").view(n, P, Cc), gs["d_feat"][rl.long()])
    gs.update(d_ctx=d_ctx, v1=v1, v2=v2)
    live = torch.zeros(rows, dtype=torch.bool)
    live[active] = True
    lv = live.cuda()
    for k in gs:
        assert not torch.isnan(gs[k]).any(), k
    for k in ("gates", "dx", "d_glob", "d_c", "r_words", "r_words_norm", "v2"):
        assert torch.count_nonzero(gs[k][~lv]) == 0, k
    other = torch.ones(H, dtype=torch.bool, device="cuda")
    other[head * dk:(head + 1) * dk] = False
    assert torch.count_nonzero(d_ctx[:, other]) == 0                     # keep_cols
    assert torch.count_nonzero(_upto(gs["r_words"], T) - gs["r_words"]) == 0
    _grade("aoa_grad", T, lens, gs, ("dA", "dB", "d_ctx", "d_h", "d_c", "d_glob", "gates", "dx", "r_words", "r_words_norm", "v1", "v2", "d_feat"), live)
