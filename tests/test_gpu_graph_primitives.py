"""The library's clear-then-use patterns, each captured on its own in a HIP graph (`torch.cuda.CUDAGraph`) and replayed: every replay
must give the BITS of the same sequence run eagerly on the same data.  These are the pieces `explain_batch_graph` of both caption engines
is made of (explainers/engine_base.py: `_static_step`); tests/test_gpu_graph_replay.py holds the whole steps to the same bar.

Every test: the sequence once eagerly on a side stream (warm-up, as `_static_step` does), captured from static input tensors, then
four replays.  Before replay k new data is copied into the inputs and every output tensor is filled with NaN; after it the outputs must
be `torch.equal` (as bit patterns) to the eager sequence on that data.  The data of replay k is the base draw times (-1/2)^k: maxima
shrink from replay to replay, so that a stale larger maximum (or the NaN fill) survives a missed or late clear, and sums get data of
the other sign.

What these found: a `hipMemsetAsync` captured as a memset node cleared only on the first launch of the graph; later
launches filled the range with a stray 16-byte pattern.  With the library's clears still on `hipMemsetAsync`,
`test_zeros_then_accumulate` from n = 64 up, the arena test and `test_amax_maps[iter7]` failed (the pattern is reused memory: in a
session where it happened to be zero they passed, while the whole steps of tests/test_gpu_graph_replay.py still failed).  The library
now clears with a kernel while its stream is being captured (csrc/lrpx_core.hip: clear_async)."""
import pytest
import torch

import lrp_amd  # noqa: F401

pytestmark = pytest.mark.gpu

REPLAYS = 4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _nan_fill(t):
    if t.element_size() == 4:
        t.view(torch.float32).fill_(float("nan"))      # (int32 rows of float bits: NaN is above every finite maximum)
    else:
        t.fill_(-1)


def _scaled(base, k):
    """the data of replay k: floats times (-1/2)^k (exact), integer inputs (token ids) rotated by k"""
    return [b * (-0.5) ** k if b.is_floating_point() else torch.roll(b, k, 0) for b in base]


def check_replays(seq, base, scale=_scaled):
    """`seq(*inputs)` -> tuple of output tensors (allocated inside, like a step's).  See the module docstring."""
    static = [b.clone() for b in base]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        seq(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = seq(*static)
    for k in range(REPLAYS):
        data = scale(base, k)
        for s, d in zip(static, data):
            s.copy_(d)
        for o in outs:
            _nan_fill(o)
        graph.replay()
        got = [o.clone() for o in outs]
        want = seq(*data)
        torch.cuda.synchronize()
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and torch.equal(_bits(g), _bits(w)), \
                "replay %d, output %d: %d of %d elements differ from the eager sequence" % (
                    k, i, int((_bits(g) != _bits(w)).sum()), g.numel())
    return outs


def _draw(seed, *shape):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).cuda()


def _accumulate(dst, src):
    from lrp_amd import _lib
    _lib.check(_lib.load().lrpx_accumulate(_lib.ptr(dst.view(torch.float32)), _lib.ptr(src), src.numel(), _lib.stream_ptr()))


TRACE_ARENA = 132800          # floats of `AOAEngine._alloc_trace(4, 5, 36)`: 531 200 bytes


# ---- ops.zeros / ops.zeros_arena, then a kernel that adds into the cleared tensor ------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32], ids=["f32", "i32"])
@pytest.mark.parametrize("n", [1, 3, 64, 65, 4099, TRACE_ARENA, (1 << 20) + 3])
def test_zeros_then_accumulate(n, dtype):
    """(TRACE_ARENA: the one clear of the bottom-up AoA trace at B 4, T 5 - half a megabyte; the last: 4 MiB and an odd tail)"""
    _need_gpu()
    from lrp_amd import ops

    def seq(src):
        z = ops.zeros(n, dtype=dtype)
        _accumulate(z, src)          # (int32: the zero BITS are 0.0f - what the amax rows of a trace rely on)
        return (z,)
    check_replays(seq, [_draw(n, n)])


def test_zeros_arena_views_each_read_by_its_own_kernel():
    """one clear, three views (5, 64 and 130 elements: every view starts on the next multiple of 64 elements)"""
    _need_gpu()
    from lrp_amd import ops
    shapes = {"a": (5,), "b": (64,), "c": (130,)}

    def seq(sa, sb, sc):
        tr = ops.zeros_arena(torch.device("cuda"), shapes)
        for k, s in zip("abc", (sa, sb, sc)):
            _accumulate(tr[k], s)
        return tuple(tr[k] for k in "abc")
    outs = check_replays(seq, [_draw(7 + i, *shapes[k]) for i, k in enumerate("abc")])
    assert outs[1].data_ptr() - outs[0].data_ptr() == 64 * 4 and outs[2].data_ptr() - outs[1].data_ptr() == 64 * 4


# ---- ops.amax_maps: the clear inside the entry point, atomic maxima on top of it --------------------------------------------------------
@pytest.mark.parametrize("n_maps,per", [(1, 4), (3, 36 * 512), (20, 1024 * 7)], ids=["one_float4", "iter9", "iter7"])
def test_amax_maps(n_maps, per):
    _need_gpu()
    from lrp_amd import ops

    def seq(s):
        return (ops.amax_maps(s, n_maps),)
    base = _draw(n_maps, n_maps, per)
    outs = check_replays(seq, [base])
    assert torch.equal(outs[0].view(torch.float32), (base * 0.5 ** (REPLAYS - 1)).abs().amax(1))      # (and the maxima are the data's)


# ---- the decoders' split-product GEMMs and the AoA trace ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aoa_bu():
    """bottom-up AoA engine on the fp16 split products (amax rows, atomics), small vocabulary"""
    if not torch.cuda.is_available():
        return None
    from lrp_amd import weights
    from lrp_amd.explainers.aoa import AOAEngine
    eng = AOAEngine(weights.make_aoa_state(seed=3, vocab_size=203, feat_dim=2048, with_encoder=False))
    eng.force_f16 = True
    return eng


def test_value_rule_records_the_maxima_the_projector_rule_reads(aoa_bu):
    """the two (word, pixel) rules of `AOAEngine.relevance` (explainers/aoa.py) at their smallest shape, n = 2 rows of P = 36 pixels,
    H = 512: the v_proj rule's GEMM reads max|in| from `ops.amax_maps` and raises max|out1| per row in a vector cleared by `ops.zeros`,
    which the projector rule then takes as its operand scale"""
    _need_gpu()
    from lrp_amd import ops
    from lrp_amd._lib import EPI_REL, STAB_EPS
    eng, n, P, H, Cc = aoa_bu, 2, 36, aoa_bu.H, aoa_bu.C
    from lrp_amd import weights
    enc = eng.encode(features=torch.from_numpy(weights.make_bu_features(5, 1)).cuda())
    row2img = torch.zeros(n, dtype=torch.int32, device="cuda")
    U = _draw(11, n, H)
    torch.cuda.synchronize()

    def seq(a_val):
        amax2 = ops.zeros(n, dtype=torch.int32)
        a_proj = torch.empty(n, P, H, device="cuda")
        r_feat = torch.empty(n, P, Cc, device="cuda")
        ops.conv_mfma(a_val, eng.p_v_rel_h, n, 0, H, H, 1, EPI_REL, pix_per_map=P, oc_split=H, x=enc["Vp"], u=U, zdiv=enc["proj_pre"],
                      stab=STAB_EPS, map2img=row2img, out1=a_proj, f16x3=1, in_amax=ops.amax_maps(a_val, n), out1_amax=amax2)
        eng._proj_rule(a_proj, n, P, enc["feats"], row2img, r_feat, kind="f16", in_amax=amax2)
        return amax2, a_proj, r_feat
    outs = check_replays(seq, [_draw(12, n, P, H)])
    assert torch.isfinite(outs[2]).all() and float(outs[2].abs().max()) > 0


@pytest.mark.parametrize("B,T", [(2, 3), (4, 5)])
def test_aoa_decoupled_trace(aoa_bu, B, T):
    """`encode` + `trace`: the trace's arena clear, the three amax rows raised by the gather / attention / gated-sum kernels, the
    split-product GEMMs that scale by them, the (T,V) scores; `h` and `c` hold the only elements of the arena that nothing but the
    clear ever writes, the initial state h[:, 0] = c[:, 0] = 0.  B 4, T 5: the arena of the end-to-end case"""
    _need_gpu()
    from lrp_amd import weights
    eng = aoa_bu
    assert eng.decoupled and eng._f16()
    feats = torch.from_numpy(weights.make_bu_features(6, B)).cuda()
    caps = [torch.from_numpy(weights.make_captions(60 + k, B, T, eng.V)).cuda() for k in range(REPLAYS)]

    def seq(f, c):
        tr = eng.trace(eng.encode(features=f), c, predictions=True)
        return tr["_amax"], tr["hc"], tr["pred"], tr["h"], tr["c"]
    check_replays(seq, [feats, caps[0]], scale=lambda base, k: [base[0] * 0.5 ** k, caps[k]])


# ---- the VGG16 chains ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vgg():
    if not torch.cuda.is_available():
        return None
    from lrp_amd import ops, weights
    from lrp_amd.explainers.gridtd import VGG_PREFIX, _t
    sd = weights.make_gridtd_state(seed=1, vocab_size=107)
    names = [k for k in sd if k.startswith(VGG_PREFIX) and k.endswith(".weight")]
    dev = torch.device("cuda")
    return ops.Vgg16([_t(sd[k], dev) for k in names], [_t(sd[k.replace(".weight", ".bias")], dev) for k in names])


@pytest.mark.parametrize("conv_mode", [1, 3], ids=["mode1", "mode3"])
@pytest.mark.parametrize("streams,n_maps", [(1, 2), (2, 4)], ids=["one_stream", "two_streams"])
def test_vgg16_forward_and_relevance(vgg, streams, n_maps, conv_mode):
    """`Vgg16.forward` + `Vgg16.relevance` of one image: on one stream, and over two (n_maps = 4: the smallest count that takes the
    fork of `relevance` - parallel branches of the captured graph).  Conv mode 3 clears and raises the chains' amax words."""
    _need_gpu()
    from lrp_amd import weights
    vgg.conv_mode = conv_mode
    img = torch.from_numpy(weights.make_images(3, 1)).cuda()
    r_feat = _draw(4, n_maps, 196, 512).abs()
    map2img = torch.zeros(n_maps, dtype=torch.int32, device="cuda")

    def seq(x, r):
        feats = vgg.forward(x)
        return feats, vgg.relevance(r, map2img, streams=streams)
    try:
        outs = check_replays(seq, [img, r_feat])
    finally:
        vgg.conv_mode = None
    assert torch.isfinite(outs[1]).all() and float(outs[1].abs().max()) > 0
