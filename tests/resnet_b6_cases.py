"""The tensors of the transposed-direction parity test of `lrpx_conv_geom_ex_b6` (tests/test_gpu_resnet_b6.py, test 1), and the
operation it implements in any precision.  tests/test_resnet_b6_host.py decides on the CPU that exactly these tensors are fit for the
fp32-grade criterion of tests/fp64_anchor.py (the six-product emulation passes the bound, the three-product witness misses it by
WITNESS_MARGIN); the GPU test builds them with the same function.

The generator is the one of test_conv_geom_ex_production_widths (tests/test_gpu_resnet_engine.py: seed 300 + k + cin, draws w, x, q, r,
addend in that order) with a heavier tail: r is multiplied by exp(2 randn), drawn right after r, and - the stem only - the weights by
exp(randn), drawn last.  Plain randn data leaves the witness 1.4 - 2.9x above the bound: too close to tell 16-bit-grade arithmetic."""
import torch

from fp64_anchor import emulate

# (id, k, stride, padding, cin, cout, hw, signed)
BWD_CASES = [
    ("pw_2048_512_7", 1, 1, 0, 2048, 512, 7, False),
    ("c3s2_512_14", 3, 2, 1, 512, 512, 14, False),
    ("pws2_256_512_14", 1, 2, 0, 256, 512, 14, False),
    ("stem7_17", 7, 2, 3, 3, 64, 17, True),
    ("c3s2_20_36_11", 3, 2, 1, 20, 36, 11, False),
]
N_MAPS = 3
_CACHE = {}


def bwd_case(name):
    """dict of the CPU tensors (NCHW) of one case; built once per process and shared, read-only"""
    if name in _CACHE:
        return _CACHE[name]
    _, k, stride, padding, cin, cout, hw, signed = next(c for c in BWD_CASES if c[0] == name)
    g = torch.Generator().manual_seed(300 + k + cin)
    ohw = (hw + 2 * padding - k) // stride + 1
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    x = torch.randn(1, cin, hw, hw, generator=g)
    if not signed:
        x = x.clamp(min=0)
    q = torch.rand(1, cout, ohw, ohw, generator=g) + 0.5
    r = torch.randn(N_MAPS, cout, ohw, ohw, generator=g)
    r = r * torch.exp(2 * torch.randn(N_MAPS, cout, ohw, ohw, generator=g))
    n_oc = 8 if signed else cin
    addend = torch.randn(N_MAPS, n_oc, hw, hw, generator=g) * 0.1
    if signed:
        w = w * torch.exp(torch.randn(cout, cin, k, k, generator=g))
    case = dict(name=name, k=k, stride=stride, padding=padding, cin=cin, cout=cout, hw=hw, ohw=ohw, signed=signed, n_oc=n_oc,
                w=w, x=x, q=q, r=r, addend=addend)
    _CACHE[name] = case
    return case


def bwd_reference(case, dtype, pairs=None):
    """out[m] = x * convT(r[m] * q, W+) + addend[m]  (signed input: the halves [x+ convT(., W+) | x- convT(., W-)], then the zero
    columns that carry the addend alone); NCHW.  pairs=None: plainly in `dtype`.  Otherwise in fp64 from those plane products of
    (S = r * q formed in fp32, as the kernel forms it, and the fp32 weights)."""
    c = case
    x, q, r, addend, w = (c[n].to(dtype) for n in ("x", "q", "r", "addend", "w"))
    shape = (r.shape[0],) + tuple(x.shape[1:])
    convT = lambda s, wt: torch.nn.grad.conv2d_input(shape, wt, s, stride=c["stride"], padding=c["padding"])
    if pairs is None:
        s = r * q
        back = lambda wt: convT(s, wt)
    else:
        assert dtype == torch.float64
        s32 = c["r"] * c["q"]
        back = lambda wt: emulate(convT, s32, wt.float(), pairs)
    if not c["signed"]:
        return x * back(w.clamp(min=0)) + addend
    cin = c["cin"]
    halves = torch.cat([x.clamp(min=0) * back(w.clamp(min=0)), x.clamp(max=0) * back(w.clamp(max=0))], 1) + addend[:, :2 * cin]
    return torch.cat([halves, addend[:, 2 * cin:]], 1)


def bwd_device_operands(case):
    """(xs, wb): the kernel's multiplicand (1, cin or 8, H, W) and weight rows (cout, cin or 8, k, k) - the stem runs on the split image
    [x+ | x- | 0 0] with rows [W+ | W- | 0 0]"""
    c = case
    if not c["signed"]:
        return c["x"], c["w"].clamp(min=0)
    cin, k, hw = c["cin"], c["k"], c["hw"]
    xs = torch.cat([c["x"].clamp(min=0), c["x"].clamp(max=0), torch.zeros(1, 8 - 2 * cin, hw, hw)], 1)
    wb = torch.cat([c["w"].clamp(min=0), c["w"].clamp(max=0), torch.zeros(c["cout"], 8 - 2 * cin, k, k)], 1)
    return xs, wb
