"""Mirror of the reference's LRPtools/lrp_wrapper.py: `add_lrp(model)` + `model.compute_lrp(sample, target=...)`.

The reference installs a forward hook and a legacy backward hook on every leaf and lets autograd drive the
relevance pass (lrp_wrapper.py:37-87).  Here `add_lrp` validates the same leaf -> rule table and attaches a
`compute_lrp` with the same signature and return value.  Two drivers behind it:
  * the VGG16 encoder (features[0:-1], what every explainer of the reference passes): weights packed once, the pass
    is the fused HIP chain `lrpx_vgg16_forward` + `lrpx_vgg16_relevance` (no autograd, no per-word forward with dead
    wgrad work);
  * ANY other leaf sequence (the reference's ResNet-style stacks with BatchNorm / Add / Flatten / Linear, small test
    nets): the model's own forward runs once under forward hooks that keep `module.input` (lrp_wrapper.py:24-25) and
    record the call order; the relevance then walks the recorded calls in reverse through this repo's rule classes
    (lrp_modules.py, HIP kernels), summing where a tensor feeds several modules - what autograd does for the reference.
    Each rule sees the input of the call it answers for, so one module may be called several times.  This carries the reference's
    bottleneck ResNets (resnet50 / resnet101: 7x7 s2 stem, MaxPool2d(3, 2, 1), 1x1 / 3x3 s2 / 1x1 blocks with a registered `Add`);
    their unused `AdaptiveAvgPool2d` leaf is accepted and only refused if a forward reaches it.  `BasicBlock` nets (resnet18 / 34)
    build an unregistered `Add()` inside `forward` (models/resnet.py:87): no hook sees it, and they stay refused by the
    "functional code" error below.
`add_lrp(model, lrp_params=...)` lays a dict over the preset's parameters (the reference's add_lrp has the comment "Override default
parameters if provided" and no argument): the VGG16 encoder with another alpha / beta and `ignore_bias=True` runs the batched
`ops.Vgg16.relevance_alpha_beta`, with `ignore_bias=False` the generic driver.
For a bottleneck ResNet under the preset `add_lrp` additionally attaches `model.compute_lrp_maps(images, targets, map2img=None, conv_mode=0)`:
the batched engine `ops.ResNetEncoder` (one trace per image, one map per target row, no hooks, no `.grad`; conv_mode=1: its
contractions in the exact bf16-split arithmetic).  Under any other alpha / beta it attaches `model.compute_lrp_maps_ab`
instead: the same contract with the model's alpha / beta, on `ops.ResNetEncoder.relevance_alpha_beta`.  `compute_lrp` is
unchanged.
Improvement over the reference: `add_lrp` is idempotent (the reference stacks hooks on every call, which
multiplies its cost without changing the result)."""
import torch
import torch.nn as nn

from . import lrp_modules
from .. import _lib, ops
from .._lib import check, ptr, stream_ptr


class SequentialPresetA(object):
    def __init__(self):
        self.lrp_params = {"alpha": 1., "beta": 0., "ignore_bias": True}      # lrp_wrapper.py:7-12


VGG16_FEATURES = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512]


def _leaves(model):
    return [m for m in model.modules() if len(list(m.children())) == 0]


def _match_vgg16(leaves):
    """True if the leaves are conv3x3+ReLU / MaxPool2d(2,2) in the VGG16 'D' order without the last pool
    (models/vgg.py:62-81, models/gridTDmodel.py:34)."""
    i, cin = 0, 3
    for v in VGG16_FEATURES:
        if i >= len(leaves):
            return False
        m = leaves[i]
        if v == 'M':
            if not isinstance(m, nn.MaxPool2d):
                return False
            i += 1
        else:
            if not (isinstance(m, nn.Conv2d) and m.in_channels == cin and m.out_channels == v and
                    m.kernel_size == (3, 3) and m.padding == (1, 1) and i + 1 < len(leaves) and
                    isinstance(leaves[i + 1], nn.ReLU)):
                return False
            cin = v
            i += 2
    return i == len(leaves)


# The one rule-less leaf type `add_lrp` lets through: the reference's ResNet encoders carry `self.avgpool = nn.AdaptiveAvgPool2d`
# (models/resnet.py:176) and their forward never calls it (:232-234), so the reference's lazy hooks never notice it.  A recorded forward
# that does reach one gets the table's ValueError("Layer type ... not known.") from `compute_lrp`.
_DEFERRED_LEAVES = (nn.AdaptiveAvgPool2d,)


def merge_lrp_params(lrp_params=None):
    """`lrp_params` laid over the preset's (lrp_wrapper.py:7-12; the reference's add_lrp carries the comment "Override default
    parameters if provided" where this happens here).  ValueError for a non-finite alpha / beta.  Host logic: no device."""
    params = dict(SequentialPresetA().lrp_params)
    params.update(lrp_params or {})
    lrp_modules.alpha_beta_params(params)
    return params


def add_lrp(model, lrp_params=None):
    """Attach `model.compute_lrp`.  Leaf -> rule as in lrp_wrapper.py:42-56 (Conv2d/MaxPool2d: alpha_beta,
    ReLU: identity); unknown leaves raise ValueError like `get_lrp_module`.
    lrp_params: a dict laid over the preset {"alpha": 1., "beta": 0., "ignore_bias": True}, kept on the model and handed to every
    rule (Conv2d reads all three, Linear `ignore_bias`); `add_lrp(model)` is the preset.  A model that matches the VGG16 encoder:
    the preset runs the fused chain; ignore_bias=True with any other alpha / beta the batched `ops.Vgg16.relevance_alpha_beta`;
    ignore_bias=False the generic leaf driver - correct, layer by layer through the rule classes, not fast."""
    params = merge_lrp_params(lrp_params)
    leaves = _leaves(model)
    for m in leaves:
        if type(m) in _DEFERRED_LEAVES:
            continue
        lrp_modules.get_lrp_module(m)                     # ValueError("Layer type ... not known.")
        if isinstance(m, nn.Conv2d):
            lrp_modules.conv_rule_params(m, params)       # ValueError: ignore_bias=False on a conv without bias
    model._lrpx_params = params
    if not _match_vgg16(leaves) or not params["ignore_bias"]:
        _add_lrp_generic(model, leaves)
        _attach_resnet_engine(model, params)
        return
    old = model.__dict__.pop("_lrpx_hooks", None)         # (a generic driver installed by an earlier add_lrp(..., ignore_bias=False))
    for h in old or ():
        h.remove()
    convs = [m for m in leaves if isinstance(m, nn.Conv2d)]
    dev = convs[0].weight.device
    if dev.type != "cuda":
        raise _lib.LrpxError("add_lrp: the model must live on the GPU (no CPU path)")
    zeros = lambda c: torch.zeros(c, device=dev)
    ctx = ops.Vgg16([c.weight.detach().float() for c in convs],
                    [c.bias.detach().float() if c.bias is not None else zeros(c.out_channels) for c in convs])
    model._lrpx_ctx = ctx
    model.compute_lrp = lambda sample, **kwargs: compute_lrp(model, sample, **kwargs)


def _attach_resnet_engine(model, params):
    """`model.compute_lrp_maps` for a bottleneck ResNet under the preset (ops.match_bottleneck_resnet), `model.compute_lrp_maps_ab`
    under any other alpha / beta (`ignore_bias` either way: the matcher refuses convs with bias, so it cannot matter); any other model:
    both attributes are absent.  Installs no hooks; the engine (packed weights) is built at the first call."""
    for key in [k for k in model.__dict__ if k.startswith("_lrpx_resnet") or k in ("compute_lrp_maps", "compute_lrp_maps_ab")]:
        del model.__dict__[key]
    preset = SequentialPresetA().lrp_params
    is_preset = params == preset
    if not is_preset and (params["alpha"], params["beta"]) == (preset["alpha"], preset["beta"]):
        return
    try:
        ops.match_bottleneck_resnet(model)
    except ValueError:
        return
    if is_preset:
        model.compute_lrp_maps = lambda images, targets, map2img=None, conv_mode=0: compute_lrp_maps(model, images, targets, map2img, conv_mode)
    else:
        model.compute_lrp_maps_ab = lambda images, targets, map2img=None, conv_mode=0: compute_lrp_maps_ab(model, images, targets, map2img,
                                                                                                         conv_mode)


def _resnet_engine_pass(model, images, targets, map2img, conv_mode, who):
    """trace `images` on the model's engine of `conv_mode` (built on first use) and check `targets`: (engine, targets NHWC)"""
    key = "_lrpx_resnet" if conv_mode == 0 else "_lrpx_resnet_mode{}".format(conv_mode)
    eng = model.__dict__.get(key)
    if eng is None:
        eng = ops.ResNetEncoder(model, conv_mode=conv_mode)
        setattr(model, key, eng)
    feats = eng.forward(images.detach())
    hw = eng.feat_hw
    if targets.dim() != 4 or tuple(targets.shape[1:]) != (feats.shape[2], hw[0], hw[1]):
        raise ValueError("{}: targets must be (n_maps, {}, {}, {}), got {}".format(who, feats.shape[2], hw[0], hw[1], tuple(targets.shape)))
    return eng, ops.nchw_to_nhwc(targets.detach().to(torch.float32))


def compute_lrp_maps(model, images, targets, map2img=None, conv_mode=0):
    """The batched form of `compute_lrp` for the bottleneck ResNet encoders: `images` (B, 3, H, W) are traced ONCE and every row of
    `targets` (n_maps, C, h, w) NCHW - the relevance at the encoder's output - becomes one map (n_maps, 3, H, W) on the trace of image
    map2img[m] (int32 tensor on the device; None: n_maps == B, map m on image m).  Runs `ops.ResNetEncoder` (built on first use from
    the model's weights as they are then; `add_lrp(model)` again after changing them), not the hooks of the generic driver.  Each map
    equals what `compute_lrp` returns for (that image, that target) on a FRESH sample tensor: this function does not touch `.grad` -
    it neither reads nor accumulates into `images.grad` - and returns the maps themselves, not a running sum.  Like `compute_lrp` it
    asserts the result is finite and not all zero (lrp_wrapper.py:81).  conv_mode: the engine's arithmetic (`ops.ResNetEncoder`: 0 fp32
    MFMA, 1 exact bf16 split); the model keeps one engine per mode, `model._lrpx_resnet` for mode 0."""
    eng, t_nhwc = _resnet_engine_pass(model, images, targets, map2img, conv_mode, "compute_lrp_maps")
    r = eng.relevance(t_nhwc, map2img)
    ops.check_relevance(r, finite=True, nonzero=True)
    return r


def compute_lrp_maps_ab(model, images, targets, map2img=None, conv_mode=0):
    """`compute_lrp_maps` under the alpha / beta `add_lrp(model, lrp_params=...)` left on the model: the general alpha-beta rule of
    every Conv2d (lrp_modules.py:124-150), everything else as there; the same per-mode engines.  Each map equals what `compute_lrp`
    (the generic driver, under the same parameters) returns on a fresh sample tensor.  A non-finite result is refused like there:
    with beta != 0 the relevance grows by about (alpha + beta) per conv, which can leave fp32's range on a deep net."""
    alpha, beta, _ = lrp_modules.alpha_beta_params(getattr(model, "_lrpx_params", None))
    eng, t_nhwc = _resnet_engine_pass(model, images, targets, map2img, conv_mode, "compute_lrp_maps_ab")
    r = eng.relevance_alpha_beta(t_nhwc, map2img, alpha, beta)
    ops.check_relevance(r, finite=True, nonzero=True)
    return r


def compute_lrp(model, sample, target=None, return_output=False, rectify_logits=False, explain_diff=False):
    """lrp_wrapper.compute_lrp (:63-87): relevance of `target` (N,512,14,14) propagated to `sample` (N,3,224,224).
    Like the reference, the result ACCUMULATES in `sample.grad` across calls on the same tensor (autograd's
    `.grad` semantics, :66-82) and the returned tensor is a clone of that running sum."""
    ctx = model._lrpx_ctx
    lib = _lib.load()
    if sample.requires_grad is False:
        sample.requires_grad = True
    if target is None:
        raise ValueError("compute_lrp needs `target` (the reference passes the anchor to backward(), :80)")
    if ctx is None:                                              # any leaf sequence: recorded forward + reverse walk
        r, logits_g = _compute_lrp_generic(model, sample, target, return_output)
        feats = None
    else:
        x = sample.detach().to(torch.float32).contiguous()
        feats = ctx.forward(x)                                   # (N,196,512) NHWC
        t_nhwc = ops.nchw_to_nhwc(target.detach().to(torch.float32))
        alpha, beta, _ = lrp_modules.alpha_beta_params(getattr(model, "_lrpx_params", None))
        r = ctx.relevance(t_nhwc, None) if (alpha, beta) == (1., 0.) else ctx.relevance_alpha_beta(t_nhwc, None, alpha, beta)
    if sample.grad is None:
        sample.grad = r
    else:
        check(lib.lrpx_accumulate(ptr(sample.grad), ptr(r), r.numel(), stream_ptr()))
    ops.check_relevance(sample.grad, finite=True, nonzero=True)  # `assert sample.grad.sum()!=0` (:81)
    output = sample.grad.clone().detach()
    if return_output:
        logits = logits_g if feats is None else ops.nhwc_to_nchw(feats.contiguous(), 512, 14, 14)
        return output, logits
    return output


# ------------------------------------------------------------------------------------------------
# generic driver: any leaf sequence the rule table knows (lrp_wrapper.py:37-59 hooks every leaf of any model)
# ------------------------------------------------------------------------------------------------
def _rule_name(module):
    """lrp_wrapper.py:42-56: Linear / BatchNorm -> 'epsilon', ReLU -> 'identity', everything else 'alpha_beta'"""
    if type(module) in (nn.Linear, nn.BatchNorm2d, nn.BatchNorm1d):
        return 'epsilon'
    if type(module) == nn.ReLU:
        return 'identity'
    return 'alpha_beta'


def _key(t):
    """Tensors are matched between a producer's output and a consumer's input by their memory: an in-place ReLU returns
    its input, `x.view(...)` between two modules shares the storage - both keep the relevance flowing, as autograd's view /
    in-place tracking does for the reference."""
    return (t.data_ptr(), t.numel())


def _add_lrp_generic(model, leaves):
    for t in list(model.parameters()) + list(model.buffers()):
        if t.device.type != "cuda":
            raise _lib.LrpxError("add_lrp: the model must live on the GPU (no CPU path)")
    old = model.__dict__.pop("_lrpx_hooks", None)
    for h in old or ():
        h.remove()                                        # idempotent: never two hooks per leaf
    tape = []

    def save_input_hook(module, input_, output):          # lrp_wrapper.py:24-25 (+ the call order)
        module.input = input_
        tape.append((module, input_, output))
    model._lrpx_hooks = [m.register_forward_hook(save_input_hook) for m in leaves]
    model._lrpx_tape = tape
    model._lrpx_ctx = None
    model.compute_lrp = lambda sample, **kwargs: compute_lrp(model, sample, **kwargs)


def _compute_lrp_generic(model, sample, target, return_output):
    lib = _lib.load()
    if sample.device.type != "cuda":
        raise _lib.LrpxError("compute_lrp: the sample must live on the GPU (no CPU path)")
    lrp_params = getattr(model, "_lrpx_params", None) or SequentialPresetA().lrp_params
    tape = model._lrpx_tape
    del tape[:]
    with torch.no_grad():
        logits = model(sample.detach())                   # the model's own forward; the hooks record it
    if not isinstance(logits, torch.Tensor):
        raise ValueError("compute_lrp: the model must return one tensor (the anchor of the relevance pass, :69-80)")
    target = target.detach().to(device=logits.device, dtype=torch.float32)
    if target.shape != logits.shape:
        raise RuntimeError("Mismatch in shape: grad_output[0] has a shape of {} and output[0] has a shape of {}."
                           .format(target.shape, logits.shape))                      # what backward(anchor) raises
    rel = {_key(logits): target.contiguous().clone()}
    r_sample = None
    for module, inputs, output in reversed(tape):
        if not isinstance(output, torch.Tensor):
            raise ValueError("compute_lrp: leaf {} returned {}, not a tensor".format(type(module).__name__, type(output)))
        r_out = rel.pop(_key(output), None)
        if r_out is None:
            continue                                      # a leaf whose output does not reach the anchor
        r_out = r_out.view(output.shape)
        rule = lrp_modules.get_lrp_module(module)         # (ValueError for a deferred leaf the forward did reach)
        # the input of THIS call: a module called several times (the one ReLU of a Bottleneck, models/resnet.py:115-138) otherwise
        # shows every rule the input of its last call
        module.input = inputs
        # `relevance_input` only fixes the arity of the rule's result (lrp_modules.py:157-170): one entry per module input,
        # the incoming relevance first (the identity gradient of Dropout in eval mode, :248-254)
        r_in = rule.propagate_relevance(module, (r_out,) + (None,) * 2, (r_out,), _rule_name(module), lrp_params=lrp_params)
        tensors_in = [t for t in inputs if isinstance(t, torch.Tensor)]
        if isinstance(rule, lrp_modules.Linear):          # the reference's Linear returns (grad_bias slot, R, grad_weight slot)
            r_in = (r_in[1],)
        for t, r in zip(tensors_in, r_in[:len(tensors_in)]):
            r = r.detach().to(torch.float32).reshape(t.shape).contiguous()
            if _key(t) == _key(sample) or t is sample:
                if r_sample is None:
                    r_sample = r.clone()
                else:
                    check(lib.lrpx_accumulate(ptr(r_sample), ptr(r), r.numel(), stream_ptr()))
                continue
            k = _key(t)
            if k in rel:                                  # the tensor feeds several modules: relevance adds up
                acc = rel[k]
                check(lib.lrpx_accumulate(ptr(acc), ptr(r), r.numel(), stream_ptr()))
            else:
                rel[k] = r.clone() if r.data_ptr() == r_out.data_ptr() else r
    if rel:
        raise ValueError("compute_lrp: {} tensor(s) between the leaf modules were produced by functional code (x + y, "
                         "torch.flatten, F.relu ...): the rules see leaf modules only - use explicit Add / Flatten modules as "
                         "the reference's models/resnet.py:25-38 does".format(len(rel)))
    if r_sample is None:
        raise ValueError("compute_lrp: no recorded leaf consumes the sample tensor")
    return r_sample, logits
