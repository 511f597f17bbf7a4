"""The other arms of the reference's experiments: the model's own attention and 2-D Grad-CAM maps at image size.

The reference compares LRP against the attention weights of the explained step (evaluation.py:198-211 ablation, :390-400 bbox, :483-494
tpfp, :744-750 `bbox_experiment_attention`) and against Grad-CAM (:125-132, :401-407, :496-501).  Both are (P,) maps on the feature grid,
taken to the image by `skimage.transform.pyramid_expand` and, for the ablation and bbox experiments, `_project_maxabs`.  The engines keep
`alpha` (B, T, P) - AoA: (B, T, NH, P) - and gridTD / AdaAtt `beta` (B, T) in every trace; `ops.expand_maps` (csrc/lrpx_expand.hip) is the
one kernel behind the functions here.  The maps go to the consumers of `lrp_amd.evaluation` and `explainers.ablation.image_ablation`
like any other saliency.

Functions, not engine methods: the engines' and drop-ins' public names are frozen (tests/test_explainer_api_host.py)."""
import torch

from .. import ops
from .ragged import ragged


def _image_grid(engine, P, what):
    """(p, hw): the feature grid of P pixels and the image size it came from.  The reference's `args.height // attention_size`: the
    encoders' strides are fixed - VGG16 16 (224 -> 14), the ResNets 32 (448 -> 14, models/gridTDmodel.py:26-31)."""
    if getattr(engine, "cnn", None) is None:
        raise ValueError("{}: {} has no encoder - its features are regions, there is no image grid to expand to".format(
            what, type(engine).__name__))
    p = int(round(P ** 0.5))
    if p * p != P:
        raise ValueError("{}: {} feature pixels are not a square grid".format(what, P))
    return p, p * (32 if engine.resnet else 16)


def _valid_rows(x, lens, device):
    """(B, T, ...) -> (rows, ...): the valid (image, word) rows, image-major - the order `explain_batch` returns maps in"""
    B, T = x.shape[0], x.shape[1]
    flat = x.reshape((B * T,) + tuple(x.shape[2:]))
    if lens is None:
        return flat.contiguous()
    rg = ragged(lens, B, T, device)
    return flat[rg.rows.to(torch.int64)].contiguous()


def attention_maps(engine, tr, lens=None, head=None, normalize=True):
    """The attention weights of every explained word at image size: tr["alpha"] (B, T, P) or (B, T, NH, P) -> (rows, H, W), rows the
    valid (image, word) pairs (all B * T without `lens`).  head=None on a multi-head trace is the mean over the heads
    (`np.mean(attention, axis=0)`, evaluation.py:202), head=k that head (:744).  normalize=True: `_project_maxabs` (:209, :400, :750);
    the tpfp statistics (:493, :516) read the raw map, normalize=False."""
    alpha = tr["alpha"]
    p, hw = _image_grid(engine, alpha.shape[-1], "attention_maps")
    if alpha.dim() == 3 and head is not None:
        raise ValueError("attention_maps: head = {} on a single-head trace {}".format(head, tuple(alpha.shape)))
    return ops.expand_maps(_valid_rows(alpha, lens, engine.device), hw, head=head, normalize=normalize)


def one_minus_beta(tr, lens=None):
    """`1 - betas[t]` of every valid row (evaluation.py:514, :547): the share of the step's context that came from the image"""
    if "beta" not in tr:
        raise ValueError("one_minus_beta: this trace has no sentinel gate (the AoA model has none)")
    beta = tr["beta"]
    return 1.0 - _valid_rows(beta, lens, beta.device)


def gradcam_maps(engine, cam, normalize=False):
    """2-D Grad-CAM maps at image size: cam (..., P) as `explain_batch_gradient(cam=True)` / `(kind="gradcam")` returns it ->
    (rows, H, W), rows = the leading dimensions flattened.  normalize=True is the bbox experiment's map (evaluation.py:401-407),
    normalize=False the ablation's and the tpfp statistics' (:125-132, :496-501)."""
    p, hw = _image_grid(engine, cam.shape[-1], "gradcam_maps")
    return ops.expand_maps(cam.reshape(-1, cam.shape[-1]).contiguous(), hw, normalize=normalize)
