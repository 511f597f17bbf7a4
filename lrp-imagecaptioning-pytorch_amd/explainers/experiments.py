"""The device work of the reference's bbox and tpfp experiments (`EvaluationExperiments.bbox_experiment`, evaluation.py:345-448,
`EvaluationExperimentsAOA.bbox_experiment_attention`, :720-771; `tpfp_experiment`, :450-560) on maps of any arm: LRP
(`evaluation.spatial_relevance` + `project_maxabs`), attention (`attention.attention_maps`), Grad-CAM (`attention.gradcam_maps`).

Id-level like explainers/ablation.py: which word matches which category, and the boxes' scaling to the image
(`int(box[i] * resize_ratio[..])`, :420-424), are the caller's; the entry points take maps, pixel boxes and row numbers."""
import torch

from .. import evaluation

THRESHOLDS = (0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)          # evaluation.py:425


def bbox_correctness(spatial, boxes, box2row, thresholds=THRESHOLDS, carry=True):
    """Per row the best correctness score over its boxes, for every threshold (evaluation.py:418-436): spatial (rows, H, W), already
    projected; boxes (nbox, 4) int [x0, y0, x1, y1] in pixels; box2row (nbox,): the row a box belongs to, a row's boxes in the order
    of the reference's `for box in bbox`.  Returns (rows, len(thresholds)); a row without boxes scores 0 (the table's initial value).

    carry=True reproduces the reference: `_calculate_overlaped_pixels` zeroes `relevance[relevance <= threshold]` IN the caller's
    array (:324-326), and that array is reused for every box of the word (:419) - so a row's first box meets the map as it is, and
    every later box a map already cut at the LAST threshold of the first pass: its effective threshold is max(threshold, last).
    carry=False scores every box on the map as it is - the definition the code was written to follow."""
    spatial = evaluation._dev(spatial)
    rows = spatial.shape[0]
    thr = [float(t) for t in thresholds]
    if not thr:
        raise ValueError("bbox_correctness: no thresholds")
    boxes = torch.as_tensor(boxes).to(spatial.device, torch.int64).reshape(-1, 4)
    rows_of = torch.as_tensor(box2row).to(torch.int64).cpu()
    if rows_of.dim() != 1 or rows_of.shape[0] != boxes.shape[0]:
        raise ValueError("bbox_correctness: one row number per box ({} boxes, box2row {})".format(boxes.shape[0], tuple(rows_of.shape)))
    if rows_of.numel() and (int(rows_of.min()) < 0 or int(rows_of.max()) >= rows):
        raise ValueError("bbox_correctness: box2row names a row outside the {} maps".format(rows))
    best = torch.zeros(rows, len(thr), device=spatial.device, dtype=torch.float32)
    seen, first = set(), []
    for r in rows_of.tolist():
        first.append(r not in seen)
        seen.add(r)
    first = torch.tensor(first, dtype=torch.bool)
    for sel, cut in ((first, thr), (~first, [max(t, thr[-1]) for t in thr] if carry else thr)):
        idx = torch.nonzero(sel).flatten()
        if idx.numel() == 0:
            continue
        r = rows_of[idx].to(spatial.device)
        score = evaluation.overlapped_pixels(spatial[r], boxes[idx.to(spatial.device)], cut)
        best.scatter_reduce_(0, r[:, None].expand(-1, len(thr)), score, "amax", include_self=True)      # `if score > table[thr]`
    return best


def tpfp_statistics(spatial, quantiles=None):
    """The statistics row of the tpfp experiment (evaluation.py:506-513; on the raw expanded attention map: :493, :516) per map:
    spatial (N, H, W) -> (stats (N, 4) = mean, mean |x|, mean of the positives (0 without any), max; quantiles (N, len(quantiles)),
    `np.quantile(map, quantiles)`, default i / 100, i = 0 .. 99)."""
    return evaluation.map_statistics(spatial), evaluation.map_quantiles(spatial, quantiles)
