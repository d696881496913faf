"""Per-Gaussian labels back on the image plane: class maps, their argmax, the counts behind mIoU and recall, and the tinted scene
(the last stage of the reference's label pipeline: evaluate_results and render_affordance of
affordance_transfer/demo_affordance_transfer.py:1445-1611, 1399-1439).

    maps, alphas = render_label_maps(means, quats, scales, opacities, labels, K_classes, viewmat, K, W, H)   # [H, W, K], [H, W]
    seg = render_label_argmax(means, quats, scales, opacities, labels, K_classes, viewmat, K, W, H)          # int32 [H, W]
    counts = score_label_views(means, quats, scales, opacities, labels, K_classes, viewmats, K, W, H, gt_fn) # int64 [V, K, 3]
    metrics = miou_recall(counts)
    tinted = recolor_by_labels(splats, labels, palette)

All three renders run gwbp_render_labels (csrc/label_render.hip) on the caller's current stream: one blend pass per view with one
int per Gaussian as its payload -- no one-hot [N, K] table, no [H, W, K] image unless asked for, and for the score no image at
all: threshold, comparison with the ground truth and the counts happen in the kernel.  There is no PyTorch fallback: CPU tensors
raise, and so does a missing library.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence

import torch

from ._lib import GwbpError
from ._views import front, score_views

C0 = 0.28209479177387814  # the SH basis' constant term, 1 / sqrt(4 pi)


def render_label_maps(means, quats, scales, opacities, labels, num_classes: int, viewmat, K, width, height, **raster_kw):
    """(maps float32 [H, W, num_classes], alphas [H, W]) of one view: maps[y, x, k] is the opacity the Gaussians of label k
    contribute to the pixel, sum_g w_g(p) [labels[g] == k] -- bit for bit what rasterization() renders from the one-hot
    [N, num_classes] table, which is never built.  labels: integer [N] on the device; a label outside [0, num_classes) adds to
    alphas and to no class.  raster_kw: near_plane, far_plane, eps2d, radius_clip, camera_model, rasterize_mode.  The engine and
    the front cache are rasterization()'s: a label render after a rendered frame of the same view projects nothing."""
    eng, view, _ = front("render_label_maps", means, quats, scales, opacities, viewmat, K, width, height, raster_kw)
    maps, alphas, _, _ = eng.render_labels(view, labels, num_classes)
    return maps, alphas


def render_label_argmax(means, quats, scales, opacities, labels, num_classes: int, viewmat, K, width, height,
                        min_opacity: float = 0.0, **raster_kw):
    """The 2-D segmentation of one view, int32 [H, W]: per pixel the class of the largest opacity (the lowest index among equals),
    -1 where no class contributes or that opacity lies below min_opacity.  No [H, W, num_classes] image is made."""
    eng, view, _ = front("render_label_argmax", means, quats, scales, opacities, viewmat, K, width, height, raster_kw)
    return eng.render_labels(view, labels, num_classes, want_maps=False, want_alphas=False, want_argmax=True,
                             min_opacity=min_opacity)[2]


def score_label_views(means, quats, scales, opacities, labels, num_classes: int, viewmats, K, width, height,
                      gt_fn: Callable[[int], Optional[torch.Tensor]], cut: int = 64, **raster_kw) -> torch.Tensor:
    """counts int64 [V, num_classes, 3] on the device: per view and class the pixels of {intersection, predicted, ground truth},
    where predicted is the reference's mask of the class' rendered indicator, uint8(clamp(render, 0, 1) * 255) > cut
    (demo_affordance_transfer.py:1555-1578: one render and one device-to-host copy per class there), and ground truth is
    gt_fn(v) == class.  gt_fn(v): the view's integer [H, W] label map, or None to skip the view (the reference skips the views
    whose gt_type is "automatic"); a skipped view's row stays zero.  Values of the map outside [0, num_classes) match no class.
    viewmats [V, 4, 4]; K [3, 3] or [V, 3, 3].  Nothing inside the loop waits for the device: the workspace's capacity is
    checked once behind it (an overflow grows the workspace and runs the views again)."""
    n_classes, device = int(num_classes), means.device

    def per_view(eng, v, counts):
        gt = gt_fn(v)
        if gt is None:
            return None
        return lambda view: eng.render_labels(view, labels, n_classes, want_maps=False, want_alphas=False, gt=gt, counts=counts[v],
                                              cut=cut)

    return score_views("score_label_views", means, quats, scales, opacities, viewmats, K, width, height, raster_kw,
                       make_result=lambda: torch.zeros(viewmats.shape[0], max(n_classes, 0), 3, dtype=torch.int64, device=device),
                       per_view=per_view, blend=False)


def miou_recall(counts, classes: Optional[Sequence[int]] = None, n_present: Optional[int] = None) -> Dict[str, object]:
    """The reference's bookkeeping (demo_affordance_transfer.py:1579-1611) on counts [V, K, 3] ({intersection, predicted, ground
    truth}; score_label_views, or one view's [K, 3]): per view and class union = predicted + ground truth - intersection; a
    class' IoU list takes intersection / union of the views with union > 0, its recall list intersection / ground truth of those
    that also have ground truth > 0; mIoU and recall are the sums of the per-class means of the non-empty lists divided by
    n_present.  classes: the scored classes, by default 1 ... K-1 (class 0 is the reference's background).  n_present: the
    reference divides by the number of distinct ground-truth labels OF ITS LAST VIEW minus one; the default is the number of
    scored classes with any ground truth in any view (pass the reference's figure to reproduce its number).
    Returns {"iou": {class: mean or None}, "recall": {class: mean or None}, "miou": float, "mean_recall": float, "n_present": int}
    (NaN for both means when n_present is 0)."""
    c = torch.as_tensor(counts).detach().cpu().to(torch.int64)
    if c.dim() == 2:
        c = c[None]
    if c.dim() != 3 or c.shape[2] != 3:
        raise GwbpError(f"counts must be [V, K, 3] or [K, 3], got {tuple(c.shape)}")
    k = c.shape[1]
    classes = list(range(1, k)) if classes is None else [int(i) for i in classes]
    if any(not 0 <= i < k for i in classes):
        raise GwbpError(f"classes {classes} outside [0, {k})")
    iou: Dict[int, Optional[float]] = {}
    rec: Dict[int, Optional[float]] = {}
    for i in classes:
        ious, recs = [], []
        for inter, pred, truth in c[:, i].tolist():
            union = pred + truth - inter
            if union == 0:
                continue
            ious.append(inter / union)
            if truth == 0:
                continue
            recs.append(inter / truth)
        iou[i] = sum(ious) / len(ious) if ious else None
        rec[i] = sum(recs) / len(recs) if recs else None
    if n_present is None:
        n_present = sum(1 for i in classes if int(c[:, i, 2].sum()) > 0)
    n_present = int(n_present)
    nan = float("nan")
    return dict(iou=iou, recall=rec, n_present=n_present,
                miou=sum(x for x in iou.values() if x is not None) / n_present if n_present else nan,
                mean_recall=sum(x for x in rec.values() if x is not None) / n_present if n_present else nan)


def recolor_by_labels(splats: Dict[str, torch.Tensor], labels: torch.Tensor, palette, mix: float = 0.5,
                      rest_scale: float = 0.1) -> Dict[str, torch.Tensor]:
    """The tint of render_affordance (demo_affordance_transfer.py:1410-1416) as one tensor expression: a copy of the splats dict
    whose SH coefficients show every Gaussian's label,
        features_dc   <- mix * features_dc + (1 - mix) * (palette[label] - 0.5) / C0     C0 = 0.28209479177387814
        features_rest <- rest_scale * features_rest
    palette: [P, 3] colours in [0, 1]; a Gaussian whose label lies outside [0, P) keeps its DC coefficient.  Everything else of
    the dict is shared.  The reference scales the higher-order coefficients INSIDE its loop over the eight classes, so by 0.1^8:
    that is a bug (it merely removes them); here they are scaled once."""
    dc, rest = splats["features_dc"], splats["features_rest"]
    pal = torch.as_tensor(palette, dtype=dc.dtype, device=dc.device).reshape(-1, 3)
    lab = labels.to(dc.device).long().reshape(-1)
    if lab.shape[0] != dc.shape[0]:
        raise GwbpError(f"{lab.shape[0]} labels for {dc.shape[0]} Gaussians")
    known = (lab >= 0) & (lab < pal.shape[0])
    tint = ((pal[lab.clamp(0, pal.shape[0] - 1)] - 0.5) / C0).reshape(dc.shape)  # dc: [N, 1, 3] (or [N, 3])
    new_dc = torch.where(known.reshape(-1, *([1] * (dc.dim() - 1))), mix * dc + (1.0 - mix) * tint, dc)
    out = dict(splats)
    out["features_dc"], out["features_rest"] = new_dc, rest_scale * rest
    return out
