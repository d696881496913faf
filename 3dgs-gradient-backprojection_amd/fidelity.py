"""How well does a finished feature field reproduce the 2-D maps it was lifted from, and where does it not?

    planes = render_field_agreement(means, quats, scales, opacities, features, feature_map, viewmat, K, W, H)   # [H, W] maps
    table  = score_field_views(means, quats, scales, opacities, features, viewmats, K, W, H, feature_fn)        # float64 [V, 8]
    report = field_fidelity(table)                         # mean cosine, MAE, MSE, relative error: per view and overall
    weight = agreement_weights(planes, cosine_min=0.5)     # a pixel_weight_fn result for a second, robust lift

The literal form is rasterization(colors=features) plus torch arithmetic on an [H, W, D] image.  Both calls here run
gwbp_field_compare (csrc/field_compare.hip) on the caller's current stream instead: the field is rendered from the view's weight
store and compared with the view's map inside the kernel, so only [H, W] planes (or nothing but eight numbers per view) leave it.
With r the rendered row and m the map row of a pixel:

    dot = sum r m     rr = sum r^2     mm = sum m^2     l1 = sum |r - m|     l2 = sum (r - m)^2     cosine = dot / sqrt(rr mm)

The rendered values are rasterization()'s bit for bit, the sums have a fixed order, and there is no atomic: two calls give the same
bits.  There is no PyTorch fallback: CPU tensors raise, and so does a missing library.  field_fidelity and agreement_weights are
plain tensor arithmetic on the results and run wherever their input lives.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

from ._lib import GwbpError
from ._views import field_rows, front, require_device, score_views
from ._views import raster_kw as merged_raster_kw
from .rasterization import get_engine

MAX_D = 2048  # GWBP_PCA_MAX_D
PLANES = ("dot", "rr", "mm", "l1", "l2", "cosine")
TABLE_COLUMNS = ("sum_cosine", "sum_l1", "sum_l2", "sum_mm", "n_valid", "n_bad", "n_pixels", "D")


def _field(fn: str, means, features) -> torch.Tensor:
    require_device(fn, means)
    x = field_rows(features, "features")[0]  # float16 / bfloat16 fields are read as stored: no float32 copy
    if x.shape[0] != means.shape[0]:
        raise GwbpError(f"{x.shape[0]} feature rows for {means.shape[0]} Gaussians")
    if not 1 <= x.shape[1] <= MAX_D:
        raise GwbpError(f"D must be in [1, {MAX_D}], got {x.shape[1]}")
    return x


def _check_upsample(fn: str, upsample: Optional[str]) -> None:
    if upsample == "bilinear":
        raise GwbpError(f"{fn}(upsample='bilinear') is not supported: the comparison reads one map row per pixel.  Pass the "
                        "upsampled [H, W, D] map (F.interpolate(..., mode='bilinear', align_corners=False), as the reference's "
                        "lseg loop builds it) with upsample=None; only upsample='nearest' reads a low-resolution map in place")
    if upsample not in (None, "nearest"):
        raise GwbpError(f"upsample must be None or 'nearest', got {upsample!r}")


def _map_and_index(fn: str, eng, fmap, d: int, width: int, height: int, upsample: Optional[str]):
    """(map, index) as Engine.field_compare takes them: the full-resolution [H, W, D] map, or with upsample="nearest" the
    low-resolution [h, w, D] map and F.interpolate(mode="nearest")'s index maps."""
    if not torch.is_tensor(fmap) or fmap.dim() != 3:
        raise GwbpError(f"the feature map must be a [H, W, D] tensor ([h, w, D] with upsample='nearest'), got "
                        f"{tuple(fmap.shape) if torch.is_tensor(fmap) else type(fmap).__name__}")
    if fmap.shape[2] != d:
        raise GwbpError(f"the field has D = {d}, the map D = {fmap.shape[2]}")
    if upsample is None:
        if tuple(fmap.shape[:2]) != (height, width):
            raise GwbpError(f"the feature map must be [H, W, D] = [{height}, {width}, {d}], got {tuple(fmap.shape)} "
                            "(a low-resolution map needs upsample='nearest')")
        return fmap, None
    return fmap, eng.nearest_maps(int(fmap.shape[0]), int(fmap.shape[1]), height, width)


def render_field_agreement(means, quats, scales, opacities, features, feature_map, viewmat, K, width, height,
                           upsample: Optional[str] = None, **raster_kw) -> Dict[str, torch.Tensor]:
    """The per-pixel agreement of one view: a dict of float32 [H, W] tensors dot, rr, mm, l1, l2 (the five channel sums of the
    module docstring), cosine (NaN where rr mm == 0: nothing rendered there, or an all-zero map row) and alpha (the render's).
    features: float32, float16 or bfloat16 [N, D], any row stride >= D, read as stored (a half field gives the bits of
    features.float(), without that copy); D <= 2048.  feature_map: the view's [H, W, D] map, float32,
    float16 or bfloat16 read as stored, channels contiguous, any non-negative pixel strides; with upsample="nearest" the network's
    low-resolution [h, w, D] map, read through F.interpolate(mode="nearest")'s index maps and never expanded.  A pixel whose map
    row holds a non-finite value is NaN in every plane but alpha.  raster_kw: near_plane, far_plane, eps2d, radius_clip,
    camera_model, rasterize_mode.  The engine and the front cache are rasterization()'s: after a rendered frame of the same view
    nothing is projected or blended again."""
    _check_upsample("render_field_agreement", upsample)
    x = _field("render_field_agreement", means, features)
    kw = merged_raster_kw("render_field_agreement", raster_kw)
    width, height = int(width), int(height)
    fmap, index = _map_and_index("render_field_agreement", get_engine(means.device, means.shape[0], width, height), feature_map,
                                 x.shape[1], width, height, upsample)
    eng, view, alphas = front("render_field_agreement", means, quats, scales, opacities, viewmat, K, width, height, kw,
                              want_alphas=True, want_store=True)
    planes, _ = eng.field_compare(view, x, fmap, index=index)
    out = {name: planes[i] for i, name in enumerate(PLANES)}
    out["alpha"] = alphas
    return out


def score_field_views(means, quats, scales, opacities, features, viewmats, K, width, height,
                      feature_fn: Callable[[int], Optional[torch.Tensor]], upsample: Optional[str] = None,
                      **raster_kw) -> torch.Tensor:
    """table float64 [V, 8] on the device, per view: sum cosine, sum l1, sum l2, sum mm, n_valid, n_bad, n_pixels, D.  A pixel is
    valid when its map row is finite, its five sums are finite and rr mm > 0; the four sums run over the valid pixels; n_bad
    counts the pixels whose map row holds a non-finite value.  feature_fn(v): the view's map as render_field_agreement takes it,
    or None to skip the view (its row stays zero).  viewmats [V, 4, 4]; K [3, 3] or [V, 3, 3].  No plane is written and no
    [H, W] tensor allocated; nothing inside the loop waits for the device: the workspace's capacity is checked once behind it
    (an overflow grows the workspace and runs the views again)."""
    _check_upsample("score_field_views", upsample)
    x = _field("score_field_views", means, features)
    width, height, device = int(width), int(height), means.device

    def per_view(eng, v, table):
        fmap = feature_fn(v)
        if fmap is None:
            return None
        fmap, index = _map_and_index("score_field_views", eng, fmap, x.shape[1], width, height, upsample)
        return lambda view: eng.field_compare(view, x, fmap, index=index, want_planes=False, table=table[v])

    return score_views("score_field_views", means, quats, scales, opacities, viewmats, K, width, height, raster_kw,
                       make_result=lambda: torch.zeros(viewmats.shape[0], 8, dtype=torch.float64, device=device),
                       per_view=per_view, blend=True)


def field_fidelity(table) -> Dict[str, object]:
    """The figures of a score_field_views table ([V, 8], or one view's [8]): mean cosine = sum cosine / n_valid, mean absolute
    error = sum l1 / (n_valid D), MSE = sum l2 / (n_valid D) and relative error = sum l2 / sum mm, per view (float64 [V] tensors
    on the host) and overall (floats; the sums of the views with n_valid > 0 divided alike).  A view with n_valid == 0 -- skipped,
    or one that sees nothing -- has NaN entries and takes no part in the overall figures, which are NaN when no view is left.
    Returns {"per_view": {"cosine", "mae", "mse", "relative"}, "overall": {the same four}, "n_valid": int64 [V], "n_bad": int64 [V],
    "views_scored": int}."""
    t = torch.as_tensor(table).detach().to(device="cpu", dtype=torch.float64)
    if t.dim() == 1:
        t = t[None]
    if t.dim() != 2 or t.shape[1] != 8:
        raise GwbpError(f"table must be [V, 8] or [8], got {tuple(t.shape)}")
    s_cos, s_l1, s_l2, s_mm, n_valid, n_bad, _, d = t.unbind(dim=1)
    live = n_valid > 0
    nan = torch.full_like(s_cos, float("nan"))
    elems = n_valid * d

    def ratio(num, den):
        return torch.where(live, num / torch.where(live, den, torch.ones_like(den)), nan)

    per_view = dict(cosine=ratio(s_cos, n_valid), mae=ratio(s_l1, elems), mse=ratio(s_l2, elems), relative=ratio(s_l2, s_mm))

    def total(num, den):
        den_all = float(den[live].sum())
        return float(num[live].sum()) / den_all if bool(live.any()) and den_all != 0.0 else float("nan")

    overall = dict(cosine=total(s_cos, n_valid), mae=total(s_l1, elems), mse=total(s_l2, elems), relative=total(s_l2, s_mm))
    return dict(per_view=per_view, overall=overall, n_valid=n_valid.to(torch.int64), n_bad=n_bad.to(torch.int64),
                views_scored=int(live.sum()))


def agreement_weights(planes, cosine_min: Optional[float] = None, quantile: Optional[float] = None) -> torch.Tensor:
    """A bool [H, W] pixel-weight map from a view's agreement (render_field_agreement's dict, or its cosine plane alone): True
    where the field built from all views agrees with this view's map, False on transients, bad poses and segmenter noise -- a valid
    pixel_weight_fn result of create_feature_field for a second, robust lift.  Exactly one criterion:
      cosine_min=t   True where cosine >= t
      quantile=q     0 <= q < 1: True where cosine >= the q-quantile of the view's finite cosines (the lowest share q goes)
    A NaN cosine (nothing rendered, a zero or non-finite map row) gives False: such a pixel has nothing to agree with."""
    if (cosine_min is None) == (quantile is None):
        raise GwbpError("agreement_weights takes exactly one of cosine_min and quantile")
    cos = planes["cosine"] if isinstance(planes, dict) else planes
    if not torch.is_tensor(cos) or cos.dim() != 2 or not cos.is_floating_point():
        raise GwbpError("agreement_weights needs render_field_agreement's planes or a floating-point [H, W] cosine plane")
    finite = torch.isfinite(cos)
    if cosine_min is not None:
        return finite & (cos >= float(cosine_min))
    q = float(quantile)
    if not 0.0 <= q < 1.0:
        raise GwbpError(f"quantile must be in [0, 1), got {quantile!r}")
    vals = cos[finite]
    if vals.numel() == 0:
        return torch.zeros_like(finite)
    cut = torch.sort(vals)[0][min(int(q * vals.numel()), vals.numel() - 1)]
    return finite & (cos >= cut)
