"""Which Gaussians a pixel is made of: per-pixel top-k contributor lists, id maps, median depth and picking -- the 2-D counterpart of
sample.point_gaussians (gsplat users: rasterize_to_indices_in_range, kept to the k heaviest per pixel).

    pg = pixel_gaussians(means, quats, scales, opacities, viewmat, K, W, H, k=4)          # ids, weights, n_contrib, alpha, median_*
    pg = pixel_gaussians(means, quats, scales, opacities, viewmat, K, W, H, k=8, xy=[[x, y]])  # the same rows at a few pixels only
    id_map = render_id_map(means, quats, scales, opacities, viewmat, K, W, H)             # the dominant Gaussian per pixel, -1: none
    inst2d = lookup(id_map, instance_of_gaussian, fill=-1)                                 # a crisp 2-D map of any per-Gaussian table
    depth = median_depth(means, quats, scales, opacities, viewmat, K, W, H)               # the depth at which T falls to one half
    seeds = pick_gaussians(means, quats, scales, opacities, viewmat, K, W, H, xy=[[x, y]])  # a click -> Gaussian indices
    mask3d = select_components(radius_components(means, r), seeds=seeds[:1])               # ... -> the object under the click

Every list comes from gwbp_pixel_gaussians (csrc/pixels.hip) on the caller's current stream, through rasterization()'s engine and front
cache: after a rendered frame of the same view nothing is projected again.  The weights are the blend's alpha T bit for bit; with
k >= n_contrib a pixel's list is its complete row of the view's weight matrix.  There is no PyTorch fallback: CPU tensors raise.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from ._lib import GwbpError
from ._views import front, require_device
from .engine import PIXEL_TOPK_MAX, PROBE_MAX_PIXELS


class PixelGaussians(NamedTuple):
    """ids int32 [..., k] (tail -1) and weights float32 [..., k] (tail 0): each pixel's contributing Gaussians of largest weight alpha T,
    heaviest first, equal weights by id; n_contrib int32 [...]: the contributing Gaussians (> k: the list was cut); alpha [...]: 1 - T;
    median_id int32 [...] / median_depth [...]: the Gaussian after which T <= 0.5 and its camera depth (-1 / 0 where alpha < 0.5).
    [...] is [H, W], or [M] for a call with xy."""
    ids: torch.Tensor
    weights: torch.Tensor
    n_contrib: torch.Tensor
    alpha: torch.Tensor
    median_id: Optional[torch.Tensor]
    median_depth: Optional[torch.Tensor]


def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= PIXEL_TOPK_MAX:
        raise GwbpError(f"k must be an int in [1, {PIXEL_TOPK_MAX}], got {k!r}")
    return k


def _check_xy(xy, device) -> Optional[torch.Tensor]:
    if xy is None:
        return None
    t = torch.as_tensor(xy)
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool or t.numel() == 0 or t.numel() % 2 or \
            (t.dim() > 1 and t.shape[-1] != 2):
        raise GwbpError("xy must be [M, 2] integer (x, y) pixels")
    t = t.reshape(-1, 2)
    if not 1 <= t.shape[0] <= PROBE_MAX_PIXELS:
        raise GwbpError(f"the number of pixels must be in [1, {PROBE_MAX_PIXELS}], got {t.shape[0]}")
    return t.to(device=device, dtype=torch.int32)


def pixel_gaussians(means, quats, scales, opacities, viewmat, K, width, height, k: int = 4, xy=None, want_median: bool = True,
                    **raster_kw) -> PixelGaussians:
    """PixelGaussians of one view: every pixel ([H, W, ...]), or the pixels xy [M, 2] ((x, y) integers, M <= 4096) only ([M, ...]) --
    the same bits as those rows of the full result; a pixel outside the image gets an empty list.  1 <= k <= 16.  raster_kw:
    near_plane, far_plane, eps2d, radius_clip, camera_model, rasterize_mode.  The engine and the front cache are rasterization()'s."""
    k = _check_k(k)
    xy = _check_xy(xy, means.device)
    require_device("pixel_gaussians", means)
    eng, view, _ = front("pixel_gaussians", means, quats, scales, opacities, viewmat, K, width, height, raster_kw)
    return PixelGaussians(*eng.pixel_gaussians(view, k, xy, want_median=want_median))


def render_id_map(means, quats, scales, opacities, viewmat, K, width, height, **raster_kw) -> torch.Tensor:
    """int32 [H, W]: the Gaussian of largest weight at every pixel (the lowest id among equals), -1 where nothing contributes."""
    return pixel_gaussians(means, quats, scales, opacities, viewmat, K, width, height, 1, want_median=False, **raster_kw).ids[..., 0]


def median_depth(means, quats, scales, opacities, viewmat, K, width, height, **raster_kw) -> torch.Tensor:
    """float32 [H, W]: the camera depth of the Gaussian at which the transmittance falls to one half -- a depth at which something
    lies, unlike the blended depth between a foreground edge and its background; 0 where alpha stays below one half."""
    return pixel_gaussians(means, quats, scales, opacities, viewmat, K, width, height, 1, **raster_kw).median_depth


def lookup(id_map: torch.Tensor, table: torch.Tensor, fill=0) -> torch.Tensor:
    """table[id_map] with `fill` where id_map is -1: a crisp map of any per-Gaussian attribute ([N] labels, instance ids, cluster
    codes, or [N, C] colours), unmixed at silhouettes.  The result has the table's dtype (a half table stays half) and the shape
    id_map.shape + table.shape[1:].  Plain torch, on the table's device."""
    if not torch.is_tensor(id_map) or id_map.is_floating_point() or id_map.dtype == torch.bool:
        raise GwbpError("id_map must be an integer tensor of Gaussian ids (-1: none)")
    if not torch.is_tensor(table) or table.dim() < 1:
        raise GwbpError("table must be a [N, ...] tensor")
    ids = id_map.to(table.device)
    out = table[ids.clamp_min(0).long()]
    out[ids < 0] = fill
    return out


def ranked_ids(ids: torch.Tensor, weights: torch.Tensor, min_weight: float = 0.0) -> torch.Tensor:
    """int64 [U]: the distinct ids >= 0 of the lists whose weight is above min_weight, by their largest weight descending, equal
    weights by id ascending.  Plain torch."""
    keep = (ids >= 0) & (weights > min_weight)
    i, w = ids[keep].long(), weights[keep].float()
    if i.numel() == 0:
        return i
    uniq, inv = torch.unique(i, return_inverse=True)  # ascending ids
    best = torch.zeros(uniq.shape[0], dtype=w.dtype, device=w.device).scatter_reduce_(0, inv, w, "amax", include_self=False)
    return uniq[torch.sort(best, descending=True, stable=True).indices]


def pick_gaussians(means, quats, scales, opacities, viewmat, K, width, height, xy, k: int = 4, min_weight: float = 0.0,
                   **raster_kw) -> torch.Tensor:
    """int64 [U]: the Gaussians under the clicks xy [M, 2] -- the distinct entries of the clicks' top-k lists with a weight above
    min_weight, heaviest first: indices for select_components(seeds=...) and run_instances.py --seed-index."""
    if xy is None:
        raise GwbpError("pick_gaussians needs xy, the clicked (x, y) pixels")
    pg = pixel_gaussians(means, quats, scales, opacities, viewmat, K, width, height, k, xy, want_median=False, **raster_kw)
    return ranked_ids(pg.ids, pg.weights, min_weight)


def dominance_counts(pg, n_gaussians: int) -> torch.Tensor:
    """int64 [n_gaussians]: the number of pixels each Gaussian dominates (heads its list) in pg, a PixelGaussians or an id map.  Summed
    over views, counts > 0 is a mask of the Gaussians that are the surface somewhere.  Plain torch."""
    ids = pg.ids[..., 0] if isinstance(pg, PixelGaussians) else pg
    ids = ids.reshape(-1)
    ids = ids[ids >= 0].long()
    if ids.numel() and int(ids.max()) >= n_gaussians:
        raise GwbpError(f"the lists name Gaussian {int(ids.max())}, n_gaussians = {n_gaussians}")
    return torch.bincount(ids, minlength=int(n_gaussians))
