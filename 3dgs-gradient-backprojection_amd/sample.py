"""What a finished field says at an arbitrary 3-D point: the Gaussians that weigh on the point by their own shape (scale, rotation,
opacity; csrc/sample.hip), the field blended over them and the weighted vote of a label field -- for the vertices of a benchmark's
mesh, a depth sensor's cloud, COLMAP's sparse points, or the Gaussians of a re-trained scene of the same place.

    pg = point_gaussians(points, means, quats, scales, opacities, k=8)      # idx, weights, n_contrib, radius, grid_stats, ...
    feats, valid = sample_field(field, pg, fallback="nearest")              # [Q, D], bool [Q]
    labels, share = sample_labels(labels3d, num_classes, pg)                # int32 [Q], float32 [Q]
    field2 = transfer_field(means, quats, scales, opacities, field, new_means)[0]
    counts = score_point_labels(labels, gt, num_classes); miou_recall(counts)

THE CONTRACT (include/gwbp.h has the same words).  A Gaussian is live when its mean, quaternion (non-zero norm), scales (> 0) and
opacity (> 0) are finite and its mask entry is set.  Its weight at x is w = o exp(-sigma), sigma = 0.5 |S^-1 R^T (x - mu)|^2, in one
fixed fp32 arrangement; it is kept when sigma <= 80 and w >= alpha_min (default 1/255: a Gaussian counts at a point exactly where
the rasteriser would let it count at a pixel).  The candidates of a point are the live Gaussians whose CENTRE lies within `radius`;
the result is the k candidates of largest kept weight by (weight descending, index ascending), and n_contrib, the number of
candidates with a kept weight (n_contrib > k: the list was truncated).  A pure function of the inputs: not of the grid, the launch
or the order of the walk; two runs give the same bits.  Everything runs on the caller's current stream; there is no PyTorch
fallback: CPU tensors raise GwbpError.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from ._lib import GwbpError, ptr
from ._views import field_rows, ld, out_type, require_device, rows, run
from .components import build_grid, plan_walk, r2_of
from .regions import similarity_quantiles
from .spatial import MAX_K, Grid, as_points, grid_args, grid_stats, sorted_keys, spatial_knn

PACK = 12                  # GWBP_SAMPLE_PACK
ALPHA_MIN = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(255.0, dtype=torch.float32))  # the blend's 1/255
MIN_ALPHA = 1e-30          # GWBP_SAMPLE_MIN_ALPHA
REACH_MARGIN = 1.0 + 1e-4  # suggest_sample_radius: room for the fp32 rounding of sigma at the edge of a Gaussian's reach


class PointGaussians(NamedTuple):
    """idx int32 [Q, k] (tail -1) and weights float32 [Q, k] (tail 0): each point's Gaussians of largest kept weight; n_contrib int32
    [Q]: the candidates with a kept weight (> k: truncated); radius: the one used; grid_stats: spatial.grid_stats() of the search;
    beyond_radius: the share of the live Gaussians whose reach exceeds the radius (they may be missed by points near their rim);
    points / means: what was asked and of what (sample_field's fallback reads them); visited int32 [Q] with return_visited."""
    idx: torch.Tensor
    weights: torch.Tensor
    n_contrib: torch.Tensor
    radius: float
    grid_stats: Optional[dict]
    beyond_radius: float
    points: torch.Tensor
    means: torch.Tensor
    visited: Optional[torch.Tensor] = None


def _alpha_min(alpha_min: float) -> float:
    a = float(alpha_min)
    if not MIN_ALPHA <= a <= 1.0:
        raise GwbpError(f"alpha_min must be in [{MIN_ALPHA}, 1], got {alpha_min}")
    return float(torch.tensor(a, dtype=torch.float32))


def _gaussians(means, quats, scales, opacities):
    """(means [N, 3], quats [N, 4], scales [N, 3], opacities [N]) as the kernels read them."""
    p = as_points(means, "means")
    n = p.shape[0]
    q, s = rows(quats, "quats"), rows(scales, "scales")
    if q.shape != (n, 4) or s.shape != (n, 3):
        raise GwbpError(f"quats must be [N = {n}, 4] and scales [N, 3], got {tuple(q.shape)} and {tuple(s.shape)}")
    if not torch.is_tensor(opacities) or not opacities.is_cuda or opacities.dim() != 1 or opacities.shape[0] != n:
        raise GwbpError(f"opacities must be a HIP tensor [N = {n}]")
    o = opacities.float().contiguous()
    if q.device != p.device or s.device != p.device or o.device != p.device:
        raise GwbpError("means, quats, scales and opacities must be on one device")
    return p, q, s, o


def reach(scales: torch.Tensor, opacities: torch.Tensor, alpha_min: float = ALPHA_MIN) -> torch.Tensor:
    """float64 [N]: how far from its centre a Gaussian can have a kept weight, sqrt(2 ln(o / alpha_min)) x its largest scale; 0 for
    a Gaussian that can have none (o < alpha_min, or a non-finite or non-positive scale or opacity).  Plain torch."""
    s, o = scales.double(), opacities.double().reshape(-1)
    ok = torch.isfinite(s).all(dim=1) & (s > 0).all(dim=1) & torch.isfinite(o) & (o >= float(alpha_min))
    r = torch.sqrt(2.0 * torch.log(torch.where(ok, o, torch.ones_like(o)) / float(alpha_min)).clamp(min=0.0)) * s.max(dim=1).values
    return torch.where(ok, r, torch.zeros_like(r))


def suggest_sample_radius(scales: torch.Tensor, opacities: torch.Tensor, alpha_min: float = ALPHA_MIN, quantile: float = 0.99) -> float:
    """The radius point_gaussians searches centres in by default: the `quantile` of reach() over the Gaussians that can count at
    all, times 1 + 1e-4.  quantile = 1.0 is the radius at which no Gaussian that could count is left out; 0.99 keeps a few huge
    Gaussians from setting the cost for every point (PointGaussians.beyond_radius says how many).  0.0 when nothing can count."""
    if not 0.0 <= float(quantile) <= 1.0:
        raise GwbpError(f"quantile must be in [0, 1], got {quantile}")
    r = reach(scales, opacities, _alpha_min(alpha_min))
    r = r[r > 0]
    if r.numel() == 0:
        return 0.0
    return similarity_quantiles(r, (float(quantile),))[0] * REACH_MARGIN


def point_gaussians(points: torch.Tensor, means: torch.Tensor, quats: torch.Tensor, scales: torch.Tensor, opacities: torch.Tensor,
                    k: int = 8, radius: Optional[float] = None, alpha_min: float = ALPHA_MIN, mask: Optional[torch.Tensor] = None, *,
                    quantile: float = 0.99, cell_size: Optional[float] = None, grid: Optional[Grid] = None,
                    return_visited: bool = False) -> PointGaussians:
    """For every point of points[Q, 3] its k Gaussians of largest kept weight under the module's contract: PointGaussians(idx,
    weights, n_contrib, radius, grid_stats, beyond_radius, points, means).  radius None: suggest_sample_radius(scales, opacities,
    alpha_min, quantile).  mask: bool [N], only these Gaussians take part.  One grid build over the means (cells of max(radius,
    the automatic edge) unless cell_size / grid say otherwise; the result does not depend on it), one pack, one walk.  A
    non-finite point gets the empty result.  Cells that hold thousands of Gaussians make the walk quadratic: see grid_stats."""
    require_device("point_gaussians", means)
    p, q, s, o = _gaussians(means, quats, scales, opacities)
    pts = as_points(points, "points")
    if pts.device != p.device:
        raise GwbpError("points and means must be on one device")
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise GwbpError(f"k must be in [1, {MAX_K}], got {k}")
    a = _alpha_min(alpha_min)
    n, nq, dev = p.shape[0], pts.shape[0], p.device
    live = None
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dim() != 1 or mask.shape[0] != n:
            raise GwbpError(f"mask must be [N = {n}]")
        live = mask.to(dev).bool().to(torch.uint8).contiguous()
    if radius is None:
        radius = suggest_sample_radius(s, o, a, quantile)
    r2 = float("inf") if float(radius) == float("inf") else r2_of(radius)  # (+inf: every finite centre is a candidate)
    idx = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    w = torch.zeros(nq, k, dtype=torch.float32, device=dev)
    n_contrib = torch.zeros(nq, dtype=torch.int32, device=dev)
    visited = torch.zeros(nq, dtype=torch.int32, device=dev) if return_visited else None
    if n == 0:
        return PointGaussians(idx, w, n_contrib, float(radius), None, 0.0, pts, p, visited)
    rch = reach(s, o, a)
    if live is not None:
        rch = torch.where(live.bool(), rch, torch.zeros_like(rch))
    can = rch > 0
    beyond = float((rch > float(radius)).sum()) / max(int(can.sum()), 1)
    g = plan_walk(p, radius if math.isfinite(float(radius)) else 0.0, cell_size, grid)
    sorted_pts, cell_start, perm = build_grid(p, g)
    pack = torch.empty(n, PACK, dtype=torch.float32, device=dev)
    run("gwbp_gaussian_pack", dev, C.c_int64(n), ptr(p), C.c_int64(ld(p)), ptr(q), C.c_int64(ld(q)), ptr(s), C.c_int64(ld(s)), ptr(o),
        ptr(live), ptr(perm), ptr(pack))
    if nq:
        order = sorted_keys(pts, g)[1]
        run("gwbp_point_gaussians", dev, C.c_int64(n), ptr(sorted_pts), ptr(cell_start), *grid_args(g), ptr(pack), C.c_float(r2),
            C.c_float(a), C.c_int64(nq), ptr(pts), C.c_int64(ld(pts)), ptr(order), k, ptr(idx), ptr(w), ptr(n_contrib), ptr(visited))
    return PointGaussians(idx, w, n_contrib, float(radius), grid_stats(g, cell_start), beyond, pts, p, visited)


def _list(idx, weights, dev):
    if not torch.is_tensor(idx) or not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 2 or idx.device != dev:
        raise GwbpError("idx must be an int32 [Q, k] tensor on the device of the features")
    if not torch.is_tensor(weights) or weights.dtype != torch.float32 or weights.shape != idx.shape or weights.device != dev:
        raise GwbpError("weights must be a float32 tensor of idx's shape on its device")
    if not 1 <= idx.shape[1] <= MAX_K:
        raise GwbpError(f"idx must have 1 .. {MAX_K} columns, got {idx.shape[1]}")
    return idx.contiguous(), weights.contiguous()


def neighbor_blend(features: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor, out_dtype=None):
    """(out [Q, D], wsum float32 [Q]): out[g] = sum_j w[g, j] features[idx[g, j]] / sum_j w[g, j], both sums chained in the
    list's order in fp32, over the entries with an index in [0, M) and w != 0 (the others are skipped, their rows not read); a
    zero row and wsum 0 where none is left.  features [M, D] is read in place at any row stride >= D (float16 / bfloat16 as stored,
    widened exactly as they are loaded).  out is float32, or with out_dtype=float16 / bfloat16 the float32 quotient rounded once to
    nearest even by the kernel's store: the bits of out32.to(out_dtype), without the float32 tensor."""
    f, ft = field_rows(features, "features")
    dtype, ot = out_type("neighbor_blend", out_dtype)
    idx, weights = _list(idx, weights, f.device)
    nq, k = idx.shape
    d = f.shape[1]
    out = torch.empty(nq, d, dtype=dtype, device=f.device)
    wsum = torch.empty(nq, dtype=torch.float32, device=f.device)
    run("gwbp_neighbor_blend_out_typed", f.device, C.c_int64(nq), C.c_int64(f.shape[0]), d, k, ptr(idx), ptr(weights), ptr(f), ft,
        C.c_int64(ld(f)), ptr(out), ot, C.c_int64(d), ptr(wsum))
    return out, wsum


def weighted_vote(labels: torch.Tensor, num_classes: int, idx: torch.Tensor, weights: torch.Tensor):
    """(label int32 [Q], share float32 [Q]): the class of largest summed weight among each row's entries (labels outside [0,
    num_classes) and skipped entries take no part), ties to the smallest class, -1 when nothing took part; share = its sum over
    the sum of all that took part."""
    if not torch.is_tensor(labels) or labels.dim() != 1 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise GwbpError("labels must be an integer tensor [M]")
    num_classes = int(num_classes)
    if not 1 <= num_classes <= 2 ** 31 - 1:
        raise GwbpError(f"num_classes must be in [1, 2^31 - 1], got {num_classes}")
    if not labels.is_cuda:
        raise GwbpError("labels must be a HIP tensor (no CPU fallback exists for this path)")
    lab = labels.clamp(min=-1, max=2 ** 31 - 1).to(torch.int32).contiguous()
    idx, weights = _list(idx, weights, lab.device)
    nq, k = idx.shape
    out = torch.empty(nq, dtype=torch.int32, device=lab.device)
    share = torch.empty(nq, dtype=torch.float32, device=lab.device)
    run("gwbp_weighted_vote", lab.device, C.c_int64(nq), C.c_int64(max(lab.shape[0], 1)), k, ptr(idx), ptr(weights), ptr(lab),
        num_classes, ptr(out), ptr(share))
    return out, share


def sample_field(features: torch.Tensor, pg: PointGaussians, fallback: str = "none", fallback_radius: Optional[float] = None, *,
                 return_wsum: bool = False, out_dtype=None):
    """(out [Q, D], valid bool [Q]): the field at pg's points, features[N, D] blended over each point's list by weight;
    valid where a Gaussian counted (wsum > 0), zero rows elsewhere.  fallback "nearest": an invalid finite point instead takes the
    row of the Gaussian with the nearest centre (spatial_knn(means, 1), on those points only, in torch), within fallback_radius if
    one is given; valid stays False there, so the caller can tell the two apart.  return_wsum: also the blend's wsum float32 [Q].
    out is float32, or out_dtype (float16 / bfloat16) as neighbor_blend writes it; the fallback's rows are written in out's dtype."""
    if fallback not in ("none", "nearest"):
        raise GwbpError(f"fallback must be 'none' or 'nearest', got {fallback!r}")
    if not isinstance(pg, PointGaussians):
        raise GwbpError("pg must be point_gaussians()'s result")
    f = field_rows(features, "features")[0]
    if f.shape[0] != pg.means.shape[0]:
        raise GwbpError(f"features must be [N = {pg.means.shape[0]}, D], got {tuple(f.shape)}")
    out, wsum = neighbor_blend(f, pg.idx, pg.weights, out_dtype)
    valid = wsum > 0
    if fallback == "nearest" and pg.means.shape[0] > 0:
        need = torch.nonzero(~valid & torch.isfinite(pg.points).all(dim=1)).squeeze(1)
        if need.numel():
            dist, near = spatial_knn(pg.means, 1, queries=pg.points[need].contiguous())
            ok = near[:, 0] >= 0
            if fallback_radius is not None:
                ok &= dist[:, 0] <= float(fallback_radius)
            out[need[ok]] = f[near[ok, 0].long()].float().to(out.dtype)
    return (out, valid, wsum) if return_wsum else (out, valid)


def fallback_rows(pg: PointGaussians, valid: torch.Tensor) -> int:
    """How many rows a "nearest" fallback would fill: the invalid points with finite coordinates."""
    return int((~valid & torch.isfinite(pg.points).all(dim=1)).sum())


def sample_labels(labels: torch.Tensor, num_classes: int, pg: PointGaussians):
    """(labels int32 [Q], share float32 [Q]) at pg's points.  labels integer [N]: the weighted vote of each point's list.  A soft
    float field [N, K] goes through sample_field: the argmax of the blended class weights (ties to the smallest class, -1 on an
    invalid row) and that class' share of the row's sum."""
    if not isinstance(pg, PointGaussians):
        raise GwbpError("pg must be point_gaussians()'s result")
    if torch.is_tensor(labels) and labels.dim() == 2 and labels.dtype.is_floating_point:
        if labels.shape[1] != int(num_classes):
            raise GwbpError(f"a soft label field must be [N, num_classes = {num_classes}], got {tuple(labels.shape)}")
        soft, valid = sample_field(labels, pg)
        best = soft.max(dim=1)
        total = soft.sum(dim=1)
        share = torch.where(valid & (total != 0), best.values / total, torch.zeros_like(total))
        return torch.where(valid, best.indices.to(torch.int32), torch.full_like(best.indices, -1, dtype=torch.int32)), share
    if not torch.is_tensor(labels) or labels.dim() != 1 or labels.shape[0] != pg.means.shape[0]:
        raise GwbpError(f"labels must be an integer tensor [N = {pg.means.shape[0]}] or a float field [N, num_classes]")
    return weighted_vote(labels, num_classes, pg.idx, pg.weights)


def transfer_field(src_means, src_quats, src_scales, src_opacities, features, dst_means, k: int = 8, radius: Optional[float] = None,
                   alpha_min: float = ALPHA_MIN, mask: Optional[torch.Tensor] = None, fallback: str = "nearest",
                   fallback_radius: Optional[float] = None, out_dtype=None):
    """A field carried onto other Gaussians of the same place (a re-trained or densified scene) without the 2-D network and the lift:
    (field [M, D], valid bool [M], pg) = the source field sampled at the destination's means; out_dtype as in sample_field."""
    pg = point_gaussians(dst_means, src_means, src_quats, src_scales, src_opacities, k, radius, alpha_min, mask)
    out, valid = sample_field(features, pg, fallback, fallback_radius, out_dtype=out_dtype)
    return out, valid, pg


def score_point_labels(pred: torch.Tensor, gt: torch.Tensor, num_classes: int, ignore: int = -1) -> torch.Tensor:
    """int64 [K, 3] counts {intersection, predicted, ground truth} per class over the points whose ground truth is not `ignore` and
    lies in [0, K): miou_recall()'s layout for one table (a prediction outside [0, K), such as -1, counts for no class).  Torch
    bincounts, on pred's device."""
    k = int(num_classes)
    if k < 1:
        raise GwbpError(f"num_classes must be at least 1, got {num_classes}")
    if not torch.is_tensor(pred) or not torch.is_tensor(gt) or pred.dim() != 1 or gt.shape != pred.shape \
            or pred.dtype.is_floating_point or gt.dtype.is_floating_point:
        raise GwbpError("pred and gt must be integer tensors of one shape [Q]")
    p, t = pred.long(), gt.to(pred.device).long()
    scored = (t != int(ignore)) & (t >= 0) & (t < k)
    p, t = p[scored], t[scored]
    inside = (p >= 0) & (p < k)
    inter = torch.bincount(t[p == t], minlength=k)
    return torch.stack([inter, torch.bincount(p[inside], minlength=k), torch.bincount(t, minlength=k)], dim=1)


# ---- seeded inputs (the CLI's --synthetic) -----------------------------------------------------------------------------------------

def synthetic_points(means: torch.Tensor, count: Optional[int] = None, jitter: float = 0.02, far: int = 16, seed: int = 5) -> torch.Tensor:
    """Seeded query points for a scene: `count` (default: as many as means) means drawn with replacement and moved by jitter x the
    scene's extent x a normal sample, followed by `far` points at 100 x the scene's extent, where no Gaussian counts.  [count +
    far, 3] float32 on the device of the means."""
    g = torch.Generator().manual_seed(seed)
    m = means.detach().float().cpu()
    m = m[torch.isfinite(m).all(dim=1)]
    n = m.shape[0]
    count = n if count is None else int(count)
    if n == 0:
        return torch.zeros(0, 3, device=means.device)
    extent = float((m.quantile(0.99, dim=0) - m.quantile(0.01, dim=0)).max()) if n <= 2 ** 24 else float((m.max(0).values - m.min(0).values).max())
    extent = extent if math.isfinite(extent) and extent > 0 else 1.0
    pick = torch.randint(0, n, (count,), generator=g)
    near = m[pick] + jitter * extent * torch.randn(count, 3, generator=g)
    away = m.mean(dim=0) + 100.0 * extent * (torch.rand(int(far), 3, generator=g) * 2 - 1)
    sign = torch.where(away - m.mean(dim=0) >= 0, 1.0, -1.0)
    away = away + 10.0 * extent * sign  # (never closer than 10 extents along any axis)
    return torch.cat([near, away]).to(means.device)
