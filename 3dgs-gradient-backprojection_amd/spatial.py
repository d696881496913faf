"""Which Gaussians are next to each other in space: exact Euclidean k-NN of the means on a uniform grid (csrc/spatial.hip), and what
a finished lift wants from it -- a majority vote over neighbours for per-Gaussian labels and masks, statistical outlier removal, a
neighbour average of a noisy field -- plus the reference trainer's scale initialisation (f3dgs/utils_simple_trainer.py:141-145
knn(), f3dgs/simple_trainer_feature_3dgs.py:200-203).

    dist, idx = spatial_knn(means, 8)                               # sklearn's NearestNeighbors(8).fit(x).kneighbors(x)
    labels = smooth_labels(means, labels, num_classes, k=8, neighbors=idx)
    keep = remove_outliers(means, mask3d, k=8, std_ratio=2.0)
    field = smooth_features(means, field, neighbors=idx)
    log_scales = init_scales(points)

Everything runs on the caller's current stream; the grid is chosen on the host from a sample (plan_grid: plumbing, torch).  There is
no PyTorch fallback: CPU tensors raise GwbpError.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Tuple

import torch

from ._lib import GwbpError, ptr
from ._views import field_rows, ld, out_type, rows, run
from .transfer import narrow_source_labels, vote_labels

MAX_K = 32
MAX_DIM = 1024          # GWBP_SPATIAL_MAX_DIM: cells per axis
MAX_CELLS = 1 << 24     # GWBP_SPATIAL_MAX_CELLS
MIN_CELL = 1e-30        # GWBP_SPATIAL_MIN_CELL
SAMPLE = 65536          # points plan_grid looks at
POINTS_PER_CELL = 4.0   # the automatic cell size aims at this many points per cell of the occupied box


class Grid(NamedTuple):
    """Cubic cells of edge h over a box that starts at lo, dims = (nx, ny, nz) cells; the border cells extend to infinity."""
    lo: Tuple[float, float, float]
    h: float
    dims: Tuple[int, int, int]

    @property
    def cells(self) -> int:
        return self.dims[0] * self.dims[1] * self.dims[2]


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def plan_grid(points: torch.Tensor, cell_size: Optional[float] = None, points_per_cell: float = POINTS_PER_CELL) -> Grid:
    """The grid spatial_knn builds for points[N, 3] (any device; a pure function of its arguments).  The box is the per-axis 1 % /
    99 % quantiles of a fixed-stride sample of at most 65 536 points, finite ones only, so that far floaters land in border cells
    instead of stretching the grid.  cell_size None: h such that the box holds points_per_cell points per cell, counting only the
    axes along which the box has an extent; raised until the box fits into 1024 cells per axis and 2^24 cells in all.  A given
    cell_size is kept, and a box that needs more cells than that is cut down around its centre (the search stays exact: border
    cells extend to infinity).  h > 0 always; a box without any extent, or a sample without a finite point, gives one cell."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise GwbpError(f"points must be [N, 3], got {tuple(points.shape)}")
    n = int(points.shape[0])
    if cell_size is not None and not (math.isfinite(cell_size) and cell_size >= MIN_CELL):
        raise GwbpError(f"cell_size must be finite and at least {MIN_CELL}, got {cell_size}")
    stride = max(1, -(-n // SAMPLE))
    sample = points[::stride][:SAMPLE].detach().float()
    sample = sample[torch.isfinite(sample).all(dim=1)]
    if sample.shape[0] == 0:
        lo, hi = [0.0] * 3, [0.0] * 3
    else:
        q = torch.quantile(sample, torch.tensor([0.01, 0.99], device=sample.device), dim=0).cpu()
        lo, hi = [float(v) for v in q[0]], [float(v) for v in q[1]]
    ext = [max(hi[a] - lo[a], 0.0) for a in range(3)]
    ext = [e if math.isfinite(e) else 0.0 for e in ext]
    live = [e for e in ext if e > 0.0]
    if cell_size is not None:
        h = _f32(cell_size)
    elif not live:
        h = 1.0
    else:
        volume = math.prod(live)
        h = (points_per_cell * volume / max(n, 1)) ** (1.0 / len(live))
        h = max(h, max(live) / MAX_DIM)
        h = _f32(h)
        if not (math.isfinite(h) and h >= MIN_CELL):
            h = _f32(max(max(live), MIN_CELL))

    def dims_of(h):
        return [min(max(int(math.ceil(e / h)), 1), MAX_DIM) if e > 0.0 else 1 for e in ext]

    dims = dims_of(h)
    if cell_size is None:
        while math.prod(dims) > MAX_CELLS:
            h = _f32(h * 1.125)
            dims = dims_of(h)
    else:
        while math.prod(dims) > MAX_CELLS:
            a = dims.index(max(dims))
            dims[a] = (dims[a] + 1) // 2
    # centre what the grid covers on the box (it covers at least the box unless the caps cut it)
    lo = [_f32(lo[a] + 0.5 * (ext[a] - dims[a] * h)) if ext[a] > 0.0 else _f32(lo[a] - 0.5 * h) for a in range(3)]
    return Grid((lo[0], lo[1], lo[2]), h, (dims[0], dims[1], dims[2]))


def _check_grid(grid: Grid) -> Grid:
    lo, h, dims = tuple(float(v) for v in grid.lo), float(grid.h), tuple(int(d) for d in grid.dims)
    if len(lo) != 3 or len(dims) != 3:
        raise GwbpError("grid: lo and dims have three entries")
    return Grid(lo, h, dims)


def _points(t: torch.Tensor, name: str) -> torch.Tensor:
    t = rows(t, name)
    if t.shape[1] != 3:
        raise GwbpError(f"{name} must be [N, 3], got {tuple(t.shape)}")
    if t.shape[0] >= 2 ** 31:
        raise GwbpError(f"{name}: {t.shape[0]} rows; indices are int32")
    return t


def _grid_args(grid: Grid):
    return (C.c_float(grid.lo[0]), C.c_float(grid.lo[1]), C.c_float(grid.lo[2]), C.c_float(grid.h), grid.dims[0], grid.dims[1],
            grid.dims[2])


def _sorted_keys(p: torch.Tensor, grid: Grid):
    keys = torch.empty(p.shape[0], dtype=torch.int32, device=p.device)
    run("gwbp_spatial_cell_keys", p.device, C.c_int64(p.shape[0]), ptr(p), C.c_int64(ld(p)), *_grid_args(grid), ptr(keys))
    return torch.sort(keys, stable=True)


# what components.py (the radius components on the same grid) shares with this module
as_points, check_grid, grid_args, sorted_keys = _points, _check_grid, _grid_args, _sorted_keys


def grid_stats(grid: Grid, cell_start: torch.Tensor) -> dict:
    """What a search on this grid costs: cells, occupied cells, the largest and the 99th-percentile occupancy (over the occupied
    cells), and the points that sit in cells at all (the finite ones)."""
    occ = (cell_start[1:] - cell_start[:-1])
    occ = occ[occ > 0]
    n_occ = int(occ.numel())
    p99 = int(occ.sort().values[min(n_occ - 1, int(math.ceil(0.99 * n_occ)) - 1)]) if n_occ else 0
    return {"lo": list(grid.lo), "cell_size": grid.h, "dims": list(grid.dims), "cells": grid.cells, "occupied_cells": n_occ,
            "max_occupancy": int(occ.max()) if n_occ else 0, "p99_occupancy": p99, "points_in_cells": int(cell_start[-1])}


def spatial_knn(points: torch.Tensor, k: int, queries: Optional[torch.Tensor] = None, cell_size: Optional[float] = None, *,
                grid: Optional[Grid] = None, return_stats: bool = False):
    """For every query the k points of points[N, 3] of smallest Euclidean distance: (dist[Q, k] float32, idx[Q, k] int32), each
    row sorted by distance ascending, then index ascending.  queries None: the points themselves (sklearn's kneighbors(x) on the
    fitted data): self is a neighbour like any other, at distance 0 in column 0 unless a duplicate with a smaller index ties.

    Exact: squared distance is fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32 with dx = p.x - q.x, dist its correctly rounded sqrt,
    and the result does not depend on the grid (cell_size, or a whole Grid through grid=; default plan_grid), only the time does.
    A point with a non-finite coordinate is nobody's neighbour and gets idx -1 / dist NaN as a query; a query with fewer than k
    finite points gets -1 / +inf in the tail.  1 <= k <= 32, k <= N.  points / queries are read in place at any row stride >= 3
    (a [:, :3] slice of a wider tensor).  No atomics; two runs give the same bits.
    return_stats: also grid_stats() of the search (this waits for the device)."""
    p = _points(points, "points")
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise GwbpError(f"k must be in [1, {MAX_K}], got {k}")
    n = p.shape[0]
    if k > n:
        raise GwbpError(f"k = {k} exceeds the number of points N = {n}")
    grid = _check_grid(grid) if grid is not None else plan_grid(p, cell_size)
    dev = p.device
    skeys, perm = _sorted_keys(p, grid)
    pts = torch.empty(n, 4, dtype=torch.float32, device=dev)
    cell_start = torch.empty(grid.cells + 1, dtype=torch.int32, device=dev)
    run("gwbp_spatial_build", dev, C.c_int64(n), ptr(p), C.c_int64(ld(p)), ptr(skeys), ptr(perm), C.c_int64(grid.cells), ptr(pts),
        ptr(cell_start))
    if queries is None:
        q, order = p, perm
    else:
        q = _points(queries, "queries")
        if q.device != dev:
            raise GwbpError("points and queries must be on one device")
        order = _sorted_keys(q, grid)[1]
    nq = q.shape[0]
    idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
    dist = torch.empty(nq, k, dtype=torch.float32, device=dev)
    run("gwbp_spatial_knn", dev, C.c_int64(n), ptr(pts), ptr(cell_start), *_grid_args(grid), C.c_int64(nq), ptr(q),
        C.c_int64(ld(q)), ptr(order), k, ptr(idx), ptr(dist))
    return (dist, idx, grid_stats(grid, cell_start)) if return_stats else (dist, idx)


def knn_distances(points: torch.Tensor, K: int = 4) -> torch.Tensor:
    """The reference's knn(x, K) (utils_simple_trainer.py:141-145): the distances [N, K] of every point to its K nearest
    neighbours, itself first, on the device instead of sklearn on a host copy."""
    return spatial_knn(points, K)[0]


def scales_from_distances(dist: torch.Tensor, init_scale: float = 1.0) -> torch.Tensor:
    """simple_trainer_feature_3dgs.py:201-203 on knn(points, 4): log(sqrt(mean of the squared distances to the 3 nearest
    neighbours) * init_scale), repeated over the three axes -> [N, 3]."""
    dist2_avg = (dist[:, 1:] ** 2).mean(dim=-1)
    dist_avg = torch.sqrt(dist2_avg)
    return torch.log(dist_avg * init_scale).unsqueeze(-1).repeat(1, 3)


def init_scales(points: torch.Tensor, init_scale: float = 1.0) -> torch.Tensor:
    """The reference trainer's initial log-scales [N, 3]: the size of a Gaussian is the root mean square distance to its three
    nearest neighbours (simple_trainer_feature_3dgs.py:200-203)."""
    return scales_from_distances(knn_distances(points, 4), init_scale)


def _neighbors(means: torch.Tensor, k: int, neighbors: Optional[torch.Tensor]) -> torch.Tensor:
    if neighbors is None:
        return spatial_knn(means, k)[1]
    if not torch.is_tensor(neighbors) or not neighbors.is_cuda or neighbors.dtype != torch.int32 or neighbors.dim() != 2 \
            or neighbors.shape[0] != means.shape[0]:
        raise GwbpError("neighbors must be spatial_knn's int32 [N, k] device tensor for these means")
    return neighbors


def smooth_labels(means: torch.Tensor, labels: torch.Tensor, num_classes: int, k: int = 8, iterations: int = 1,
                  neighbors: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Each Gaussian's label replaced by the majority label among its k spatial neighbours (itself included), ties to the smallest
    label; int32 [N].  Labels outside [0, num_classes) count as -1: ignored by the vote, and kept where every neighbour is
    ignored.  Each iteration votes on the labels of the one before.  neighbors: a precomputed idx[N, k'] of spatial_knn(means,
    k'), so that one search serves several calls (k is then not used)."""
    if not means.is_cuda:
        raise GwbpError("smooth_labels() needs HIP tensors (there is no CPU path)")
    idx = _neighbors(means, k, neighbors)
    lab, nc = narrow_source_labels(labels, num_classes)
    lab = lab.to(idx.device)
    if lab.shape[0] != idx.shape[0]:
        raise GwbpError(f"{lab.shape[0]} labels for {idx.shape[0]} Gaussians")
    for _ in range(int(iterations)):
        lab = vote_labels(idx, lab, nc)
    return lab


def smooth_mask(means: torch.Tensor, mask: torch.Tensor, k: int = 8, min_fraction: float = 0.5, iterations: int = 1,
                neighbors: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bool form: a Gaussian is in the result when at least min_fraction of its k spatial neighbours (itself included; the
    valid ones) are in the mask.  bool [N]."""
    if not means.is_cuda:
        raise GwbpError("smooth_mask() needs HIP tensors (there is no CPU path)")
    idx = _neighbors(means, k, neighbors)
    if mask.dim() != 1 or mask.shape[0] != idx.shape[0]:
        raise GwbpError(f"mask must be [N = {idx.shape[0]}], got {tuple(mask.shape)}")
    m = mask.to(idx.device).bool()
    for _ in range(int(iterations)):
        _, counts = vote_labels(idx, m.to(torch.int32), 2, return_counts=True)
        valid = counts.sum(dim=1)
        m = (counts[:, 1].double() >= float(min_fraction) * valid.double()) & (valid > 0)
    return m


def outlier_keep(dist: torch.Tensor, std_ratio: float = 2.0) -> torch.Tensor:
    """remove_outliers' statistics on dist[M, 1 + k] of a self-search (column 0 is the point itself): a row's quantity is the mean
    of its finite distances in columns 1.., in float64; rows above mean + std_ratio * std (std over M - 1) of that quantity over
    the rows that have one are dropped, and so are rows without any finite distance.  bool [M]."""
    d = dist[:, 1:].double()
    ok = torch.isfinite(d)
    cnt = ok.sum(dim=1)
    md = torch.where(ok, d, torch.zeros_like(d)).sum(dim=1) / cnt.clamp(min=1)
    have = cnt > 0
    vals = md[have]
    if vals.numel() < 2:
        return have
    limit = vals.mean() + float(std_ratio) * vals.std()
    return have & ~(md > limit)


def remove_outliers(means: torch.Tensor, mask: Optional[torch.Tensor] = None, k: int = 8, std_ratio: float = 2.0) -> torch.Tensor:
    """Statistical outlier removal as a keep-mask, bool [N]: within mask (all Gaussians if None) the Gaussians whose mean distance
    to their k nearest neighbours WITHIN THE SUBSET (itself not counted, so the search asks for k + 1 <= 32) exceeds the subset's
    mean + std_ratio * std of that quantity are dropped.  Gaussians outside mask stay outside."""
    if not means.is_cuda:
        raise GwbpError("remove_outliers() needs HIP tensors (there is no CPU path)")
    if not 1 <= int(k) <= MAX_K - 1:
        raise GwbpError(f"k must be in [1, {MAX_K - 1}], got {k}")
    p = _points(means, "means")
    n = p.shape[0]
    if mask is None:
        sel = torch.arange(n, device=p.device)
    else:
        if mask.dim() != 1 or mask.shape[0] != n:
            raise GwbpError(f"mask must be [N = {n}], got {tuple(mask.shape)}")
        sel = torch.nonzero(mask.to(p.device).bool()).squeeze(1)
    keep = torch.zeros(n, dtype=torch.bool, device=p.device)
    m = int(sel.numel())
    if m == 0:
        return keep
    kk = min(int(k) + 1, m)
    sub = p if mask is None else p[sel]
    dist, _ = spatial_knn(sub, kk)
    keep[sel] = outlier_keep(dist, std_ratio) if kk > 1 else torch.ones(m, dtype=torch.bool, device=p.device)
    return keep


def neighbor_mean(features: torch.Tensor, idx: torch.Tensor, out_dtype=None) -> torch.Tensor:
    """out[i, :] = the mean of features[idx[i, j], :] over the valid j (idx >= 0), summed in the list's order in fp32; a zero row
    where none is valid.  features [M, D] is read in place at any row stride >= D (float16 / bfloat16 as stored, widened exactly as
    they are loaded); the result is a new [N, D] tensor: float32, or with out_dtype=float16 / bfloat16 the float32 mean rounded once
    to nearest even by the kernel's store (the bits of out32.to(out_dtype), without the float32 tensor)."""
    f, ft = field_rows(features, "features")
    dtype, ot = out_type("neighbor_mean", out_dtype)
    if not torch.is_tensor(idx) or not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 2 or idx.device != f.device:
        raise GwbpError("idx must be an int32 [N, k] tensor on the device of the features")
    idx = idx.contiguous()
    n, k = idx.shape
    if not 1 <= k <= MAX_K:
        raise GwbpError(f"idx must have 1 .. {MAX_K} columns, got {k}")
    d = f.shape[1]
    out = torch.empty(n, d, dtype=dtype, device=f.device)
    run("gwbp_neighbor_mean_out_typed", f.device, C.c_int64(n), C.c_int64(f.shape[0]), d, k, ptr(idx), ptr(f), ft, C.c_int64(ld(f)),
        ptr(out), ot, C.c_int64(d))
    return out


def smooth_features(means: torch.Tensor, features: torch.Tensor, k: int = 8, neighbors: Optional[torch.Tensor] = None,
                    out_dtype=None) -> torch.Tensor:
    """The field averaged over each Gaussian's k spatial neighbours (itself included, uniform weights): a new [N, D] tensor, float32
    or (out_dtype) float16 / bfloat16 as neighbor_mean writes it."""
    if not means.is_cuda:
        raise GwbpError("smooth_features() needs HIP tensors (there is no CPU path)")
    if features.dim() != 2 or features.shape[0] != means.shape[0]:
        raise GwbpError(f"features must be [N = {means.shape[0]}, D], got {tuple(features.shape)}")
    return neighbor_mean(features, _neighbors(means, k, neighbors), out_dtype)


# ---- seeded inputs (the CLI's --synthetic, tools/time_spatial.py) -----------------------------------------------------------------

def synthetic_labels(means: torch.Tensor, num_classes: int = 6, flip: float = 0.05, seed: int = 0):
    """Labels from a Voronoi partition of space (num_classes seeded sites among the means) with a seeded fraction flipped to
    another class: (noisy[N] int64, clean[N] int64), on the device of the means."""
    g = torch.Generator().manual_seed(seed)
    n = means.shape[0]
    sites = means[torch.randperm(n, generator=g)[:num_classes].to(means.device)]
    clean = torch.cdist(means.float(), sites.float()).argmin(dim=1)
    flips = (torch.rand(n, generator=g) < flip).to(means.device)
    shift = torch.randint(1, max(num_classes, 2), (n,), generator=g).to(means.device)
    return torch.where(flips, (clean + shift) % num_classes, clean), clean


def synthetic_mask(means: torch.Tensor, floaters: float = 0.01, seed: int = 1):
    """A mask with seeded floaters: the Gaussians nearest to a seeded site (a ball holding a quarter of them), plus a seeded
    fraction of all the others switched on.  (mask[N] bool, clean[N] bool)."""
    g = torch.Generator().manual_seed(seed)
    n = means.shape[0]
    site = means[int(torch.randint(0, n, (1,), generator=g))]
    d = (means.float() - site.float()).norm(dim=1)
    clean = d <= d.kthvalue(max(n // 4, 1)).values
    noise = (torch.rand(n, generator=g) < floaters).to(means.device)
    return clean | noise, clean


def clustered_points(n: int, clusters: int = 64, floaters: float = 0.001, seed: int = 0) -> torch.Tensor:
    """A seeded stand-in for a real scene's uneven density: a mixture of `clusters` isotropic Gaussians with centres in the unit
    cube and sigmas log-uniform over two decades (1e-3 .. 1e-1), plus a fraction of far floaters at 100 x the scene's size.
    [n, 3] float32 on the host."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.rand(clusters, 3, generator=g)
    sigma = 10.0 ** (-3.0 + 2.0 * torch.rand(clusters, generator=g))
    which = torch.randint(0, clusters, (n,), generator=g)
    pts = centres[which] + sigma[which, None] * torch.randn(n, 3, generator=g)
    far = torch.rand(n, generator=g) < floaters
    pts[far] = 100.0 * (torch.rand(int(far.sum()), 3, generator=g) * 2 - 1)
    return pts
