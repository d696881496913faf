"""Which Gaussians form one object: connected components of the means under "within a radius of each other, and in the same group"
(csrc/components.hip), as DBSCAN with a deterministic border rule -- PCL's Euclidean cluster extraction, Open3D's cluster_dbscan,
sklearn's DBSCAN, which the reference would run on a host copy like its only neighbour search (f3dgs/utils_simple_trainer.py:141-145)
-- and the small layer that turns the components of a 3-D mask or of a label field into instances a user can select.

    res = radius_components(means, radius, min_points=4, mask=mask3d)         # labels[N], sizes[C], core[N]
    keep = select_components(res, seeds=[clicked], largest=3, min_size=200)   # bool [N]
    inst = split_instances(means, labels, radius=None, min_size=200)          # instance ids by size, and each instance's class
    counts = radius_count(means, radius)                                      # neighbours within the radius, itself included

THE CONTRACT (include/gwbp.h has the same words).  d2(p, q) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32 with dx = p.x - q.x,
spatial_knn's; r2 = float32(radius) * float32(radius), rounded once.  A point is live when its coordinates are finite and its
group is >= 0 (no group: every finite point).  i and j are neighbours when both are live, in one group, and d2 <= r2; a point is its
own neighbour; radius = 0 joins exact duplicates.  count[i] is the number of neighbours of i, core means count >= min_points
(sklearn's min_samples).  Core points joined by a chain of core points, each a neighbour of the next, are one component; a live
non-core point with a core neighbour is a border point of the component of its nearest core neighbour by (d2, index) (sklearn's
rule, first come first served, depends on the visiting order; this one does not); everything else is noise, label -1.  Components
are numbered by their smallest core member's index.  With min_points = 1 every live point is core: plain Euclidean clustering.
The result is a pure function of the inputs -- not of the grid, the launch or the order in which lanes run -- and two runs give the
same bits.  Everything runs on the caller's current stream; there is no PyTorch fallback: CPU tensors raise GwbpError.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence

import torch

from ._lib import GwbpError, ptr
from ._views import ld, run
from .spatial import MAX_K, Grid, as_points, check_grid, grid_args, grid_stats, plan_grid, sorted_keys, spatial_knn

INT32_MAX = 2 ** 31 - 1


class Components(NamedTuple):
    """labels int32 [N]: the component of every point, -1 for noise; sizes int64 [C]: members per component, border points included;
    core bool [N]; grid_stats: spatial.grid_stats() of the search with return_stats, else None."""
    labels: torch.Tensor
    sizes: torch.Tensor
    core: torch.Tensor
    grid_stats: Optional[dict] = None


class Instances(NamedTuple):
    """instances int32 [N]: instance ids in descending order of size (ties to the smaller component id), -1 for dropped points;
    sizes int64 [I]; classes int64 [I]: each instance's class (0 for a mask); core bool [N]; radius: the one used; grid_stats."""
    instances: torch.Tensor
    sizes: torch.Tensor
    classes: torch.Tensor
    core: torch.Tensor
    radius: float
    grid_stats: Optional[dict] = None

    @property
    def labels(self) -> torch.Tensor:  # (what select_components reads)
        return self.instances


def _r2(radius: float) -> float:
    radius = float(radius)
    if not (math.isfinite(radius) and radius >= 0.0):
        raise GwbpError(f"radius must be finite and >= 0, got {radius}")
    r = torch.tensor(radius, dtype=torch.float32)
    return float(r * r)  # the fp32 product, rounded once


def _group(group, mask, n: int, dev, what: str = "group") -> Optional[torch.Tensor]:
    if group is not None and mask is not None:
        raise GwbpError("give group or mask, not both")
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dim() != 1 or mask.shape[0] != n:
            raise GwbpError(f"mask must be [N = {n}]")
        return torch.where(mask.to(dev).bool(), 0, -1).to(torch.int32)
    if group is None:
        return None
    if not torch.is_tensor(group) or group.dim() != 1 or group.shape[0] != n or group.dtype.is_floating_point or group.dtype == torch.bool:
        raise GwbpError(f"{what} must be an integer tensor [{n}]")
    return group.to(dev).clamp(min=-1, max=INT32_MAX).to(torch.int32).contiguous()


as_group = _group  # what regions.py (components over a neighbour list) shares with this module


def _plan(p: torch.Tensor, radius: float, cell_size: Optional[float], grid: Optional[Grid]) -> Grid:
    """The grid of a walk: the caller's, or cells of max(radius, the automatic edge), so that a radius reaches one ring."""
    if grid is not None:
        return check_grid(grid)
    if cell_size is not None:
        return plan_grid(p, cell_size)
    auto = plan_grid(p)
    return auto if float(radius) <= auto.h else plan_grid(p, cell_size=float(radius))


def _build(p: torch.Tensor, grid: Grid):
    """(sorted points [N, 4], cell_start [cells + 1], perm [N]) of spatial.hip's build."""
    n, dev = p.shape[0], p.device
    skeys, perm = sorted_keys(p, grid)
    pts = torch.empty(n, 4, dtype=torch.float32, device=dev)
    cell_start = torch.empty(grid.cells + 1, dtype=torch.int32, device=dev)
    run("gwbp_spatial_build", dev, C.c_int64(n), ptr(p), C.c_int64(ld(p)), ptr(skeys), ptr(perm), C.c_int64(grid.cells), ptr(pts),
        ptr(cell_start))
    return pts, cell_start, perm


r2_of, plan_walk, build_grid = _r2, _plan, _build  # what sample.py (the Gaussians that weigh on a point, on the same grid) shares


def _walk_args(n: int, pts, cell_start, grid: Grid, group, r2: float):
    return (C.c_int64(n), ptr(pts), ptr(cell_start), *grid_args(grid), ptr(group), C.c_float(r2))


def _count(built, grid: Grid, group, r2: float, q, order, query_group, cap: int, visited=None) -> torch.Tensor:
    pts, cell_start, _ = built
    count = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
    run("gwbp_radius_count", q.device, *_walk_args(pts.shape[0], pts, cell_start, grid, group, r2), C.c_int64(q.shape[0]), ptr(q),
        C.c_int64(ld(q)), ptr(order), ptr(query_group), cap, ptr(count), ptr(visited))
    return count


def radius_count(points: torch.Tensor, radius: float, queries: Optional[torch.Tensor] = None, *, group: Optional[torch.Tensor] = None,
                 query_group: Optional[torch.Tensor] = None, cap: Optional[int] = None, cell_size: Optional[float] = None,
                 grid: Optional[Grid] = None) -> torch.Tensor:
    """int32 [Q]: for every query the number of points[N, 3] within radius of it (d2 <= r2, the module's contract) whose group is
    the query's, saturated at cap (None: the full count; the walk of a query ends once it has reached cap).  queries None: the points
    themselves with their own groups, so that the count includes the point itself.  group: integer [N], negative = excluded (None:
    all in group 0); query_group: integer [Q] for separate queries (None: all in group 0).  A non-finite or excluded query gets 0.
    points / queries are read in place at any row stride >= 3.  The result does not depend on cell_size / grid."""
    r2 = _r2(radius)
    cap = INT32_MAX if cap is None else int(cap)
    if not 1 <= cap <= INT32_MAX:
        raise GwbpError(f"cap must be in [1, 2^31 - 1], got {cap}")
    p = as_points(points, "points")
    n, dev = p.shape[0], p.device
    grp = _group(group, None, n, dev)
    if queries is None:
        if query_group is not None:
            raise GwbpError("query_group goes with separate queries; the points' own groups are group")
        q, qgrp = p, grp
    else:
        q = as_points(queries, "queries")
        if q.device != dev:
            raise GwbpError("points and queries must be on one device")
        qgrp = _group(query_group, None, q.shape[0], dev, "query_group")
    if n == 0 or q.shape[0] == 0:
        return torch.zeros(q.shape[0], dtype=torch.int32, device=dev)
    g = _plan(p, radius, cell_size, grid)
    built = _build(p, g)
    order = built[2] if queries is None else sorted_keys(q, g)[1]
    return _count(built, g, grp, r2, q, order, qgrp, cap)


def dense_labels(root: torch.Tensor):
    """(labels int32 [N], sizes int64 [C]) from root[N] (-1: noise): the distinct roots in ascending order are components 0 .. C-1,
    which is the order of their smallest core members, a root being its component's smallest member.  Plain torch."""
    live = root >= 0
    uniq = torch.unique(root[live])  # sorted
    labels = torch.full_like(root, -1, dtype=torch.int32)
    labels[live] = torch.searchsorted(uniq, root[live]).to(torch.int32)
    sizes = torch.bincount(labels[live].long(), minlength=int(uniq.numel()))
    return labels, sizes


def radius_components(points: torch.Tensor, radius: float, min_points: int = 1, *, group: Optional[torch.Tensor] = None,
                      mask: Optional[torch.Tensor] = None, cell_size: Optional[float] = None, grid: Optional[Grid] = None,
                      return_stats: bool = False) -> Components:
    """The components of points[N, 3] under the module's contract: Components(labels, sizes, core[, grid_stats]).  group: integer
    [N], points of different groups are never neighbours and a negative group excludes a point; mask: bool [N], the group where(mask,
    0, -1).  Default grid: plan_grid(points, cell_size=max(radius, the automatic edge)); the result does not depend on it.  Four
    launches on the built grid: the counts (saturated at min_points), the union-find over the core points, the border points'
    nearest core neighbour (min_points > 1 only), the roots; the dense numbering is torch.unique over the roots, the sizes a
    bincount.  Cells that hold thousands of points make the walk quadratic in their occupancy: see grid_stats."""
    r2 = _r2(radius)
    min_points = int(min_points)
    if not 1 <= min_points <= INT32_MAX:
        raise GwbpError(f"min_points must be in [1, 2^31 - 1], got {min_points}")
    p = as_points(points, "points")
    n, dev = p.shape[0], p.device
    grp = _group(group, mask, n, dev)
    if n == 0:
        empty = Components(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                           torch.zeros(0, dtype=torch.bool, device=dev))
        return empty._replace(grid_stats=grid_stats(Grid((0.0, 0.0, 0.0), 1.0, (1, 1, 1)), torch.zeros(2, dtype=torch.int32))) \
            if return_stats else empty
    g = _plan(p, radius, cell_size, grid)
    built = _build(p, g)
    pts, cell_start, perm = built
    count = _count(built, g, grp, r2, p, perm, grp, min_points)
    parent = torch.arange(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    walk = _walk_args(n, pts, cell_start, g, grp, r2)
    run("gwbp_radius_union", dev, *walk, ptr(count), min_points, ptr(parent), ptr(status))
    attach = None
    if min_points > 1:
        attach = torch.empty(n, dtype=torch.int32, device=dev)
        run("gwbp_radius_attach", dev, *walk, ptr(count), min_points, ptr(attach))
    root = torch.empty(n, dtype=torch.int32, device=dev)
    run("gwbp_components_flatten", dev, C.c_int64(n), ptr(count), min_points, ptr(attach), ptr(parent), ptr(root), ptr(status))
    if int(status):
        raise GwbpError("radius_components: a loop of the union-find reached its trip cap (internal error)")
    labels, sizes = dense_labels(root)
    return Components(labels, sizes, count >= min_points, grid_stats(g, cell_start) if return_stats else None)


def radius_from_distances(dist: torch.Tensor, factor: float = 2.0) -> float:
    """suggest_radius' arithmetic on dist[M, 1 + k] of a self-search: factor x the median (the lower one of an even number) of the
    finite distances in the last column.  0.0 without any."""
    d = dist[:, -1].double()
    d = d[torch.isfinite(d)]
    return float(factor) * float(d.median()) if d.numel() else 0.0


def suggest_radius(points: torch.Tensor, k: int = 8, factor: float = 2.0, mask: Optional[torch.Tensor] = None) -> float:
    """A radius from the points' own density: factor x the median distance to the k-th nearest neighbour (itself not counted, so
    the search asks for k + 1 <= 32), within mask if one is given.  Plain torch on spatial_knn's distances."""
    if not points.is_cuda:
        raise GwbpError("suggest_radius() needs HIP tensors (there is no CPU path)")
    if not 1 <= int(k) <= MAX_K - 1:
        raise GwbpError(f"k must be in [1, {MAX_K - 1}], got {k}")
    p = as_points(points, "points")
    if mask is not None:
        if mask.dim() != 1 or mask.shape[0] != p.shape[0]:
            raise GwbpError(f"mask must be [N = {p.shape[0]}], got {tuple(mask.shape)}")
        p = p[mask.to(p.device).bool()]
    m = p.shape[0]
    if m < 2:
        return 0.0
    return radius_from_distances(spatial_knn(p, min(int(k) + 1, m))[0], factor)


def select_components(result, *, seeds: Optional[Sequence[int]] = None, largest: Optional[int] = None,
                      min_size: Optional[int] = None) -> torch.Tensor:
    """bool [N]: the members of the union of the components that contain the seed indices (a seed that is noise selects nothing),
    the `largest` biggest components (ties to the smaller id) and all components with at least min_size members.  result: a
    Components or an Instances (anything with labels[N] and sizes[C]).  Plain torch, on the device of the result."""
    if seeds is None and largest is None and min_size is None:
        raise GwbpError("select_components: give seeds, largest or min_size")
    labels, sizes = result.labels, result.sizes
    n, c = labels.shape[0], sizes.shape[0]
    chosen = torch.zeros(c + 1, dtype=torch.bool, device=labels.device)  # (the last entry stands for noise and stays False)
    if seeds is not None:
        s = torch.as_tensor(seeds, dtype=torch.int64, device=labels.device).reshape(-1)
        if s.numel() and (int(s.min()) < 0 or int(s.max()) >= n):
            raise GwbpError(f"seeds must be indices in [0, {n})")
        hit = labels[s].long()
        chosen[hit[hit >= 0]] = True
    if largest is not None:
        if int(largest) < 0:
            raise GwbpError(f"largest must be >= 0, got {largest}")
        chosen[torch.sort(sizes, descending=True, stable=True).indices[:int(largest)]] = True
    if min_size is not None:
        chosen[:c] |= sizes >= int(min_size)
    return chosen[torch.where(labels >= 0, labels.long(), c)]


def rank_components(labels: torch.Tensor, sizes: torch.Tensor, min_size: int = 1):
    """(instances int32 [N], order int64 [I]): the components of at least min_size members renumbered by descending size, ties to the
    smaller component id; order[i] = the component that became instance i; every other point gets -1.  Plain torch."""
    order = torch.sort(sizes, descending=True, stable=True).indices
    order = order[sizes[order] >= int(min_size)]
    c = sizes.shape[0]
    new_id = torch.full((c + 1,), -1, dtype=torch.int32, device=labels.device)
    new_id[order] = torch.arange(order.numel(), dtype=torch.int32, device=labels.device)
    return new_id[torch.where(labels >= 0, labels.long(), c)], order


def split_instances(means: torch.Tensor, labels_or_mask: torch.Tensor, radius: Optional[float] = None, min_points: int = 1,
                    min_size: int = 1, num_classes: Optional[int] = None) -> Instances:
    """A 3-D mask (bool [N]) or a label field (integer [N]; labels outside [0, num_classes) are dropped, num_classes None: max + 1)
    split into spatially separate instances: the radius components of the means with the class as the group, so that two classes
    never merge, numbered by descending size (ties to the smaller component id); components below min_size members and noise get
    -1.  radius None: suggest_radius() within the live set.  Instances(instances, sizes, classes, core, radius, grid_stats)."""
    if not means.is_cuda:
        raise GwbpError("split_instances() needs HIP tensors (there is no CPU path)")
    p = as_points(means, "means")
    n, dev = p.shape[0], p.device
    lab = labels_or_mask
    if not torch.is_tensor(lab) or lab.dim() != 1 or lab.shape[0] != n or lab.dtype.is_floating_point:
        raise GwbpError(f"labels_or_mask must be a bool or integer tensor [N = {n}]")
    lab = lab.to(dev)
    if lab.dtype == torch.bool:
        group = torch.where(lab, 0, -1).to(torch.int32)
    else:
        nc = int(num_classes) if num_classes is not None else (int(lab.max()) + 1 if n else 0)
        group = torch.where((lab >= 0) & (lab < nc), lab, torch.full_like(lab, -1)).to(torch.int32)
    live = group >= 0
    if radius is None:
        radius = suggest_radius(p, mask=live)
    res = radius_components(p, radius, min_points, group=group, return_stats=True)
    instances, order = rank_components(res.labels, res.sizes, min_size)
    comp_class = torch.zeros(res.sizes.shape[0], dtype=torch.int64, device=dev)
    member = res.labels >= 0
    comp_class[res.labels[member].long()] = group[member].long()  # (a component's members share their group)
    return Instances(instances, res.sizes[order], comp_class[order], res.core, float(radius), res.grid_stats)


# ---- seeded inputs (the CLI's --synthetic) -----------------------------------------------------------------------------------------

def synthetic_instances(means: torch.Tensor, balls: int = 3, floaters: float = 0.005, seed: int = 3):
    """A mask that holds several objects and some floaters: around each of `balls` seeded sites among the means the n / (8 (b + 1))
    nearest Gaussians (ball b; a Gaussian near two sites goes to the first), plus a seeded fraction of all the others switched on.
    (mask[N] bool, ball[N] int64: the ball of a Gaussian, -1 outside every ball), on the device of the means."""
    g = torch.Generator().manual_seed(seed)
    n = means.shape[0]
    sites = means[torch.randperm(n, generator=g)[:balls].to(means.device)].float()
    ball = torch.full((n,), -1, dtype=torch.int64, device=means.device)
    for b in range(sites.shape[0]):
        d = (means.float() - sites[b]).norm(dim=1)
        near = d <= d.kthvalue(max(n // (8 * (b + 1)), 1)).values
        ball[near & (ball < 0)] = b
    noise = (torch.rand(n, generator=g) < floaters).to(means.device)
    return (ball >= 0) | noise, ball
