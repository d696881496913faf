"""Per-view instance masks associated into consistent 3-D groups, training-free, with a 3-D memory bank.

An "everything" segmenter (automatic masks, superpixels) runs on each view by itself: mask 7 of view 3 and mask 7 of view 4 have
nothing to do with each other, and no label lift of this package (create_label_field, create_vote_field,
create_mask_feature_field, render_label_maps / score_label_views, split_instances) can take such maps.  This module renames them:

    assoc = associate_masks(means, quats, scales, opacities, viewmats, K, W, H, mask_fn, max_masks)
    label_fn = associated_label_fn(assoc, mask_fn)                       # the views' maps with GLOBAL group ids
    P = create_label_field(means, quats, scales, opacities, viewmats, K, W, H, label_fn, assoc.n_groups)
    assoc.groups                                                          # or the group of every Gaussian directly

The views are taken in order and every Gaussian carries the group it currently belongs to.  For a new view gwbp_label_overlap
builds the table "mask m x existing group j" in the Gaussians' weight space straight from the weight store, the host matches
masks to groups one-to-one by IoU (match_masks) and opens groups for what is left, and gwbp_label_votes adds the view's evidence
to the per-Gaussian group votes.  Both kernels sum fixed-point integers (quantize_weights), so the tables -- and with them every
decision, each of which feeds the next view -- are exact and the same on every run.  There is no merging of groups behind the pass
and no second pass.  The defaults iou_min = 0.2 and min_mass = 1.0 come from one synthetic scene and are not tuned.

votes="sparse" keeps the evidence in per-Gaussian slot lists (sparse_votes.py, gwbp_label_votes_sparse) instead of the dense
[N, max_groups] table -- N * (12 * slots + 8) bytes whatever the number of groups -- and sizes the per-view overlap table by the
groups that exist; max_groups is then a bound on ids only.  create_sparse_label_field is create_label_field's P in that form.
"""
from __future__ import annotations

import warnings
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from ._lib import GwbpError
from .engine import Engine
from .sparse_votes import (SparseLabelField, SparseVotes, new_sparse_votes, sparse_label_field_of, sparse_votes_canonical,
                           sparse_votes_groups)

WEIGHT_SCALE = 2 ** 20  # fixed-point steps per unit of blend weight
WEIGHT_CLAMP = 4.0      # a stored weight saturates here (above 1 only with a pixel weight map)


def quantize_weights(w):
    """The fixed-point weight both kernels add for a stored blend weight w (the arithmetic contract of include/gwbp.h):
    q = rint(min(max(w, 0), WEIGHT_CLAMP) * WEIGHT_SCALE), round to nearest and half to even, NaN and negative values 0.
    w: a float32 torch tensor or numpy array; returns int64 of the same kind (every value fits uint32)."""
    if torch.is_tensor(w):
        x = torch.nan_to_num(w.to(torch.float32), nan=0.0).clamp(0.0, WEIGHT_CLAMP)
        return torch.round(x * float(WEIGHT_SCALE)).to(torch.int64)
    x = np.asarray(w, dtype=np.float32)
    x = np.fmin(np.fmax(x, np.float32(0.0)), np.float32(WEIGHT_CLAMP))  # fmax / fmin drop a NaN operand
    return np.rint(x * np.float32(WEIGHT_SCALE)).astype(np.int64)


def match_masks(O, n_groups: int, iou_min: float = 0.2, min_mass: float = 1.0, max_groups: int = 256, return_counts: bool = False):
    """One view's masks matched to the existing groups: (remap int32 [K_v], new n_groups), pure host code on the overlap table.

    O: int64 [K_v + 1, >= n_groups + 1] as gwbp_label_overlap fills it (row K_v: the ignored pixels; column 0: Gaussians without
    a group; column j + 1: group j).  With A[m] the sum of row m and B[j] the sum of column j + 1 over ALL rows:
      1. a mask is live if A[m] >= rint(min_mass * WEIGHT_SCALE); a dead mask maps to -1;
      2. live m, j < n_groups with o = O[m, j + 1] > 0 have iou = o / (A[m] + B[j] - o), one float64 division of exact integers;
      3. the candidates with iou >= iou_min are taken greedily by descending iou, then ascending m, then ascending j, each mask and
         each group at most once (one-to-one: many-to-one merges unrelated instances);
      4. unmatched live masks open the groups n_groups, n_groups + 1, ... in ascending m;
      5. once max_groups is reached they map to -1 and count as dropped.
    return_counts: also return {"matched", "opened", "dropped", "dead"}."""
    O = np.asarray(O.cpu() if torch.is_tensor(O) else O)
    if O.ndim != 2 or O.dtype != np.int64 or O.shape[0] < 2:
        raise ValueError(f"O must be an int64 [K + 1, n_cols] table, got {O.dtype} {O.shape}")
    n_groups, max_groups = int(n_groups), int(max_groups)
    if n_groups < 0 or n_groups + 1 > O.shape[1]:
        raise ValueError(f"O has {O.shape[1]} columns, too few for {n_groups} groups")
    K = O.shape[0] - 1
    A = O[:K].sum(axis=1)
    B = O[:, 1:n_groups + 1].sum(axis=0)
    live = A >= int(np.rint(float(min_mass) * WEIGHT_SCALE))
    cand = []
    for m in np.nonzero(live)[0]:
        row = O[m, 1:n_groups + 1]
        for j in np.nonzero(row > 0)[0]:
            o = int(row[j])
            iou = float(o) / float(int(A[m]) + int(B[j]) - o)
            if iou >= iou_min:
                cand.append((-iou, int(m), int(j)))
    cand.sort()
    remap = np.full(K, -1, np.int32)
    used = np.zeros(max(n_groups, 1), bool)
    matched = 0
    for _, m, j in cand:
        if remap[m] < 0 and not used[j]:
            remap[m], used[j] = j, True
            matched += 1
    opened = dropped = 0
    for m in np.nonzero(live & (remap < 0))[0]:
        if n_groups < max_groups:
            remap[m] = n_groups
            n_groups += 1
            opened += 1
        else:
            dropped += 1
    if return_counts:
        return remap, n_groups, dict(matched=matched, opened=opened, dropped=dropped, dead=int((~live).sum()))
    return remap, n_groups


class Association(NamedTuple):
    maps: List[torch.Tensor]   # per view (view-index order): int32 [max_masks] on the device, mask id -> group id or -1
    groups: torch.Tensor       # int32 [N]: every Gaussian's group, -1 without one
    votes: Union[torch.Tensor, SparseVotes]  # int64 [N, max_groups]: fixed-point evidence per group (votes / WEIGHT_SCALE is
    #                            blend weight); with votes="sparse" the slot lists, in canonical order
    n_groups: int
    views: List[Dict]          # per processed view, in processing order: view, matched, opened, dropped, dead, unassigned_share
    #                            (sparse: and overflow_rows, the rows with spill after the view)


def remap_masks(labels: torch.Tensor, remap) -> torch.Tensor:
    """A 2-D integer map renamed through remap (int32 [K]): int32, -1 where the id lies outside [0, K) or remap says -1."""
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.is_floating_point():
        raise GwbpError("labels must be a 2-D integer tensor")
    remap = torch.as_tensor(remap, dtype=torch.int32, device=labels.device)
    ids = labels.view(torch.uint8).to(torch.int64) if labels.dtype == torch.bool else labels.to(torch.int64)
    ok = (ids >= 0) & (ids < remap.numel())
    return torch.where(ok, remap[torch.where(ok, ids, 0)], -1).to(torch.int32)


def associated_label_fn(association: Association, mask_fn: Callable[[int], torch.Tensor]) -> Callable[[int], torch.Tensor]:
    """label_fn for create_label_field / create_vote_field with num_classes = association.n_groups: view v's map with global ids."""
    return lambda v: remap_masks(mask_fn(v), association.maps[v])


def group_of_votes(votes: torch.Tensor) -> torch.Tensor:
    """int32 [N]: the column of each row's maximum where it is positive (the smallest index among equals), else -1."""
    best, arg = votes.max(dim=1)  # (the first maximal index, as torch documents)
    return torch.where(best > 0, arg, -1).to(torch.int32)


def _blend_view(what: str, eng: Engine, v: int, view, gauss, weights, after=None):
    """The front of one view for the drivers of this module: project, sort, blend_weights (blend_weighted with `weights`), then
    after() -- what has to be enqueued before the one synchronisation that reads the overflow word; its result is returned.  The
    drivers' policy: overflow bits 0 / 1 are capacities (grow the workspace, run the view again, six attempts; nothing of the
    view has been added to an accumulator yet), anything else cannot be cured."""
    for attempt in range(6):
        eng.project(view, *gauss)
        eng.bin_sort(view)
        if weights is not None:
            eng.blend_weighted(view, weights())
        else:
            eng.blend_weights(view)
        out = after() if after is not None else None
        stats = eng.stats()
        if not stats["overflow"]:
            return out
        if stats["overflow"] & ~3 or attempt == 5:
            raise RuntimeError(f"{what}: view {v} ended with gwbp_stats.overflow = {stats['overflow']}"
                               + (" after five enlargements" if not stats["overflow"] & ~3 else ""))
        eng.grow(stats)


def associate_masks(means, quats, scales, opacities, viewmats, K, width: int, height: int,
                    mask_fn: Callable[[int], torch.Tensor], max_masks: int, max_groups: int = 256, iou_min: float = 0.2,
                    min_mass: float = 1.0, order: Optional[Sequence[int]] = None,
                    pixel_weight_fn: Optional[Callable[[int], torch.Tensor]] = None, upsample: Optional[str] = None,
                    engine: Optional[Engine] = None, votes: str = "dense", slots: int = 8, on_overflow: str = "warn",
                    **raster_kw) -> Association:
    """Associate the views' instance maps into 3-D groups (module docstring).  mask_fn(v) -> the view's integer [height, width]
    map on the device (with upsample="nearest": any [h, w]), ids in [0, max_masks); anything else is ignored, as in
    create_label_field.  Per view of `order` (default 0 .. V-1): project, sort, blend_weights (blend_weighted with
    pixel_weight_fn(v)), label_overlap, ONE copy of the [max_masks + 1, max_groups + 1] table to the host (a synchronisation per
    view: the algorithm is sequential by nature), match_masks, label_votes with the new remap, groups = argmax of the votes.
    A workspace overflow grows the workspace and runs that view again; nothing of an overflowed view has been added.
    raster_kw: near_plane, far_plane, eps2d, radius_clip, camera_model, rasterize_mode.
    Memory: the votes take 8 * N * max_groups bytes -- 2 GB at N = 1 M and 256 groups.

    votes="sparse": the evidence goes into `slots` (1 .. 32) slots per Gaussian (label_votes_sparse), N * (12 * slots + 8) bytes,
    and the per-view argmax comes from the lists; Association.votes is a SparseVotes in canonical order.  The overlap table is
    zeroed and copied with the columns 0 .. n_groups only (its buffer grows geometrically), so max_groups bounds ids and nothing
    else and may be 65536.  While no row spills, every decision equals the dense mode's, bit for bit and on every run.  A row that
    has received more than `slots` distinct groups spills (WHICH rows is a function of the input; which groups keep their slots
    is not): on_overflow="raise" raises at the first view that leaves such a row, "warn" warns once and goes on -- the groups
    that feed the next view are then no longer promised to be the same on every run.  Every entry of Association.views gains
    overflow_rows."""
    from ._views import raster_kw as _raster_kw, require_device
    require_device("associate_masks", means)
    kw = _raster_kw("associate_masks", raster_kw)
    if upsample not in (None, "nearest"):
        raise ValueError(f"upsample must be None or 'nearest' for mask maps, got {upsample!r}")
    n, dev = int(means.shape[0]), means.device
    n_masks, max_groups = int(max_masks), int(max_groups)
    if n_masks < 1 or max_groups < 1:
        raise ValueError("max_masks and max_groups must be positive")
    if votes not in ("dense", "sparse"):
        raise ValueError(f"votes must be 'dense' or 'sparse', got {votes!r}")
    if on_overflow not in ("warn", "raise"):
        raise ValueError(f"on_overflow must be 'warn' or 'raise', got {on_overflow!r}")
    sparse = votes == "sparse"
    width, height = int(width), int(height)
    n_views = int(viewmats.shape[0])
    order = list(range(n_views)) if order is None else [int(v) for v in order]
    vm_host, K_host = viewmats.detach().cpu(), K.detach().cpu()
    eng = engine or Engine(n, width, height, device=dev, tight_binning=True)
    gauss = (means, quats, scales, opacities)

    def weights_of(v):
        return None if pixel_weight_fn is None else (lambda: pixel_weight_fn(v))
    acc = new_sparse_votes(n, slots, device=dev) if sparse else torch.zeros(n, max_groups, dtype=torch.int64, device=dev)
    groups = torch.full((n,), -1, dtype=torch.int32, device=dev)
    # dense: one table as wide as max_groups.  sparse: as wide as the groups that exist (the buffer doubles when they outgrow it)
    O_store = torch.empty(n_masks + 1, min(max_groups, 15) + 1 if sparse else max_groups + 1, dtype=torch.int64, device=dev)
    warned = False
    maps = [torch.full((n_masks,), -1, dtype=torch.int32, device=dev) for _ in range(n_views)]
    n_groups, table = 0, []
    for v in order:
        labels = mask_fn(v)
        if sparse and n_groups + 1 > O_store.shape[1]:
            O_store = torch.empty(n_masks + 1, min(max_groups, max(2 * O_store.shape[1] - 2, n_groups)) + 1, dtype=torch.int64,
                                  device=dev)
        O = O_store[:, :n_groups + 1] if sparse else O_store  # (a row stride wider than n_cols: label_overlap takes it)
        view = eng.view(vm_host[v], K_host if K_host.dim() == 2 else K_host[v], width, height, **kw)

        def overlap(view=view, labels=labels, O=O, groups=groups):
            O.zero_()
            eng.label_overlap(view, labels, groups, O, n_masks, upsample=upsample)
            return O.cpu().numpy()

        O_host = _blend_view("associate_masks", eng, v, view, gauss, weights_of(v), overlap)
        remap, n_groups, counts = match_masks(O_host, n_groups, iou_min, min_mass, max_groups, return_counts=True)
        maps[v] = torch.from_numpy(remap).to(dev)
        total = int(O_host.sum())
        table.append(dict(view=v, **counts, unassigned_share=float(O_host[:, 0].sum()) / total if total else 0.0))
        if not sparse:
            eng.label_votes(view, labels, maps[v], acc, n_masks, upsample=upsample)
            groups = group_of_votes(acc)
            continue
        eng.label_votes_sparse(view, labels, maps[v], acc, n_masks, upsample=upsample)
        groups, _ = sparse_votes_groups(acc)
        table[-1]["overflow_rows"] = spilled = int((acc.spill > 0).sum())
        if spilled and on_overflow == "raise":
            raise GwbpError(f"associate_masks: after view {v}, {spilled} Gaussians have received more than {slots} distinct groups "
                            "(their votes spilled): raise slots")
        if spilled and not warned:
            warned = True
            warnings.warn(f"associate_masks: after view {v}, {spilled} Gaussians have received more than {slots} distinct groups; "
                          "which of them keep a slot depends on the order of the run, so the groups that feed the next views "
                          "are no longer promised to be the same on every run (raise slots, or on_overflow='raise')",
                          RuntimeWarning, stacklevel=2)
    return Association(maps, groups, sparse_votes_canonical(acc) if sparse else acc, n_groups, table)


def create_sparse_label_field(means, quats, scales, opacities, viewmats, K, width: int, height: int,
                              label_fn: Callable[[int], torch.Tensor], num_classes: int, slots: int = 8,
                              pixel_weight_fn: Optional[Callable[[int], torch.Tensor]] = None, upsample: Optional[str] = None,
                              engine: Optional[Engine] = None, **raster_kw) -> SparseLabelField:
    """create_label_field's P[g, k] = F[g, k] / d[g] restricted to each Gaussian's non-zero classes: SparseLabelField(ids int32
    [N, slots], fractions float32 [N, slots], spill_fraction float32 [N], total int64 [N]) in canonical order (largest share first,
    then the smaller id; -1 = empty), N * (12 * slots + 16) bytes of accumulator whatever num_classes.  Per view (in order, one
    stream): project, sort, blend_weights (blend_weighted with pixel_weight_fn(v)), label_votes_sparse with the identity remap and
    total; a workspace overflow grows the workspace and runs the view again before anything of it has been added.  The sums are
    the fixed-point integers of quantize_weights, so fractions = vals / total (one float64 division, then narrowed) differs from
    P by the quantisation (at most 2^-21 per stored entry) and P's own float error; total is d in the same fixed point.  A
    Gaussian that saw more than `slots` classes keeps `slots` of them (which ones depends on the run) and reports the rest as
    spill_fraction.  label_fn, upsample, raster_kw: as associate_masks' mask_fn, upsample, raster_kw."""
    from ._views import raster_kw as _raster_kw, require_device
    require_device("create_sparse_label_field", means)
    kw = _raster_kw("create_sparse_label_field", raster_kw)
    if upsample not in (None, "nearest"):
        raise ValueError(f"upsample must be None or 'nearest' for label maps, got {upsample!r}")
    n, dev, n_classes = int(means.shape[0]), means.device, int(num_classes)
    if n_classes < 1:
        raise ValueError("num_classes must be positive")
    width, height = int(width), int(height)
    vm_host, K_host = viewmats.detach().cpu(), K.detach().cpu()
    eng = engine or Engine(n, width, height, device=dev, tight_binning=True)
    gauss = (means, quats, scales, opacities)

    def weights_of(v):
        return None if pixel_weight_fn is None else (lambda: pixel_weight_fn(v))
    sv = new_sparse_votes(n, slots, device=dev, total=True)
    identity = torch.arange(n_classes, dtype=torch.int32, device=dev)
    for v in range(int(viewmats.shape[0])):
        labels = label_fn(v)
        view = eng.view(vm_host[v], K_host if K_host.dim() == 2 else K_host[v], width, height, **kw)
        _blend_view("create_sparse_label_field", eng, v, view, gauss, weights_of(v))
        eng.label_votes_sparse(view, labels, identity, sv, n_classes, upsample=upsample)
    return sparse_label_field_of(sv)
