"""Which Gaussians form one object by geometry AND features: region growing on the cosine of a feature field over the spatial k-NN
graph (csrc/regions.hip).  radius_components joins whatever touches (a cup with its table), fit_kmeans whatever looks alike (two
chairs across the room); here two Gaussians are joined when one lists the other among its k nearest neighbours and their features'
cosine reaches a threshold, and the regions are the connected components of that graph.  (The reference has nothing of the kind; its
users would run a host-side graph library on a copy of the [N, D] field.)

    res = similarity_components(means, field, k=8, sim_min=0.9)                 # Components(labels[N], sizes[C], core[N])
    levels = similarity_levels(means, field, [0.8, 0.9, 0.95], neighbors=(dist, idx))   # int32 [3, N], each refining the last
    sim, live = neighbor_similarity(field, idx)                                 # the cosine of every listed pair
    edges = edge_strength(sim)                                                  # a per-Gaussian boundary score, [N]
    mask = region_prompt_mask(field, res.labels, prompts, n_pos)                # a prompt mask that is constant per region

THE CONTRACT (include/gwbp.h and csrc/regions.hip have the same words).  features [N, D] fp32 at any row stride >= D; idx [N, k]
int32, an entry < 0 or >= N is no neighbour, an entry == i is allowed and ignored by the union; dist [N, k] optional (spatial_knn's
distances); group [N] optional.  dot(i, j) and sq(i) = dot(i, i) are each one fixed arrangement of fp32 operations that depends on D
alone: lane l of 64 owns the channels 256 s + 4 l + e (s = 0, 1, ...; e = 0 .. 3; those < D), runs acc = fmaf(a, b, acc) from +0 in
the order (s, e), and the 64 partial sums are combined by the butterfly p_l = p_l + p_(l xor o), o = 1, 2, 4, 8, 16, 32.  It is
symmetric (dot(i, j) has the bits of dot(j, i)) and independent of N, k, the row's position, the stride, the alignment and the
launch.  norm(i) = sqrtf(sq(i)); row i is feature-live when sq(i) is finite and norm(i) >= 1e-12f (F.normalize's epsilon: a
never-seen Gaussian's zero row is dead, as in cluster.py).  sim[i, c] = dot(i, j) / (norm(i) * norm(j)) for j = idx[i, c], one
multiply and one correctly rounded divide; NaN when j is no neighbour or either row is not feature-live.  live(i) = feature-live and
group[i] >= 0 (no group: 0).  i -- j is an edge when j = idx[i, c] for some c or i = idx[j, c], i != j, both live, group[i] ==
group[j], sim[i, c] >= sim_min (NaN fails) and, with a cut, dist[i, c] <= max_dist = float32(radius).  The labels are the connected
components of the live points under the edges (a live point without an edge is a component of one), numbered by their smallest
member (components.dense_labels); everything else gets -1.  They are a pure function of (features, idx, dist, group, sim_min,
max_dist), whatever the order in which lanes run: two runs give the same bits.  Everything runs on the caller's current stream;
there is no PyTorch fallback: CPU tensors raise GwbpError.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import torch

from ._lib import GwbpError, ptr
from ._views import FIELD_TYPES, field_rows, ld, rows, run  # noqa: F401
from .cluster import class_prototypes, codebook_prompt_mask
from .components import Components, as_group, dense_labels
from .spatial import MAX_K as SPATIAL_MAX_K, as_points, spatial_knn

MAX_K = 64      # GWBP_REGIONS_MAX_K: columns of a neighbour list
MAX_D = 2048    # GWBP_REGIONS_MAX_D
DEFAULT_SIM_MIN = 0.9   # a guess, not a tuned value: nothing is claimed about real LSeg or DINO fields


def _field(features: torch.Tensor) -> torch.Tensor:
    f = field_rows(features, "features")[0]  # float16 / bfloat16 rows are read as stored (gwbp_neighbor_similarity_typed)
    if f.shape[1] > MAX_D:
        raise GwbpError(f"features: D = {f.shape[1]} exceeds {MAX_D}")
    if f.shape[0] >= 2 ** 31:
        raise GwbpError(f"features: {f.shape[0]} rows; indices are int32")
    return f


def _list(idx, n: int, dev, name: str = "idx") -> torch.Tensor:
    if not torch.is_tensor(idx) or not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 2 or idx.device != dev \
            or idx.shape[0] != n:
        raise GwbpError(f"{name} must be an int32 [N = {n}, k] tensor on the device of the features")
    if not 1 <= idx.shape[1] <= MAX_K:
        raise GwbpError(f"{name} must have 1 .. {MAX_K} columns, got {idx.shape[1]}")
    return idx.contiguous()


def _similarity(f: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sim float32 [N, k], live int32 [N]) of gwbp_neighbor_similarity; N >= 1."""
    n, k = idx.shape
    sim = torch.empty(n, k, dtype=torch.float32, device=f.device)
    live = torch.empty(n, dtype=torch.int32, device=f.device)
    run("gwbp_neighbor_similarity_typed", f.device, C.c_int64(n), f.shape[1], k, ptr(idx), ptr(f), FIELD_TYPES[f.dtype], C.c_int64(ld(f)),
        ptr(sim), ptr(live))
    return sim, live


def neighbor_similarity(features: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sim float32 [N, k], live bool [N]): the cosine of features[i] and features[idx[i, c]] under the module's contract, NaN where
    idx[i, c] is no neighbour or either row is not feature-live, and which rows are feature-live.  features [N, D <= 2048] is read in
    place at any row stride >= D; idx: int32 [N, k <= 64] on the same device (spatial_knn's, or any list).  No atomics."""
    f = _field(features)
    idx = _list(idx, f.shape[0], f.device)
    if f.shape[0] == 0:
        return torch.empty(0, idx.shape[1], dtype=torch.float32, device=f.device), torch.zeros(0, dtype=torch.bool, device=f.device)
    sim, live = _similarity(f, idx)
    return sim, live != 0


def _sim_min(sim_min: float) -> float:
    sim_min = float(sim_min)
    if math.isnan(sim_min):
        raise GwbpError("sim_min must not be NaN")
    return sim_min


def _max_dist(radius: Optional[float]) -> float:
    if radius is None:
        return math.inf
    radius = float(radius)
    if not (math.isfinite(radius) and radius >= 0.0):
        raise GwbpError(f"radius must be finite and >= 0, got {radius}")
    return float(torch.tensor(radius, dtype=torch.float32))


def _roots(idx, sim, live, dist, group, sim_min: float, max_dist: float):
    """(root int32 [N], count int32 [N]): one union launch and one flatten launch; N >= 1."""
    n, k = idx.shape
    dev = idx.device
    parent = torch.arange(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    root = torch.empty(n, dtype=torch.int32, device=dev)
    run("gwbp_edge_union", dev, C.c_int64(n), k, ptr(idx), ptr(sim), ptr(live), ptr(dist if max_dist < math.inf else None), ptr(group),
        C.c_float(sim_min), C.c_float(max_dist), ptr(count), ptr(parent), ptr(status))
    run("gwbp_components_flatten", dev, C.c_int64(n), ptr(count), 1, None, ptr(parent), ptr(root), ptr(status))
    if int(status):
        raise GwbpError("similarity_components: a loop of the union-find reached its trip cap (internal error)")
    return root, count


def _labels(root: torch.Tensor, min_size: int):
    labels, sizes = dense_labels(root)
    if min_size > 1 and sizes.numel():
        small = (sizes < min_size)[labels.clamp(min=0).long()] & (labels >= 0)
        labels, sizes = dense_labels(torch.where(small, torch.full_like(root, -1), root))
    return labels, sizes


def _setup(fn: str, means, features, k: int, radius, mask, group, neighbors, min_size):
    if not torch.is_tensor(means) or not means.is_cuda:
        raise GwbpError(f"{fn}() needs HIP tensors (there is no CPU path)")
    p = as_points(means, "means")
    n, dev = p.shape[0], p.device
    f = _field(features)
    if f.shape[0] != n or f.device != dev:
        raise GwbpError(f"features must be [N = {n}, D] on the device of the means, got {tuple(f.shape)}")
    min_size = int(min_size)
    if min_size < 1:
        raise GwbpError(f"min_size must be at least 1, got {min_size}")
    max_dist = _max_dist(radius)
    grp = as_group(group, mask, n, dev)
    if neighbors is None:
        k = int(k)
        if not 1 <= k <= SPATIAL_MAX_K - 1:
            raise GwbpError(f"k must be in [1, {SPATIAL_MAX_K - 1}], got {k} (the search asks for k + 1: itself is one of them)")
        dist, idx = spatial_knn(p, min(k + 1, n)) if n else (None, torch.empty(0, 1, dtype=torch.int32, device=dev))
    else:
        if not isinstance(neighbors, (tuple, list)) or len(neighbors) != 2:
            raise GwbpError("neighbors must be spatial_knn's (dist, idx) for these means")
        dist, idx = neighbors
    idx = _list(idx, n, dev, "neighbors' idx")
    if dist is not None:
        if not torch.is_tensor(dist) or dist.dtype != torch.float32 or dist.shape != idx.shape or dist.device != dev:
            raise GwbpError("neighbors' dist must be a float32 tensor of idx's shape on its device (or None)")
        dist = dist.contiguous()
    elif max_dist < math.inf and n:
        raise GwbpError("a radius needs the neighbours' distances: neighbors=(dist, idx)")
    return n, dev, f, idx, dist, grp, max_dist, min_size


def _pass(f: torch.Tensor, idx: torch.Tensor, similarity):
    """(sim, live int32) of the [N, D] pass, or the caller's (sim, live) of an earlier neighbor_similarity(features, idx)."""
    if similarity is None:
        return _similarity(f, idx)
    if not isinstance(similarity, (tuple, list)) or len(similarity) != 2:
        raise GwbpError("similarity must be neighbor_similarity's (sim, live) for these features and neighbors")
    sim, live = similarity
    if not torch.is_tensor(sim) or sim.dtype != torch.float32 or sim.shape != idx.shape or sim.device != idx.device:
        raise GwbpError("similarity's sim must be a float32 tensor of idx's shape on its device")
    if not torch.is_tensor(live) or live.shape != idx.shape[:1] or live.device != idx.device or live.is_floating_point():
        raise GwbpError(f"similarity's live must be a bool [N = {idx.shape[0]}] tensor on idx's device")
    return sim.contiguous(), (live != 0).to(torch.int32)


def similarity_quantiles(sim: torch.Tensor, qs: Sequence[float]):
    """The quantiles qs (each in [0, 1]) of the valid (not NaN) entries of sim, as floats, with torch.quantile's linear interpolation;
    [] without a valid entry.  From a sorted float64 copy, on sim's device: torch.quantile itself refuses more than 2^24 values, and a
    scene of a few million Gaussians has several times that many listed pairs.  Plain torch."""
    v = sim[~torch.isnan(sim)].double().sort().values
    m = int(v.numel())
    if m == 0:
        return []
    out = []
    for q in qs:
        pos = float(q) * (m - 1)
        lo = min(max(int(math.floor(pos)), 0), m - 1)
        hi = min(lo + 1, m - 1)
        a, b = float(v[lo]), float(v[hi])
        out.append(a + (b - a) * (pos - lo))
    return out


def similarity_components(means: torch.Tensor, features: torch.Tensor, k: int = 8, sim_min: float = DEFAULT_SIM_MIN,
                          radius: Optional[float] = None, *, mask: Optional[torch.Tensor] = None,
                          group: Optional[torch.Tensor] = None, neighbors=None, similarity=None, min_size: int = 1, return_similarity: bool = False):
    """The regions of the module's contract: Components(labels int32 [N], sizes int64 [C], core bool [N]); core is the live mask
    (feature-live and in a group).  The neighbour list is spatial_knn(means, k + 1) -- the self entry leaves k real neighbours, k <=
    31 -- or neighbors=(dist, idx) of an earlier search (any int32 [N, k' <= 64] list; dist may be None without a radius).  radius:
    also cut the edges longer than max_dist = float32(radius).  mask: bool [N], only these Gaussians take part; group: integer [N],
    Gaussians of different groups are never joined and a negative group excludes one.  min_size > 1: components with fewer members
    become -1 and the rest keep their order (components.dense_labels).  return_similarity: (Components, sim [N, k'], (dist, idx)).
    similarity: (sim, live) of an earlier neighbor_similarity(features, idx) for the same neighbors, which skips the [N, D] pass.
    Three launches: the similarities, the union over the edges that pass, the roots.  sim_min = 0.9 is a guess, not a tuned value."""
    sim_min = _sim_min(sim_min)
    n, dev, f, idx, dist, grp, max_dist, min_size = _setup("similarity_components", means, features, k, radius, mask, group,
                                                            neighbors, min_size)
    if n == 0:
        res = Components(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                         torch.zeros(0, dtype=torch.bool, device=dev))
        return (res, torch.empty(0, idx.shape[1], dtype=torch.float32, device=dev), (dist, idx)) if return_similarity else res
    sim, live = _pass(f, idx, similarity)
    root, count = _roots(idx, sim, live, dist, grp, sim_min, max_dist)
    labels, sizes = _labels(root, min_size)
    res = Components(labels, sizes, count != 0)
    return (res, sim, (dist, idx)) if return_similarity else res


def similarity_levels(means: torch.Tensor, features: torch.Tensor, thresholds: Sequence[float], k: int = 8,
                      radius: Optional[float] = None, *, mask: Optional[torch.Tensor] = None, group: Optional[torch.Tensor] = None,
                      neighbors=None, similarity=None, min_size: int = 1) -> torch.Tensor:
    """labels int32 [L, N]: similarity_components at every threshold of `thresholds`, from ONE similarity pass: a level costs only
    the integer union and the flatten.  The edges of a higher threshold are a subset of those of a lower one, so for ascending
    thresholds each partition refines the one before (with min_size = 1: every region of level l + 1 lies inside one region of
    level l; min_size > 1 drops small regions per level).  Row l equals similarity_components(..., sim_min=thresholds[l]).labels.
    similarity: (sim, live) of an earlier neighbor_similarity(features, idx) for the same neighbors: then no [N, D] pass at all."""
    ts = [_sim_min(t) for t in thresholds]
    n, dev, f, idx, dist, grp, max_dist, min_size = _setup("similarity_levels", means, features, k, radius, mask, group, neighbors,
                                                            min_size)
    out = torch.full((len(ts), n), -1, dtype=torch.int32, device=dev)
    if n == 0 or not ts:
        return out
    sim, live = _pass(f, idx, similarity)
    for level, t in enumerate(ts):
        out[level] = _labels(_roots(idx, sim, live, dist, grp, t, max_dist)[0], min_size)[0]
    return out


def edge_strength(sim: torch.Tensor, reduce: str = "min") -> torch.Tensor:
    """A per-Gaussian boundary score, float32 [N]: 1 - the NaN-skipping min (the weakest link) or mean of a row of sim [N, k]; a row
    with no valid neighbour gives 0.  Plain torch; it renders as a colour through rasterization()."""
    if reduce not in ("min", "mean"):
        raise GwbpError(f"reduce must be 'min' or 'mean', got {reduce!r}")
    if not torch.is_tensor(sim) or sim.dim() != 2:
        raise GwbpError("sim must be a [N, k] tensor")
    valid = ~torch.isnan(sim)
    if reduce == "min":
        v = torch.where(valid, sim, torch.full_like(sim, math.inf)).min(dim=1).values if sim.shape[1] else sim.new_zeros(sim.shape[0])
    else:
        v = torch.where(valid, sim, torch.zeros_like(sim)).sum(dim=1) / valid.sum(dim=1).clamp(min=1)
    return torch.where(valid.any(dim=1), 1.0 - v, torch.zeros_like(v)).float()


def region_prompt_mask(features: torch.Tensor, labels: torch.Tensor, prompts: torch.Tensor, n_pos: int,
                       threshold: Optional[float] = None) -> torch.Tensor:
    """bool [N]: prompt_mask asked of the regions instead of the Gaussians -- class_prototypes(features, labels, C) (each region's
    unit mean feature) followed by codebook_prompt_mask, so the mask is constant per region; label -1 scores as a zero row does.
    Composition only: no kernel of its own."""
    if not torch.is_tensor(labels) or labels.dim() != 1 or labels.is_floating_point():
        raise GwbpError("labels must be an integer [N] tensor")
    c = int(labels.max()) + 1 if labels.numel() else 0
    if c < 1:
        raise GwbpError("region_prompt_mask: no region (every label is -1)")
    protos, _ = class_prototypes(features, labels, c)
    return codebook_prompt_mask(protos, labels, prompts, n_pos, threshold)


# ---- seeded inputs (the CLI's --synthetic, the tests, tools/time_regions.py) -------------------------------------------------------

def synthetic_regions(means: torch.Tensor, d: int = 64, noise: float = 0.1, dead: float = 0.02, seed: int = 5):
    """A seeded field with planted regions over the means: four generating sets -- the two half-spaces either side of the median x
    (sets 0 and 1: they TOUCH and carry different prototypes) and, laid over them, two balls of N / 16 Gaussians each around the two
    seeded sites that lie farthest apart (sets 2 and 3: SEPARATED, and they share one prototype).  Row g = unit-normalised
    (prototype[set[g]] + noise * randn / sqrt(d)); the three prototypes are orthonormal, so rows of one prototype have a cosine near
    1 / (1 + noise^2) and rows of two prototypes a cosine near 0.  A seeded fraction `dead` of the rows is zero.
    (features [N, d] float32, sets [N] int64 with -1 for a zero row, prototype_of_set [4] int64), on the device of the means."""
    g = torch.Generator().manual_seed(seed)
    n = means.shape[0]
    m = means.detach().float().cpu()
    sets = (m[:, 0] >= m[:, 0].median()).long() if n else torch.zeros(0, dtype=torch.int64)
    if n >= 2:
        cand = m[torch.randperm(n, generator=g)[:8]]
        far = int(torch.cdist(cand, cand).argmax())
        per = max(n // 16, 1)
        for b, site in enumerate((cand[far // cand.shape[0]], cand[far % cand.shape[0]])):
            dist = (m - site).norm(dim=1)
            sets[(dist <= dist.kthvalue(per).values) & (sets < 2)] = 2 + b
    proto_of_set = torch.tensor([0, 1, 2, 2])
    protos = torch.linalg.qr(torch.randn(d, 3, generator=g, dtype=torch.float64)).Q.T.float() if d >= 3 else \
        torch.nn.functional.normalize(torch.randn(3, d, generator=g), dim=1)
    x = protos[proto_of_set[sets]] + float(noise) * torch.randn(n, d, generator=g) / math.sqrt(d)
    x = torch.nn.functional.normalize(x, dim=1)
    zero = torch.rand(n, generator=g) < float(dead)
    x[zero] = 0.0
    sets = torch.where(zero, torch.full_like(sets, -1), sets)
    return x.to(means.device), sets.to(means.device), proto_of_set.to(means.device)
