"""Cluster a finished feature field: k-means on the fp32 matrix cores, class prototypes, and the field as a codebook.

    labels, score = kmeans_assign(features, centroids)              # nearest centroid of every row (cosine or euclidean)
    sums, wsum, counts = cluster_sums(features, labels, k)           # per-class float64 column sums: the k-means update
    prototypes, counts = class_prototypes(features, labels, k)       # the inverse of transfer_labels: mean feature per class
    km = fit_kmeans(features, 64)                                     # KMeans(centroids, labels, counts, inertia, history, ...)
    codebook, codes = quantize_field(features, 256)                  # [k, D] + one int32 per Gaussian instead of [N, D]
    scores = codebook_prompt_scores(codebook, codes, prompts)        # == prompt_scores(dequantize_field(codebook, codes), prompts)

The two [N, D] passes run gwbp_kmeans_assign / gwbp_cluster_sums (csrc/cluster.hip) on the caller's current stream: the assignment
is knn_search's exact fp32 score with an optional per-centroid bias and no top-k list, the sums are float64, atomic-free and
bit-reproducible.  Everything between them -- the stable sort that groups the rows, the [k, D] centroid update in float64, the
seeding -- is torch.  Every random number comes from a CPU torch.Generator(seed): same inputs and seed give the same bits.  There
is no PyTorch fallback for the kernels: CPU tensors raise GwbpError.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, List, NamedTuple, Optional, Tuple, Union

import torch

from ._lib import GwbpError, check, lib, ptr
from ._views import FIELD_TYPES, field_rows, ld, rows, run  # noqa: F401  (rows: geometry and small operands; callers of _assign)
from .transfer import narrow_source_labels

MAX_K = 1 << 20          # GWBP_CLUSTER_MAX_K
RUN = 256                # GWBP_CLUSTER_RUN: members per run of the sums (part of their arithmetic contract)
METRICS = ("cosine", "euclidean")
PP_CANDIDATES = 64       # "kmeans++" looks at a seeded sample of at most this many non-zero rows per cluster


class KMeans(NamedTuple):
    """centroids [k, D] float32; labels [N] int32 (-1: a zero or NaN row); counts [k] int64; inertia: the last entry of history;
    history: the inertia of every assignment; n_iter = len(history); converged: the labels stopped changing or the inertia's
    relative drop fell to tol before `iters` ran out; reseeds: empty clusters that were given a row over the whole fit."""
    centroids: torch.Tensor
    labels: torch.Tensor
    counts: torch.Tensor
    inertia: float
    history: List[float]
    n_iter: int
    converged: bool
    reseeds: int


def _metric(metric: str) -> str:
    if metric not in METRICS:
        raise GwbpError(f"metric must be one of {METRICS}, got {metric!r}")
    return metric


def centroid_bias(centroids: torch.Tensor, metric: str) -> Optional[torch.Tensor]:
    """The per-centroid bias of the assignment: None for cosine; -|c|^2 / 2 in float64, rounded to float32 once, for euclidean
    (argmax_j <x, c_j> - |c_j|^2 / 2 is the Euclidean nearest centroid)."""
    if _metric(metric) == "cosine":
        return None
    return (-0.5 * (centroids.double() ** 2).sum(dim=1)).float()


def _centroids(centroids, d: int, device) -> torch.Tensor:
    if not torch.is_tensor(centroids) or centroids.dim() != 2 or centroids.shape[1] != d:
        raise GwbpError(f"centroids must be a [K, D = {d}] tensor")
    if not 1 <= centroids.shape[0] <= MAX_K:
        raise GwbpError(f"the number of centroids must be in [1, {MAX_K}], got {centroids.shape[0]}")
    return centroids.to(device=device, dtype=torch.float32).contiguous()


def _assign(x: torch.Tensor, c: torch.Tensor, bias: Optional[torch.Tensor]):
    """x: checked field rows in their own dtype (field_rows); c, bias: float32."""
    n, d = x.shape
    labels = torch.empty(n, dtype=torch.int32, device=x.device)
    best = torch.empty(n, dtype=torch.float32, device=x.device)
    run("gwbp_kmeans_assign_typed", x.device, C.c_int64(n), int(c.shape[0]), d, ptr(x), FIELD_TYPES[x.dtype], C.c_int64(ld(x)), ptr(c),
        C.c_int64(ld(c)), ptr(bias), ptr(labels), ptr(best))
    return labels, best


def _norms(x: torch.Tensor) -> torch.Tensor:
    return torch.linalg.vector_norm(x, dim=1, dtype=torch.float32)  # one pass over the field (half: widened in the reduction), no [N, D] temporary


def kmeans_assign(features: torch.Tensor, centroids: torch.Tensor, metric: str = "cosine"):
    """The nearest centroid of every row: (labels [N] int32, score [N] float32).  cosine: score = <x, c> (the largest inner
    product; give unit centroids), euclidean: score = <x, c> - |c|^2 / 2 (the smallest distance; |x - c|^2 = |x|^2 - 2 score).
    Exact fp32, knn_search's arithmetic; ties go to the lowest index; a row of zero norm and a row with a NaN get label -1.
    features: as knn_search (any row stride >= D, read in place; float16 / bfloat16 as stored, widened exactly in the kernel: the
    bits of the result on features.float(), without that copy)."""
    x, _ = field_rows(features, "features")
    c = _centroids(centroids, x.shape[1], x.device)
    labels, best = _assign(x, c, centroid_bias(c, metric))
    labels[_norms(x) == 0] = -1
    return labels, best


def _weights(weights, n: int, device) -> Optional[torch.Tensor]:
    if weights is None:
        return None
    if not torch.is_tensor(weights) or weights.dim() != 1 or weights.shape[0] != n:
        raise GwbpError(f"weights must be a [N = {n}] tensor")
    return weights.to(device=device, dtype=torch.float32).contiguous()


def _sums(x: torch.Tensor, lab: torch.Tensor, k: int, w: Optional[torch.Tensor]):
    """lab: int32 [N] on x's device, values outside [0, k) take no part."""
    n, d = x.shape
    dev = x.device
    skeys, order = torch.sort(lab, stable=True)
    start = torch.searchsorted(skeys, torch.arange(k + 1, dtype=torch.int32, device=dev))
    nbytes = C.c_size_t(0)
    check(lib().gwbp_cluster_workspace_size(C.c_int64(n), d, k, C.byref(nbytes)), "gwbp_cluster_workspace_size")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    sums = torch.empty(k, d, dtype=torch.float64, device=dev)
    wsum = torch.empty(k, dtype=torch.float64, device=dev)
    run("gwbp_cluster_sums_typed", dev, C.c_int64(n), d, k, ptr(x), FIELD_TYPES[x.dtype], C.c_int64(ld(x)), ptr(w), ptr(order), ptr(start),
        ptr(sums), ptr(wsum), ptr(ws), C.c_size_t(nbytes.value))
    return sums, wsum, start[1:] - start[:-1]


def cluster_sums(features: torch.Tensor, labels: torch.Tensor, num_classes: int, weights: Optional[torch.Tensor] = None):
    """(sums [K, D] float64, wsum [K] float64, counts [K] int64): sums[k] = the sum of weights[g] * features[g] over the rows with
    labels[g] == k, wsum[k] the sum of their weights (weights None: 1), counts[k] their number.  Labels outside [0, K) take no
    part.  Every term is formed in float64 (exact); a class's members are cut into runs of 256 in row order, each run is summed in
    ascending row order, the runs are added in ascending order: no atomics, the same bits on every run.  float16 / bfloat16 features
    are read as stored (widening is exact: the sums are those of features.float())."""
    x, _ = field_rows(features, "features")
    k = int(num_classes)
    if not 1 <= k <= MAX_K:
        raise GwbpError(f"num_classes must be in [1, {MAX_K}], got {k}")
    lab, _ = narrow_source_labels(labels, k)
    if lab.shape[0] != x.shape[0]:
        raise GwbpError(f"{lab.shape[0]} labels for {x.shape[0]} rows")
    return _sums(x, lab.to(x.device), k, _weights(weights, x.shape[0], x.device))


def class_prototypes(features: torch.Tensor, labels: torch.Tensor, num_classes: int, weights: Optional[torch.Tensor] = None,
                     normalize: bool = True):
    """The inverse of transfer_labels: (prototypes [K, D] float32, counts [K] int64), the (weighted) mean feature of each class,
    scaled to unit length with normalize -- the prompts or sources for the next scene.  Means and norms in float64, rounded to
    float32 once.  A class with no member (or of zero total weight, or whose mean is zero) gets a zero row."""
    sums, wsum, counts = cluster_sums(features, labels, num_classes, weights)
    return _means(sums, wsum, normalize).float(), counts


def _means(sums: torch.Tensor, wsum: torch.Tensor, normalize: bool) -> torch.Tensor:
    mean = sums / wsum.clamp(min=1e-300).unsqueeze(1)
    if normalize:
        norm = torch.linalg.vector_norm(mean, dim=1, keepdim=True)
        mean = torch.where(norm > 0, mean / norm.clamp(min=1e-300), torch.zeros_like(mean))
    return torch.where((wsum > 0).unsqueeze(1), mean, torch.zeros_like(mean))


# ---- the Lloyd loop, over two callables -------------------------------------------------------------------------------------------

def update_centroids(sums: torch.Tensor, wsum: torch.Tensor, previous: torch.Tensor, metric: str) -> torch.Tensor:
    """cosine: sums_k / |sums_k|; euclidean: sums_k / wsum_k; in float64, rounded to float32 once.  A cluster whose sum has no
    direction (no member, zero weight) keeps its previous centroid."""
    if metric == "cosine":
        norm = torch.linalg.vector_norm(sums, dim=1, keepdim=True)
        ok = (norm > 0) & (wsum > 0).unsqueeze(1)
        new = sums / torch.where(ok, norm, torch.ones_like(norm))
    else:
        ok = (wsum > 0).unsqueeze(1)
        new = sums / torch.where(ok, wsum.unsqueeze(1), torch.ones_like(wsum.unsqueeze(1)))
    return torch.where(ok, new.float(), previous)


def reseed_empty(x: torch.Tensor, labels: torch.Tensor, best: torch.Tensor, centroids: torch.Tensor, metric: str):
    """The empty-cluster rule.  After an assignment the e clusters without a member take, in ascending cluster order, the e assigned
    rows of lowest `best` (the rows their centroids serve worst), ties by row index: each such row becomes its cluster's centroid
    (scaled to unit length for cosine) and its only member, and the step continues with these labels.  Returns (labels, centroids,
    e); the inputs are not modified.  With fewer assigned rows than empty clusters the last ones stay empty."""
    k = centroids.shape[0]
    assigned = labels >= 0
    counts = torch.bincount(labels[assigned].long(), minlength=k)
    empty = torch.nonzero(counts == 0).squeeze(1)
    e = int(empty.numel())  # (the step's host synchronisation)
    if e == 0:
        return labels, centroids, 0
    cand = torch.nonzero(assigned).squeeze(1)
    worst = cand[torch.sort(best[cand], stable=True)[1][:e]]  # ascending best, then ascending row index
    empty = empty[:worst.numel()]
    labels, centroids = labels.clone(), centroids.clone()
    labels[worst] = empty.to(labels.dtype)
    seed = x[worst].double()
    if metric == "cosine":
        seed = seed / torch.linalg.vector_norm(seed, dim=1, keepdim=True)
    centroids[empty] = seed.float()
    return labels, centroids, int(worst.numel())


def inertia_of(labels: torch.Tensor, best: torch.Tensor, metric: str, sqnorm: torch.Tensor, w: Optional[torch.Tensor]) -> float:
    """cosine: sum w (1 - best); euclidean: sum w (|x|^2 - 2 best); over the assigned rows, in float64."""
    b = best.double()
    term = (1.0 - b) if metric == "cosine" else (sqnorm - 2.0 * b)
    if w is not None:
        term = term * w.double()
    return float(torch.where(labels >= 0, term, torch.zeros_like(term)).sum())


def lloyd_step(x: torch.Tensor, centroids: torch.Tensor, assign: Callable, sums: Callable, metric: str):
    """One Lloyd step from `centroids`: assign -> empty-cluster rule -> (stable sort ->) sums -> centroids.  assign(centroids) ->
    (labels int32 [N] with -1 for the rows that take no part, best float32 [N]); sums(labels) -> (sums float64 [k, D], wsum float64
    [k], counts int64 [k]).  Returns (labels, best, new_centroids, counts, reseeded): labels after the empty-cluster rule, best as
    assigned."""
    labels, best = assign(centroids)
    labels, seeded, e = reseed_empty(x, labels, best, centroids, metric)
    s, wsum, counts = sums(labels)
    return labels, best, update_centroids(s, wsum, seeded, metric), counts, e


def lloyd(x: torch.Tensor, centroids: torch.Tensor, assign: Callable, sums: Callable, metric: str = "cosine", iters: int = 25,
          tol: float = 0.0, sqnorm: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None) -> KMeans:
    """The k-means loop over two callables (fit_kmeans passes the kernels, the tests a numpy mirror): up to `iters` assignments,
    each followed by the empty-cluster rule (reseed_empty) and -- unless the loop stops there -- the update.  It stops after an
    assignment when the labels equal the previous step's, when the relative drop of the inertia against the previous step is <=
    tol, or at `iters`; the update is skipped then, so the returned labels are always the assignment to the returned centroids.
    One host synchronisation per step."""
    _metric(metric)
    k = centroids.shape[0]
    history: List[float] = []
    prev_labels, converged, reseeds = None, False, 0
    labels = torch.full((x.shape[0],), -1, dtype=torch.int32, device=x.device)
    for it in range(max(int(iters), 1)):
        labels, best = assign(centroids)
        labels, centroids, e = reseed_empty(x, labels, best, centroids, metric)
        reseeds += e
        history.append(inertia_of(labels, best, metric, sqnorm, weights))
        if prev_labels is not None and bool(torch.equal(labels, prev_labels)):
            converged = True
            break
        if len(history) > 1 and history[-2] - history[-1] <= tol * abs(history[-2]):
            converged = True
            break
        if it + 1 >= iters:
            break
        s, wsum, _ = sums(labels)
        centroids = update_centroids(s, wsum, centroids, metric)
        prev_labels = labels
    counts = torch.bincount(labels[labels >= 0].long(), minlength=k)
    return KMeans(centroids, labels, counts, history[-1], history, len(history), converged, reseeds)


# ---- seeding ------------------------------------------------------------------------------------------------------------------------

def _unit(rows_: torch.Tensor) -> torch.Tensor:
    r = rows_.double()
    return (r / torch.linalg.vector_norm(r, dim=1, keepdim=True)).float()


def init_sample(valid_rows: torch.Tensor, k: int, gen: torch.Generator) -> torch.Tensor:
    """k distinct entries of valid_rows (the indices of the non-zero rows) by a seeded permutation."""
    m = int(valid_rows.numel())
    if m < k:
        raise GwbpError(f"k = {k} clusters need at least k non-zero rows, the field has {m}")
    return valid_rows[torch.randperm(m, generator=gen)[:k].to(valid_rows.device)]


def init_kmeanspp(x: torch.Tensor, valid_rows: torch.Tensor, k: int, metric: str, gen: torch.Generator, distance: Callable,
                  weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """D^2 sampling (k-means++) among a seeded sample of at most 64 k non-zero rows: the row indices of the k seeds.  Every uniform
    is drawn on the CPU from gen; distance(candidate_rows [m, D], centre [1, D]) -> float64 [m], the distance term of the metric
    (fit_kmeans: through kmeans_assign with K = 1), runs where x lives.  A candidate's chance is its (weighted) distance term to
    the nearest seed so far; the pick is the first candidate whose running sum exceeds u * total."""
    m_all = int(valid_rows.numel())
    if m_all < k:
        raise GwbpError(f"k = {k} clusters need at least k non-zero rows, the field has {m_all}")
    m = min(m_all, PP_CANDIDATES * k)
    cand = valid_rows[torch.randperm(m_all, generator=gen)[:m].to(valid_rows.device)]
    u = torch.rand(k, generator=gen, dtype=torch.float64).to(x.device)
    xc = x[cand]
    wc = weights[cand].double() if weights is not None else None
    first = torch.clamp((u[0] * m).long(), max=m - 1)
    picks = [first]
    d = None
    for i in range(1, k):
        di = distance(xc, xc[picks[-1]].unsqueeze(0)).clamp(min=0.0)
        di = torch.where(torch.isfinite(di), di, torch.zeros_like(di))
        d = di if d is None else torch.minimum(d, di)
        p = d * wc if wc is not None else d
        cs = torch.cumsum(p, dim=0)
        picks.append(torch.clamp(torch.searchsorted(cs, (u[i] * cs[-1]).unsqueeze(0), right=True)[0], max=m - 1))
    return cand[torch.stack(picks)]


def _distance_term(metric: str) -> Callable:
    def distance(xc: torch.Tensor, centre: torch.Tensor) -> torch.Tensor:
        c = _unit(centre) if metric == "cosine" else centre.float().contiguous()
        _, best = _assign(xc, c, centroid_bias(c, metric))
        if metric == "cosine":
            return 1.0 - best.double() / _norms(xc).double()
        return (xc.double() ** 2).sum(dim=1) - 2.0 * best.double()
    return distance


def fit_kmeans(features: torch.Tensor, k: int, metric: str = "cosine", iters: int = 25, tol: float = 0.0,
               init: Union[str, torch.Tensor] = "kmeans++", seed: int = 0, weights: Optional[torch.Tensor] = None) -> KMeans:
    """k-means (Lloyd) on a field.  One step is assign -> stable sort -> sums -> centroids: cosine, c_k = sums_k / |sums_k|
    (spherical k-means: give rows of comparable length, e.g. a finalised field); euclidean, c_k = sums_k / wsum_k; both in float64,
    rounded to float32 once.  Stops when the labels did not change, when the relative drop of the inertia is <= tol, or after `iters`
    assignments.  Inertia: cosine sum w (1 - <x, c>), euclidean sum w |x - c|^2 as |x|^2 - 2 score.  Rows of zero norm and rows
    with a NaN get label -1 and enter nothing.  Empty clusters: see reseed_empty.

    init: "kmeans++" (D^2 sampling among a seeded sample of at most 64 k non-zero rows), "sample" (k distinct non-zero rows by a
    seeded permutation) or a [k, D] tensor.  Every random number comes from a CPU torch.Generator(seed): the same inputs and seed
    give the same bits in every output.  weights: [N] non-negative row weights (e.g. the lift's d).  One host synchronisation per
    step."""
    _metric(metric)
    x, _ = field_rows(features, "features")  # float16 / bfloat16 fields stay as stored; centroids, sums and norms are float32 / 64
    n, d = x.shape
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise GwbpError(f"k must be in [1, {MAX_K}], got {k}")
    w = _weights(weights, n, x.device)
    norms = _norms(x)
    zero = norms == 0
    gen = torch.Generator().manual_seed(int(seed))
    if torch.is_tensor(init):
        if init.shape[0] != k:
            raise GwbpError(f"init has {init.shape[0]} rows for k = {k}")
        c0 = _centroids(init, d, x.device)
    elif init in ("sample", "kmeans++"):
        valid = torch.nonzero((norms > 0) & torch.isfinite(norms)).squeeze(1)
        pick = init_sample(valid, k, gen) if init == "sample" else init_kmeanspp(x, valid, k, metric, gen, _distance_term(metric), w)
        c0 = _unit(x[pick]) if metric == "cosine" else x[pick].float().contiguous()
    else:
        raise GwbpError(f"init must be 'kmeans++', 'sample' or a [k, D] tensor, got {init!r}")

    def assign(c):
        labels, best = _assign(x, c, centroid_bias(c, metric))
        labels[zero] = -1
        return labels, best

    return lloyd(x, c0, assign, lambda labels: _sums(x, labels, k, w), metric, iters, tol, norms.double() ** 2, w)


# ---- the field as a codebook --------------------------------------------------------------------------------------------------------

def quantize_field(features: torch.Tensor, k: int, **fit_kw) -> Tuple[torch.Tensor, torch.Tensor]:
    """(codebook [k, D] float32, codes [N] int32): the centroids of fit_kmeans(features, k, **fit_kw) and each row's centroid; -1
    for a zero or NaN row.  [N, D] floats become k D floats and N integers."""
    km = fit_kmeans(features, k, **fit_kw)
    return km.centroids, km.labels


def _codes(codebook: torch.Tensor, codes: torch.Tensor):
    if not torch.is_tensor(codebook) or codebook.dim() != 2:
        raise GwbpError("codebook must be a [k, D] tensor")
    if not torch.is_tensor(codes) or codes.dim() != 1 or codes.is_floating_point():
        raise GwbpError("codes must be an integer [N] tensor")
    k = codebook.shape[0]
    at = codes.to(codebook.device).long()
    return torch.where((at < 0) | (at >= k), torch.full_like(at, k), at)  # every code outside the codebook: the zero row k


def _with_zero_row(codebook: torch.Tensor) -> torch.Tensor:
    return torch.cat([codebook.float(), torch.zeros(1, codebook.shape[1], dtype=torch.float32, device=codebook.device)])


def dequantize_field(codebook: torch.Tensor, codes: torch.Tensor) -> torch.Tensor:
    """[N, D] float32: codebook[codes]; a code of -1 (or any code outside the codebook) gives a zero row."""
    return _with_zero_row(codebook)[_codes(codebook, codes)]


def codebook_prompt_scores(codebook: torch.Tensor, codes: torch.Tensor, prompts: torch.Tensor, normalize: bool = True):
    """prompt_scores of the dequantised field without making it: the [k, D] codebook is scored and the result gathered by code.
    A score is a function of the row alone, so this equals prompt_scores(dequantize_field(codebook, codes), prompts) bit for bit;
    code -1 scores as a zero row does."""
    from .segment import prompt_scores
    return prompt_scores(_with_zero_row(codebook), prompts, normalize)[_codes(codebook, codes)]


def codebook_prompt_mask(codebook: torch.Tensor, codes: torch.Tensor, prompts: torch.Tensor, n_pos: int,
                         threshold: Optional[float] = None) -> torch.Tensor:
    """prompt_mask of the dequantised field from the codebook: bool [N]."""
    from .segment import prompt_mask
    return prompt_mask(_with_zero_row(codebook), prompts, n_pos, threshold)[_codes(codebook, codes)]


# ---- seeded inputs (the CLI's --synthetic, the tests, tools/time_cluster.py) -------------------------------------------------------

def synthetic_clusters(n: int, k: int, d: int, noise: float = 0.3, seed: int = 0):
    """A seeded field with a planted partition: k unit directions, row g = unit-normalised (direction[label[g]] + noise * randn /
    sqrt(d)) with seeded labels that use every cluster.  Returns CPU tensors (features [n, d] float32, labels [n] int64, directions
    [k, d] float32)."""
    g = torch.Generator().manual_seed(seed)
    dirs = torch.randn(k, d, generator=g, dtype=torch.float64)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    labels = torch.cat([torch.arange(k), torch.randint(0, k, (max(n - k, 0),), generator=g)])[:n]
    labels = labels[torch.randperm(n, generator=g)]
    x = dirs[labels] + noise * torch.randn(n, d, generator=g, dtype=torch.float64) / d ** 0.5
    x = x / x.norm(dim=1, keepdim=True)
    return x.float(), labels, dirs.float()
