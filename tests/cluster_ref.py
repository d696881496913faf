"""TEST SUPPORT: float64 numpy mirror of the clustering of a field -- the assignment (inner product + per-centroid bias, argmax, ties
to the lowest index), the per-cluster sums (np.add.at), one Lloyd step and the loop with the package's empty-cluster and stop rules
-- and the two recipes whose rows are all decided.  No GPU, no torch."""
import numpy as np

import knn_ref

U = 2.0 ** -24
METRICS = ("cosine", "euclidean")


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def bias_of(C, metric):
    """None for cosine; -|c|^2 / 2 computed in float64 and rounded to float32 once for euclidean (what the caller hands the kernel)."""
    if metric == "cosine":
        return None
    return (-0.5 * (f64(C) ** 2).sum(axis=1)).astype(np.float32)


def scores64(X, C, b=None):
    """Float64 scores [N, K] of the fp32 inputs: <x, c_j> + b_j."""
    s = f64(X) @ f64(C).T
    return s if b is None else s + f64(b)[None, :]


def eps(X, C, b=None):
    """Per row: 2 (D + 1) u |x| max|c| + 4 u (|x| max|c| + max|b|) -- knn_ref.eps, twice the worst-case error of an fp32 dot product
    of length D in any order, plus twice the error of one fp32 addition of the bias to it (|sum| <= |x| max|c| + max|b|, and the
    float32 rounding of b itself; b None: max|b| = 0)."""
    X, C = f64(X), f64(C)
    xc = np.linalg.norm(X, axis=1) * np.linalg.norm(C, axis=1).max()
    mb = 0.0 if b is None else np.abs(f64(b)).max()
    return 2.0 * (X.shape[1] + 1) * U * xc + 4.0 * U * (xc + mb)


def assign(X, C, b=None, sc=None):
    """(labels [N] int64, best [N] float64): argmax of the float64 scores, ties to the lowest index; a row whose scores are all NaN
    gets -1 / NaN; a NaN score is never chosen over a number."""
    sc = scores64(X, C, b) if sc is None else sc
    safe = np.where(np.isnan(sc), -np.inf, sc)
    lab = safe.argmax(axis=1)
    best = sc[np.arange(sc.shape[0]), lab]
    dead = np.isnan(sc).all(axis=1)
    return np.where(dead, -1, lab), np.where(dead, np.nan, best)


def decided_rows(sc, e):
    """Rows whose float64 gap between the best and the second-best score exceeds eps."""
    if sc.shape[1] < 2:
        return np.ones(sc.shape[0], bool)
    top = -np.partition(-sc, (0, 1), axis=1)[:, :2]
    return (top[:, 0] - top[:, 1]) > e


def sums(X, labels, K, w=None):
    """(sums [K, D], wsum [K], counts [K]) in float64 / int64 with np.add.at; labels outside [0, K) take no part."""
    X = f64(X)
    labels = np.asarray(labels).astype(np.int64)
    w = np.ones(X.shape[0]) if w is None else f64(w)
    on = (labels >= 0) & (labels < K)
    s, ws, cnt = np.zeros((K, X.shape[1])), np.zeros(K), np.zeros(K, np.int64)
    np.add.at(s, labels[on], w[on, None] * X[on])
    np.add.at(ws, labels[on], w[on])
    np.add.at(cnt, labels[on], 1)
    return s, ws, cnt


def abs_sums(X, labels, K, w=None):
    """sum |w x| per (cluster, column): the scale of the any-order summation bound."""
    return sums(np.abs(f64(X)), labels, K, None if w is None else np.abs(f64(w)))[0]


def centroids_of(s, ws, previous, metric):
    """cosine: s_k / |s_k|; euclidean: s_k / ws_k; float64, rounded to float32 once; a cluster without a direction keeps `previous`."""
    if metric == "cosine":
        norm = np.linalg.norm(s, axis=1, keepdims=True)
        ok = (norm > 0) & (ws > 0)[:, None]
        new = s / np.where(ok, norm, 1.0)
    else:
        ok = (ws > 0)[:, None]
        new = s / np.where(ok, ws[:, None], 1.0)
    return np.where(ok, new.astype(np.float32), np.asarray(previous, np.float32))


def reseed_empty(X, labels, best, C, metric):
    """The e empty clusters take, in ascending cluster order, the e assigned rows of lowest best (ties by row index): each row
    becomes its cluster's centroid (unit length for cosine) and its only member.  Returns (labels, C, e)."""
    K = C.shape[0]
    cnt = np.bincount(labels[labels >= 0], minlength=K)
    empty = np.nonzero(cnt == 0)[0]
    if empty.size == 0:
        return labels, C, 0
    cand = np.nonzero(labels >= 0)[0]
    worst = cand[np.argsort(best[cand], kind="stable")[:empty.size]]
    empty = empty[:worst.size]
    labels, C = labels.copy(), np.array(C, np.float32)
    labels[worst] = empty
    seed = f64(X)[worst]
    if metric == "cosine":
        seed = seed / np.linalg.norm(seed, axis=1, keepdims=True)
    C[empty] = seed.astype(np.float32)
    return labels, C, int(worst.size)


def inertia(X, labels, best, metric, w=None):
    X = f64(X)
    term = (1.0 - best) if metric == "cosine" else ((X ** 2).sum(axis=1) - 2.0 * best)
    if w is not None:
        term = term * f64(w)
    return float(np.where(labels >= 0, term, 0.0).sum())


def assign_rows(X, C, metric):
    """The assignment of the package's kmeans_assign: zero rows get -1."""
    lab, best = assign(X, C, bias_of(C, metric))
    lab = np.where(np.linalg.norm(f64(X), axis=1) == 0, -1, lab)
    return lab, best


def lloyd_step(X, C, metric, w=None):
    """(labels, best, new centroids, counts, reseeded) of one step from C."""
    lab, best = assign_rows(X, C, metric)
    lab, seeded, e = reseed_empty(X, lab, best, C, metric)
    s, ws, cnt = sums(X, lab, C.shape[0], w)
    return lab, best, centroids_of(s, ws, seeded, metric), cnt, e


def lloyd(X, C, metric="cosine", iters=25, tol=0.0, w=None):
    """The loop: dict(centroids, labels, history, n_iter, converged, reseeds).  Stops after an assignment when the labels equal the
    previous step's, when the inertia's relative drop is <= tol, or at iters; the update is skipped then."""
    C = np.asarray(C, np.float32)
    history, prev, converged, reseeds = [], None, False, 0
    for it in range(max(iters, 1)):
        lab, best = assign_rows(X, C, metric)
        lab, C, e = reseed_empty(X, lab, best, C, metric)
        reseeds += e
        history.append(inertia(X, lab, best, metric, w))
        if prev is not None and np.array_equal(lab, prev):
            converged = True
            break
        if len(history) > 1 and history[-2] - history[-1] <= tol * abs(history[-2]):
            converged = True
            break
        if it + 1 >= iters:
            break
        s, ws, _ = sums(X, lab, C.shape[0], w)
        C = centroids_of(s, ws, C, metric)
        prev = lab
    return dict(centroids=C, labels=lab, history=history, n_iter=len(history), converged=converged, reseeds=reseeds)


# ---- the two recipes ----------------------------------------------------------------------------------------------------------------

def make_case(metric, D, K, N, rng):
    """(X [N, D], C [K, D]) float32.  cosine: knn_ref.make_case with the centroids as sources (unit centroids, rows = unit-normalised
    noisy copies).  euclidean: centroids 3 randn, rows = a random centroid + 0.5 randn."""
    if metric == "cosine":
        X, C = knn_ref.make_case(D, K, N, rng)
        return X, C
    C = 3.0 * rng.standard_normal((K, D))
    X = C[rng.integers(0, K, N)] + 0.5 * rng.standard_normal((N, D))
    return X.astype(np.float32), C.astype(np.float32)
