"""TEST SUPPORT: the contract of csrc/regions.hip (include/gwbp.h) in numpy float32, no GPU.

    dot(i, j), sq(i)   lane l of 64 owns the channels 256 s + 4 l + e (those < D) and runs acc = fma32(a, b, acc) from +0 in the order
                       (s, e) -- chain_ref.fma32, vectorised over the pairs; the 64 partial sums are combined by the butterfly p_l = p_l +
                       p_(l xor o), o = 1, 2, 4, 8, 16, 32
    norm, liveness     np.sqrt in float32; finite sq and norm >= float32(1e-12)
    sim[i, c]          one float32 multiply, one float32 divide; NaN for no neighbour or a dead row
    edges -> labels    scipy's connected_components over the live points, numbered by the smallest member

A channel >= D enters as a product of zeros here, which leaves the bits as skipping it would.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from chain_ref import fma32

F = np.float32
EPS = F(1e-12)
LANES = np.arange(64)


def lane_partials(A, B):
    """[m, 64] float32: every lane's chain over its channels for the row pairs (A[r], B[r]); A, B [m, D] float32."""
    A, B = np.asarray(A, F), np.asarray(B, F)
    m, D = A.shape
    ns = -(-D // 256)
    Ap, Bp = np.zeros((m, ns * 256), F), np.zeros((m, ns * 256), F)
    Ap[:, :D], Bp[:, :D] = A, B
    Ap, Bp = Ap.reshape(m, ns, 64, 4), Bp.reshape(m, ns, 64, 4)
    acc = np.zeros((m, 64), F)
    for s in range(ns):
        for e in range(4):
            acc = fma32(Ap[:, s, :, e], Bp[:, s, :, e], acc)
    return acc


def butterfly(p):
    """[m] float32 from the partial sums [m, 64]: p_l = p_l + p_(l xor o) for o = 1, 2, 4, 8, 16, 32; every lane ends with lane 0's bits."""
    p = np.asarray(p, F)
    with np.errstate(invalid="ignore", over="ignore"):
        for o in (1, 2, 4, 8, 16, 32):
            p = (p + p[:, LANES ^ o]).astype(F)
    return p[:, 0]


def dots(A, B):
    return butterfly(lane_partials(A, B))


def similarity(features, idx):
    """(sim float32 [N, k], live bool [N]) of the contract."""
    X = np.asarray(features, F)
    idx = np.asarray(idx)
    n, k = idx.shape
    sq = dots(X, X)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        norm = np.sqrt(sq)
        live = np.isfinite(sq) & (norm >= EPS)
        sim = np.full((n, k), np.nan, F)
        valid = (idx >= 0) & (idx < n)
        i, c = np.nonzero(valid)
        j = idx[i, c]
        if len(i):
            d = dots(X[i], X[j])
            s = (d / (norm[i] * norm[j]).astype(F)).astype(F)
            sim[i, c] = np.where(live[i] & live[j], s, F(np.nan))
    return sim, live


def edges(idx, sim, live, dist=None, group=None, sim_min=0.9, max_dist=np.inf):
    """(i [E], j [E]) of the contract's edges as listed (one direction each), and the live mask with the groups applied."""
    idx = np.asarray(idx)
    n, k = idx.shape
    grp = np.zeros(n, np.int64) if group is None else np.asarray(group).astype(np.int64)
    alive = np.asarray(live, bool) & (grp >= 0)
    valid = (idx >= 0) & (idx < n)
    j = np.where(valid, idx, 0)
    i = np.broadcast_to(np.arange(n)[:, None], idx.shape)
    with np.errstate(invalid="ignore"):
        ok = valid & (j != i) & alive[i] & alive[j] & (grp[i] == grp[j]) & (np.asarray(sim, F) >= F(sim_min))
        if dist is not None and F(max_dist) < np.inf:
            ok &= np.asarray(dist, F) <= F(max_dist)
    return i[ok], j[ok], alive


def dense(root):
    """(labels int32 [N], sizes int64 [C]): components.dense_labels in numpy."""
    root = np.asarray(root)
    uniq = np.unique(root[root >= 0])
    labels = np.full(len(root), -1, np.int32)
    labels[root >= 0] = np.searchsorted(uniq, root[root >= 0]).astype(np.int32)
    return labels, np.bincount(labels[labels >= 0], minlength=len(uniq)).astype(np.int64)


def components(features, idx, dist=None, group=None, sim_min=0.9, max_dist=np.inf, sim_live=None):
    """dict(sim, live (feature-live), core (live with groups), root, labels, sizes) of the contract."""
    sim, live = similarity(features, idx) if sim_live is None else sim_live
    n = len(live)
    ei, ej, alive = edges(idx, sim, live, dist, group, sim_min, max_dist)
    _, comp = connected_components(coo_matrix((np.ones(len(ei), np.int8), (ei, ej)), shape=(n, n)), directed=False)
    smallest = np.full(n, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    root = np.where(alive, smallest[comp], -1)
    labels, sizes = dense(root)
    return dict(sim=sim, live=live, core=alive, root=root, labels=labels, sizes=sizes)


def same_bits(a, b):
    """Equal float32 arrays bit for bit, every NaN counted as one value (the kernel writes one NaN; numpy may make another)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


# ---- inputs the CPU and the GPU tests share -------------------------------------------------------------------------------------------

def binary_rows(n=96, d=40, seed=0):
    """Rows of {0, 1}^d with 4 or 16 ones: sq is 4 or 16, every norm product 4, 8 or 16, every cosine m / 4, m / 8 or m / 16 -- exact
    in float32 and in float64 alike."""
    rng = np.random.default_rng(seed)
    X = np.zeros((n, d), F)
    for r in range(n):
        X[r, rng.choice(12 if r % 2 else d, 4 if r % 2 else 16, replace=False)] = 1.0  # (the sparse rows share a few columns: overlaps)
    return X


def random_lists(n, k, seed):
    return np.random.default_rng(seed).integers(0, n, (n, k)).astype(np.int32)
