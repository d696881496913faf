"""References for the spatial k-NN search (csrc/spatial.hip).

brute(): all distances in float64, each row ordered by (distance, index).
grid_knn_ref(): a numpy mirror IN FLOAT32 of the kernel's cell assignment, ring walk and stop rule -- the only way to check the stop
rule without a GPU.  Its fused multiply-adds are chain_ref.fma32: the fp32 fmaf, correctly rounded on every input.
"""
import numpy as np

from chain_ref import fma32  # noqa: F401  (d2_f32 below; the tests call it by this name)

F = np.float32
NO_INDEX = 0x7FFFFFFF


def finite_rows(p):
    return np.isfinite(p).all(axis=1)


def brute(points, k, queries=None):
    """(dist[Q, k] float64, idx[Q, k] int64): the k points of smallest Euclidean distance in float64, ties by index; non-finite
    points are nobody's neighbour, a non-finite query gets -1 / NaN, a short row -1 / +inf in the tail."""
    p = np.asarray(points, np.float64)
    q = p if queries is None else np.asarray(queries, np.float64)
    ok = finite_rows(p)
    cand = np.nonzero(ok)[0]
    dist = np.full((q.shape[0], k), np.inf)
    idx = np.full((q.shape[0], k), -1, np.int64)
    for i in range(q.shape[0]):
        if not np.isfinite(q[i]).all():
            dist[i] = np.nan
            continue
        d = p[cand] - q[i]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]  # (exact on the lattice sets; the order there is the kernel's)
        o = np.lexsort((cand, d2))[:k]
        dist[i, :o.size] = np.sqrt(d2[o])
        idx[i, :o.size] = cand[o]
    return dist, idx


def cell_axis(x, lo, h, n):
    """The kernel's cell_axis in float32: floorf((x - lo) / h) clamped to [0, n - 1]."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.nan_to_num(np.floor((F(x) - F(lo)) / F(h)), nan=0.0, posinf=np.inf, neginf=-np.inf)  # (non-finite rows only: they get the sentinel key)
    return np.minimum(np.maximum(t, F(0)), F(n - 1)).astype(np.int64)


def cell_keys(p, lo, h, dims):
    p = np.asarray(p, F)
    c = [cell_axis(p[:, a], lo[a], h, dims[a]) for a in range(3)]
    key = (c[2] * dims[1] + c[1]) * dims[0] + c[0]
    return np.where(finite_rows(p), key, dims[0] * dims[1] * dims[2])


def build(points, lo, h, dims):
    """(sorted points float32 [N, 3], their original indices, cell_start[cells + 1]) as k_spatial_build writes them."""
    p = np.asarray(points, F)
    keys = cell_keys(p, lo, h, dims)
    perm = np.argsort(keys, kind="stable")
    cells = dims[0] * dims[1] * dims[2]
    cell_start = np.searchsorted(keys[perm], np.arange(cells + 1), side="left")
    return p[perm], perm, cell_start


def d2_f32(p, q):
    """fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with dx = p.x - q.x in float32."""
    with np.errstate(over="ignore"):
        d = (np.asarray(p, F) - np.asarray(q, F)).astype(F)
        return fma32(d[..., 2], d[..., 2], fma32(d[..., 1], d[..., 1], (d[..., 0] * d[..., 0]).astype(F)))


def _bound(A, kf, h, above, margin=True):
    KH = F(F(kf) * F(h))
    B = F(KH - A) if above else F(A - KH)
    LB = F(B - F(F(abs(KH) + abs(A)) * F(2.0 ** -21))) if margin else B
    return LB if LB > 0 else F(0)


def grid_knn_ref(points, k, lo, h, dims, queries=None, return_rings=False, margin=True):
    """(dist[Q, k] float32, idx[Q, k] int64) by the kernel's walk: rings of Chebyshev radius r around the query's cell, clipped to
    the grid, until the k-th squared distance is strictly below the square of the smallest bound over the sides that still have
    cells.  return_rings: also the number of rings each query visited."""
    p = np.asarray(points, F)
    q = p if queries is None else np.asarray(queries, F)
    lo = [F(v) for v in lo]
    h = F(h)
    nx, ny, nz = dims
    sp, perm, cell_start = build(p, lo, h, dims)
    dist = np.full((q.shape[0], k), np.inf, F)
    idx = np.full((q.shape[0], k), -1, np.int64)
    rings = np.zeros(q.shape[0], np.int64)
    for i in range(q.shape[0]):
        if not np.isfinite(q[i]).all():
            dist[i] = np.nan
            continue
        cx, cy, cz = (int(cell_axis(q[i, a], lo[a], h, dims[a])) for a in range(3))
        A = [F(q[i, a] - lo[a]) for a in range(3)]
        best_d = np.full(k, np.inf, F)
        best_i = np.full(k, NO_INDEX, np.int64)
        for r in range(max(dims) + 1):
            x0, x1 = max(cx - r, 0), min(cx + r, nx - 1)
            zs, ys = np.meshgrid(np.arange(max(cz - r, 0), min(cz + r, nz - 1) + 1),
                                 np.arange(max(cy - r, 0), min(cy + r, ny - 1) + 1), indexing="ij")
            base = ((zs * ny + ys) * nx).ravel()
            shell = ((np.abs(zs - cz) == r) | (np.abs(ys - cy) == r)).ravel()  # the whole run along x lies in the ring
            b, e = [cell_start[base[shell] + x0]], [cell_start[base[shell] + x1 + 1]]
            for x in ((cx - r, cx + r) if r > 0 else ()):                      # elsewhere only the two ends do
                if 0 <= x <= nx - 1:
                    b.append(cell_start[base[~shell] + x])
                    e.append(cell_start[base[~shell] + x + 1])
            b, e = np.concatenate(b), np.concatenate(e)
            spans = [(lo_, hi_) for lo_, hi_ in zip(b, e) if hi_ > lo_]
            at = np.concatenate([np.arange(b, e) for b, e in spans]) if spans else np.zeros(0, np.int64)
            if at.size:
                d2 = np.concatenate([best_d, d2_f32(sp[at], q[i])])
                ids = np.concatenate([best_i, perm[at]])
                o = np.lexsort((ids, d2))[:k]
                best_d, best_i = d2[o], ids[o]
            rings[i] = r + 1
            lbs = []
            for a, c, n in ((0, cx, nx), (1, cy, ny), (2, cz, nz)):
                if c + r + 1 <= n - 1:
                    lbs.append(_bound(A[a], c + r + 1, h, True, margin))
                if c - r - 1 >= 0:
                    lbs.append(_bound(A[a], c - r, h, False, margin))
            if not lbs:
                break
            lb = min(lbs)
            with np.errstate(over="ignore"):
                if best_d[k - 1] < F(lb * lb):
                    break
        have = best_i != NO_INDEX
        dist[i, have] = np.sqrt(best_d[have])
        idx[i, have] = best_i[have]
    return (dist, idx, rings) if return_rings else (dist, idx)


# ---- the lattice sets: coordinates i / 64 with |i| < 2^10 (+ an optional common offset of 1024), so that every difference, square
# and sum of the distance is exact in fp32 and in float64 alike: indices and distances must agree bit for bit, ties included ------

def lattice(n_side=8, seed=0, offset=0.0):
    g = np.arange(n_side)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float64) * (4.0 / 64.0)  # on 1/16 cell faces
    rng = np.random.default_rng(seed)
    return (pts[rng.permutation(pts.shape[0])] + offset).astype(F)


def lattice_sets(n_side=8, offset=0.0):
    """name -> points [N, 3] float32 (N >= 32 except 'n_equals_k', which test code cuts to k)."""
    rng = np.random.default_rng(7)
    lat = lattice(n_side, 0, offset)
    dup = np.concatenate([lat, lat])[rng.permutation(2 * lat.shape[0])]
    same = np.full((40, 3), 5.0 / 64.0 + offset, F)
    plane = np.zeros((64, 3), F)
    plane[:, 0], plane[:, 1] = (np.arange(64) % 8) / 16.0, (np.arange(64) // 8) / 64.0
    plane = (plane + offset).astype(F)
    line = np.zeros((48, 3), F)
    line[:, 2] = (rng.permutation(48) - 20) / 64.0
    line = (line + offset).astype(F)
    # two 3^3 clusters of spacing 1/2 and ten floaters with coordinates in {-1024, 0, 1024}: differences are multiples of 1/2 below
    # 2^11, so three squares still sum exactly in fp32's 24 bits
    g = np.arange(3) / 2.0
    small = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    cl = np.concatenate([small, small + 2.0])
    far = rng.integers(-1, 2, (10, 3)) * 1024.0
    far[(far == 0).all(axis=1)] = 1024.0
    clusters = (np.concatenate([cl, far])[rng.permutation(cl.shape[0] + 10)] + offset).astype(F)
    return {"lattice": lat, "duplicates": dup, "identical": same, "coplanar": plane, "collinear": line, "clusters_floaters": clusters}


def grids_for(points, one_per_cell_h):
    """name -> (lo, h, dims): the issue's 1/16 grid on the points' own box, one cell, 2 cells per axis, about one point per cell."""
    p = np.asarray(points, np.float64)
    p = p[finite_rows(p)]
    inside = p[(np.abs(p - np.median(p, axis=0)) < 100).all(axis=1)]
    lo, hi = inside.min(axis=0), inside.max(axis=0)
    ext = np.maximum(hi - lo, 0)

    def dims(h):
        return tuple(int(min(max(np.ceil(e / h), 1), 1024)) for e in ext)

    half = float(max(ext.max() / 2, 1.0 / 64.0))
    return {"sixteenth": (tuple(lo), 1.0 / 16.0, dims(1.0 / 16.0)), "one_cell": (tuple(lo), 1.0, (1, 1, 1)),
            "two_per_axis": (tuple(lo), half, tuple(2 if e > 0 else 1 for e in ext)),
            "one_per_cell": (tuple(lo), one_per_cell_h, dims(one_per_cell_h))}
