"""References for the radius components (csrc/components.hip, gsbp_amd.components).

components(): brute force in the contract's own arithmetic -- the neighbour matrix is spatial_ref.d2_f32 (the fp32 chain through
chain_ref.fma32) <= r2 with liveness and groups, the components are scipy's connected_components of the core-core graph, the
border rule and the numbering are the contract's.
radius_walk_ref(): a numpy mirror IN FLOAT32 of the kernel's ring walk and stop rule, in the style of spatial_ref.grid_knn_ref.
"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

from spatial_ref import F, _bound, build, cell_axis, d2_f32, finite_rows


def r2_of(radius):
    return F(F(radius) * F(radius))


def groups_of(n, group=None, mask=None):
    assert group is None or mask is None
    if mask is not None:
        return np.where(np.asarray(mask, bool), 0, -1).astype(np.int64)
    return np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)


def d2_matrix(q, p, rows=512):
    """[Q, N] float32: d2_f32(p[j], q[i]) (the kernel's dx = point - query), in row blocks."""
    q, p = np.asarray(q, F), np.asarray(p, F)
    out = np.empty((q.shape[0], p.shape[0]), F)
    for a in range(0, q.shape[0], rows):
        with np.errstate(invalid="ignore", over="ignore"):
            out[a:a + rows] = d2_f32(p[None, :, :], q[a:a + rows, None, :])
    return out


def neighbour_matrix(points, radius, group=None, mask=None, queries=None, query_group=None):
    """bool [Q, N] and the fp32 d2 matrix: query i and point j are neighbours.  queries None: the points with their own groups."""
    p = np.asarray(points, F)
    g = groups_of(p.shape[0], group, mask)
    live = finite_rows(p) & (g >= 0)
    if queries is None:
        q, qg, qlive = p, g, live
    else:
        q = np.asarray(queries, F)
        qg = groups_of(q.shape[0], query_group)
        qlive = finite_rows(q) & (qg >= 0)
    d2 = d2_matrix(q, p)
    with np.errstate(invalid="ignore"):
        nb = (d2 <= r2_of(radius)) & qlive[:, None] & live[None, :] & (qg[:, None] == g[None, :])
    return nb, d2


def radius_count_ref(points, radius, queries=None, group=None, query_group=None, cap=None):
    nb, _ = neighbour_matrix(points, radius, group, None, queries, query_group)
    count = nb.sum(axis=1)
    return (count if cap is None else np.minimum(count, cap)).astype(np.int32)


def components(points, radius, min_points=1, group=None, mask=None):
    """dict(labels int32 [N], sizes int64 [C], core bool [N], count int64 [N], border bool [N], ambiguous bool [N]): ambiguous marks
    the border points whose core neighbours lie in more than one component (where sklearn's visiting order decides)."""
    p = np.asarray(points, F)
    n = p.shape[0]
    nb, d2 = neighbour_matrix(p, radius, group, mask)
    count = nb.sum(axis=1)
    core = count >= min_points
    cc = nb & core[:, None] & core[None, :]
    _, comp = connected_components(csr_matrix(cc), directed=False)
    # number the components of core points by their smallest core member
    labels = np.full(n, -1, np.int64)
    ci = np.nonzero(core)[0]
    first = {}
    for i in ci:
        first.setdefault(comp[i], len(first))  # ascending i: the order of the smallest members
        labels[i] = first[comp[i]]
    border = np.zeros(n, bool)
    ambiguous = np.zeros(n, bool)
    for i in np.nonzero(~core & (count > 0))[0]:
        js = np.nonzero(nb[i] & core)[0]
        if js.size:
            border[i] = True
            j = js[np.lexsort((js, d2[i, js]))[0]]  # nearest core neighbour by (d2, index)
            labels[i] = labels[j]
            ambiguous[i] = np.unique(labels[js]).size > 1
    sizes = np.bincount(labels[labels >= 0], minlength=len(first)).astype(np.int64)
    return dict(labels=labels.astype(np.int32), sizes=sizes, core=core, count=count, border=border, ambiguous=ambiguous)


def radius_walk_ref(points, r2, lo, h, dims, queries=None):
    """(neighbours: per query the sorted array of the indices of the finite points with d2 <= r2, rings[Q]) by the kernel's walk:
    rings of Chebyshev radius r around the query's cell, clipped to the grid, until r2 is STRICTLY below the square of the smallest
    bound over the sides that still have cells, or no side has cells left.  A non-finite query finds nothing in 0 rings."""
    p = np.asarray(points, F)
    q = p if queries is None else np.asarray(queries, F)
    lo = [F(v) for v in lo]
    h, r2 = F(h), F(r2)
    nx, ny, nz = dims
    sp, perm, cell_start = build(p, lo, h, dims)
    found, rings = [], np.zeros(q.shape[0], np.int64)
    for i in range(q.shape[0]):
        mine = []
        if not np.isfinite(q[i]).all():
            found.append(np.zeros(0, np.int64))
            continue
        cx, cy, cz = (int(cell_axis(q[i, a], lo[a], h, dims[a])) for a in range(3))
        A = [F(q[i, a] - lo[a]) for a in range(3)]
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
            b, e = b[e > b], e[e > b]
            if b.size:
                ln = e - b  # the spans' positions, without a Python loop: each span's start repeated, plus the offset inside it
                at = np.repeat(b - np.concatenate([[0], np.cumsum(ln)[:-1]]), ln) + np.arange(ln.sum())
                mine.append(perm[at[d2_f32(sp[at], q[i]) <= r2]])
            rings[i] = r + 1
            lbs = []
            for a, c, n in ((0, cx, nx), (1, cy, ny), (2, cz, nz)):
                if c + r + 1 <= n - 1:
                    lbs.append(_bound(A[a], c + r + 1, h, True))
                if c - r - 1 >= 0:
                    lbs.append(_bound(A[a], c - r, h, False))
            if not lbs:
                break
            lb = min(lbs)
            with np.errstate(over="ignore"):
                if r2 < F(lb * lb):
                    break
        found.append(np.sort(np.concatenate(mine)) if mine else np.zeros(0, np.int64))
    return found, rings
