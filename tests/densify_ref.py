"""The yardstick of densification (csrc/densify.hip, csrc/densify_math.h) in numpy.

Two restatements:

  * the FUSED rule as the kernels run it, in float32 and in the documented operation order -- accumulate, plan, emit, gather.  The
    build forbids contraction and rounds divide and sqrt correctly, and numpy's float32 ufuncs round each operation once, so this gives
    the kernels' bits.  The one exception is exp in a split child's offset: numpy's float32 exp and the device's expf may differ in the
    last bit, so split_means takes the exponentials as an optional argument and split_bound says how far a float32 result may lie from
    the float64 formula whatever exp was used.
  * the LITERAL two steps of gsplat's DefaultStrategy -- duplicate, then split, then prune, with boolean masks and concatenation, the
    new rows appended behind the old ones (literal_two_steps).  It decides in the same pre-activation space and calls the same
    split_means, so that it yields the same MULTISET of rows as the fused rule, bit for bit, in another order.

`mutant` arguments build deliberately wrong variants; tests/test_densify_cpu.py shows that each of them is caught.
"""
import numpy as np

F = np.float32
PRUNED, KEEP, CLONE, SPLIT = 0, 1, 2, 3
ROWS_OUT = np.array([0, 1, 2, 2], dtype=np.int64)


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


# ---- accumulate ------------------------------------------------------------------------------------------------------------------
def accumulate(grad2d, count, v_means2d, radii, sx, sy):
    """(grad2d, count) after one call: the cameras in order; where radii > 0, grad2d += sqrt(a a + b b), a = gx sx, b = gy sy."""
    g, n = f32(grad2d).copy(), f32(count).copy()
    v, radii = f32(v_means2d), np.asarray(radii)
    sx, sy = F(sx), F(sy)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(v.shape[0]):
            a = v[c, :, 0] * sx
            b = v[c, :, 1] * sy
            norm = np.sqrt(a * a + b * b)
            vis = radii[c] > 0
            g = np.where(vis, g + norm, g).astype(np.float32)
            n = np.where(vis, n + F(1.0), n).astype(np.float32)
    return g, n


# ---- plan ------------------------------------------------------------------------------------------------------------------------
def largest_scale(scaling):
    s = f32(scaling)
    m = s[:, 0]
    m = np.where(s[:, 1] > m, s[:, 1], m)
    return np.where(s[:, 2] > m, s[:, 2], m)


def flags(grad2d, count, scaling, opacity, th, mutant=None):
    """(low, high, small, m): the three tests of the rule in pre-activation space.  th = (t_grad, t_small, t_big, t_opa, log16)."""
    t_grad, t_small, _, t_opa, _ = (F(t) for t in th)
    m = largest_scale(scaling)
    c = f32(count)
    d = np.where(c > F(1.0), c, F(1.0))
    with np.errstate(invalid="ignore"):
        g = f32(grad2d) / d
        low = f32(opacity) < t_opa
        high = (g >= t_grad) if mutant == "ge_grad" else (g > t_grad)
        small = m <= t_small
    return low, high, small, m


def plan(grad2d, count, scaling, opacity, th, prune_big, mutant=None):
    """(kind uint8 [N], offsets int64 [N + 1]): gsplat's grow followed by its prune, composed per Gaussian."""
    t_big, log16 = F(th[2]), F(th[4])
    low, high, small, m = flags(grad2d, count, scaling, opacity, th, mutant)
    with np.errstate(invalid="ignore"):
        big = bool(prune_big) & (m > t_big)
        child_big = big if mutant == "prune_before_shrink" else bool(prune_big) & ((m - log16) > t_big)
    kind = np.where(high & small, CLONE, np.where(high & ~small, SPLIT, KEEP))
    gone = low | np.where(kind == SPLIT, child_big, big)
    kind = np.where(gone, PRUNED, kind).astype(np.uint8)
    rows = ROWS_OUT[kind]
    incl = np.cumsum(rows)
    offsets = np.concatenate([incl, incl[-1:] if len(incl) else np.zeros(1, np.int64)]) if mutant == "inclusive" \
        else np.concatenate([np.zeros(1, np.int64), incl])
    return kind, offsets.astype(np.int64)


# ---- the children of a split ---------------------------------------------------------------------------------------------------
def split_means(means, scaling, rotation, noise, exp_scaling=None, dtype=np.float32):
    """mean + R(q / |q|) (exp(scaling) * noise) in `dtype`, in the order of csrc/densify_math.h densify_split.  noise [M, 3].
    exp_scaling: the exponentials to use instead of numpy's (float32 only: somebody else's expf)."""
    T = np.dtype(dtype).type
    mu, s, q, z = (np.asarray(a, dtype=dtype) for a in (means, scaling, rotation, noise))
    one, two = T(1.0), T(2.0)
    n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    inv = one / np.sqrt(n2)
    w, x, y, zz = q[:, 0] * inv, q[:, 1] * inv, q[:, 2] * inv, q[:, 3] * inv
    # (the exponential of the float32 scaling rounded ONCE: numpy's own float32 exp is a vector routine that is off by up to two units
    # in the last place on a third of its arguments, which would make it the odd one out beside any libm)
    e = np.exp(s.astype(np.float64)).astype(dtype) if exp_scaling is None else np.asarray(exp_scaling, dtype=dtype)
    v0, v1, v2 = e[:, 0] * z[:, 0], e[:, 1] * z[:, 1], e[:, 2] * z[:, 2]
    r00, r01, r02 = one - two * (y * y + zz * zz), two * (x * y - w * zz), two * (x * zz + w * y)
    r10, r11, r12 = two * (x * y + w * zz), one - two * (x * x + zz * zz), two * (y * zz - w * x)
    r20, r21, r22 = two * (x * zz - w * y), two * (y * zz + w * x), one - two * (x * x + y * y)
    return np.stack([mu[:, 0] + ((r00 * v0 + r01 * v1) + r02 * v2), mu[:, 1] + ((r10 * v0 + r11 * v1) + r12 * v2),
                     mu[:, 2] + ((r20 * v0 + r21 * v1) + r22 * v2)], axis=1)


# How far a float32 split mean may lie from the float64 formula on the same float32 inputs, per component i:
#
#     |float32 - float64| <= 2^-21 (|mean_i| + 3 s |z|),   s = the largest exp(scaling) of the row, |z| = the noise row's 2-norm.
#
# Derivation, from the operation count of the chain (u = 2^-24, one rounding; first order in u):
#   q / |q|   n2 is four products and three sums of non-negative terms: relative error <= 4 u; sqrt halves it and rounds: 3 u; the
#             reciprocal: 4 u; the product with q_k: 5 u.  The 4 u is COMMON to the four components: it scales the quaternion and turns
#             R into R + 2 e (R - I), |e| <= 4 u.  The last u is each component's own.
#   R         an entry is two products of components (own part: 2 u + 1 u each), their sum or difference (1 u), a doubling (exact)
#             and, on the diagonal, 1 - t (1 u): with |x y| + |w z| <= 1/2 and y^2 + z^2 <= 1 the own part is <= 4 u off the diagonal
#             and <= 9 u on it, absolute.
#   v         exp (<= 2 u: one ulp, the library's bound, either library) and the product with the noise: 3 u relative, |v_j| <= s |z_j|.
#   the sum   three products (1 u each on |R_ij v_j| <= |v_j|), two sums (<= 2 u on |sum|), the sum with the mean: 1 u on
#             |mean_i| + |d_i|.
# Adding up, per component, with |v| <= s |z| (2-norms) and sum_j |v_j| <= sqrt(3) |v|:
#   the common scaling of q moves d = R v by 2 e (R - I) v, at most 2 . 4 u . 2 |v| = 16 u s |z|;
#   the entries' own roundings, (9 + 4 + 4) u times |v_j| <= s |z| each, at most 17 u s |z|;
#   v's own 3 u and the sum's 3 u on sum_j |R_ij| |v_j| <= |v|: 6 u s |z|;  the last sum: 1 u (|mean_i| + s |z|).
# Every one of these with the same sign gives 40 u s |z| + u |mean_i|: a worst case this count does not exclude, and no row comes near
# it -- the forty-odd roundings are independent, their sum grows like the square root of their number, and the common scaling mostly
# cancels in (R - I) v.  The design sets 2^-21 = 8 u on (|mean_i| + 3 s |z|), i.e. 24 u s |z| + 8 u |mean_i|: the common-scaling
# term in full and a third of the own roundings' worst case.  That figure is the one asserted, as set; tests/test_densify_cpu.py prints
# the largest error over the bound beside it (0.29 on 100 000 seeded rows, median 0.03), and the device's children are held to the same
# bound (tests/test_gpu_densify.py: at most 0.31).
SPLIT_BOUND = 2.0 ** -21


def split_bound(means, scaling, noise):
    """[M, 3] float64: SPLIT_BOUND (|mean_i| + 3 s |z|) of each split child (see the derivation above)."""
    mu, s, z = (np.asarray(a, dtype=np.float64) for a in (means, scaling, noise))
    reach = 3.0 * np.exp(s).max(axis=1) * np.sqrt((z * z).sum(axis=1))
    return SPLIT_BOUND * (np.abs(mu) + reach[:, None])


# ---- emit and gather -----------------------------------------------------------------------------------------------------------
def emit(kind, offsets, means, scaling, rotation, opacity, noise, log16, exp_scaling=None):
    """dict(parent int32 [N'], child uint8 [N'], means, scaling, rotation, opacity): every parent's children at offsets[p], in parent
    order.  keep / clone copy the row; split: split_means and scaling - log16.  noise [N, 2, 3]."""
    kind = np.asarray(kind)
    rows = ROWS_OUT[kind]
    n_out = int(rows.sum())
    parent = np.repeat(np.arange(len(kind), dtype=np.int32), rows)
    child = (np.arange(n_out) - np.asarray(offsets)[:-1][parent]).astype(np.uint8)
    mu, s, q, o, z = f32(means), f32(scaling), f32(rotation), f32(opacity), f32(noise)
    out = dict(parent=parent, child=child, means=mu[parent].copy(), scaling=s[parent].copy(), rotation=q[parent].copy(),
               opacity=o[parent].copy())
    sp = kind[parent] == SPLIT
    if sp.any():
        p, c = parent[sp], child[sp]
        e = None if exp_scaling is None else f32(exp_scaling)[p]
        out["means"][sp] = split_means(mu[p], s[p], q[p], z[p, c], e)
        out["scaling"][sp] = s[p] - F(log16)
    return out


def gather(table, parent, child=None, kind=None, mode="copy", mutant=None):
    """out[r] = table[parent[r]]; "zero_new": zeros where the parent was split, or was cloned and this is the copy (child 1)."""
    out = np.asarray(table)[parent].copy()
    if mode == "zero_new":
        k = np.asarray(kind)[parent]
        new = (k == SPLIT) | ((k == CLONE) & ((np.asarray(child) == 0) if mutant == "zero_original" else (np.asarray(child) != 0)))
        out[new] = 0
    return out


# ---- gsplat's two steps, literally ------------------------------------------------------------------------------------------------
def literal_two_steps(grad2d, count, tables, th, prune_big, noise, moments=None, exp_scaling=None):
    """duplicate -> split -> prune as gsplat's DefaultStrategy runs them (_grow_gs, then _prune_gs on the grown set), with boolean masks
    and concatenation: clones are appended behind the set, then the split rows are removed and their two children appended, then the
    prune masks the grown set.  tables: dict(means, scaling, rotation, opacity, ...further [N, ...] tables).  moments: an optional table
    that follows gsplat's optimiser-state rule (zeros for every appended row).  Returns (tables', moments') of the new set, in gsplat's
    order -- not the fused rule's."""
    t = {k: np.asarray(v).copy() for k, v in tables.items()}
    mom = None if moments is None else np.asarray(moments).copy()
    low, high, small, _ = flags(grad2d, count, t["scaling"], t["opacity"], th)
    n = len(high)
    is_dupli, is_split = high & small, high & ~small
    idx = np.arange(n)
    # duplicate
    sel = idx[is_dupli]
    t = {k: np.concatenate([v, v[sel]]) for k, v in t.items()}
    if mom is not None:
        mom = np.concatenate([mom, np.zeros_like(mom[sel])])
    is_split = np.concatenate([is_split, np.zeros(len(sel), dtype=bool)])
    # split: the rows leave, two children each are appended (first children, then second children)
    sel = np.nonzero(is_split)[0]
    rest = ~is_split
    e = None if exp_scaling is None else f32(exp_scaling)[sel]
    kids = []
    for c in range(2):
        kid = {k: v[sel].copy() for k, v in t.items()}
        kid["means"] = split_means(t["means"][sel], t["scaling"][sel], t["rotation"][sel], f32(noise)[sel, c], e)
        kid["scaling"] = f32(t["scaling"][sel]) - F(th[4])
        kids.append(kid)
    t = {k: np.concatenate([v[rest], kids[0][k], kids[1][k]]) for k, v in t.items()}
    if mom is not None:
        mom = np.concatenate([mom[rest], np.zeros_like(mom[sel]), np.zeros_like(mom[sel])])
    # prune, on the grown set
    with np.errstate(invalid="ignore"):
        is_prune = f32(t["opacity"]) < F(th[3])
        if prune_big:
            is_prune = is_prune | (largest_scale(t["scaling"]) > F(th[2]))
    keep = ~is_prune
    return {k: v[keep] for k, v in t.items()}, (None if mom is None else mom[keep])


def row_multiset(tables, keys=None):
    """The rows of a dict of [M, ...] tables as a sorted list of byte strings: equal for two sets that hold the same rows in any order."""
    keys = sorted(tables) if keys is None else keys
    m = len(tables[keys[0]])
    flat = np.concatenate([np.ascontiguousarray(np.asarray(tables[k], dtype=np.float32)).reshape(m, -1) for k in keys], axis=1)
    return sorted(flat[i].tobytes() for i in range(m))
