"""References for the point samples (csrc/sample.hip, gsbp_amd.sample): the contract of include/gwbp.h restated in numpy, every fused
multiply-add through chain_ref.fma32, every other operation one float32 numpy operation (correctly rounded).  Brute force: the weights
are computed for every (query, candidate) pair with d2 <= r2, no grid.

    exp_neg(x)                           gwbp_dev.h's deterministic exp(x), x <= 0
    pack(means, quats, scales, o, live)  (M [N, 3, 3], o [N], live [N])
    pair_weights(points, means, M, o)    (sigma, w) of given (query, Gaussian) index pairs
    point_gaussians(...)                 (idx [Q, k] int32, w [Q, k] float32, n_contrib [Q] int32)
    blend(idx, w, F)                     (out [Q, D], wsum [Q])
    vote(idx, w, labels, K)              (label [Q] int32, share [Q] float32)
"""
import numpy as np

from chain_ref import fma32
from spatial_ref import d2_f32, finite_rows

F = np.float32
ALPHA_MIN = F(1.0) / F(255.0)  # 0x1.010102p-8f, the blend's kAlphaMin


def f32(x):
    return np.asarray(x, F)


def exp_neg(x):
    """exp_neg(x) of gwbp_dev.h for float32 x <= 0 (clamped at -80): ln 2 hi / lo range reduction, degree-7 Horner, exponent added to
    the bit pattern."""
    x = np.maximum(f32(x), F(-80.0))
    t = (x * F(float.fromhex("0x1.715476p+0"))).astype(F)
    n = np.rint(t).astype(F)
    r = fma32(n, F(float.fromhex("-0x1.62e4p-1")), x)
    r = fma32(n, F(float.fromhex("-0x1.7f7d1cp-20")), r)
    p = np.full(r.shape, F(float.fromhex("0x1.a01a02p-13")), F)
    for c in ("0x1.6c16c2p-10", "0x1.111112p-7", "0x1.555556p-5", "0x1.555556p-3", "0x1p-1", "0x1p0", "0x1p0"):
        p = fma32(p, r, F(float.fromhex(c)))
    return (p.view(np.int32) + (n.astype(np.int32) << 23)).view(F)


def pack(means, quats, scales, opacities, live=None):
    """(M [N, 3, 3] float32 with M[a][b] = R[b][a] / s[a], o [N] float32, live [N] bool); a dead Gaussian has M = 0 and o = 0."""
    mu, q, s, o = f32(means), f32(quats), f32(scales), f32(opacities)
    n = mu.shape[0]
    with np.errstate(all="ignore"):
        n2 = fma32(q[:, 3], q[:, 3], fma32(q[:, 2], q[:, 2], fma32(q[:, 1], q[:, 1], (q[:, 0] * q[:, 0]).astype(F))))
        ok = finite_rows(mu) & finite_rows(q) & (n2 > 0) & np.isfinite(n2) & finite_rows(s) & (s > 0).all(axis=1) & np.isfinite(o) & (o > 0)
        if live is not None:
            ok &= np.asarray(live) != 0
        inv = (F(1.0) / np.sqrt(n2).astype(F)).astype(F)
        w, x, y, z = ((q[:, c] * inv).astype(F) for c in range(4))
        x2, y2, z2, xy, xz, yz = x * x, y * y, z * z, x * y, x * z, y * z
        wx, wy, wz = w * x, w * y, w * z
        one, two = F(1.0), F(2.0)
        R = np.empty((n, 3, 3), F)
        R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = one - two * (y2 + z2), two * (xy - wz), two * (xz + wy)
        R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = two * (xy + wz), one - two * (x2 + z2), two * (yz - wx)
        R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = two * (xz - wy), two * (yz + wx), one - two * (x2 + y2)
        M = (R.transpose(0, 2, 1) / s[:, :, None]).astype(F)
    M[~ok] = 0.0
    return M, np.where(ok, o, F(0.0)).astype(F), ok


def pair_weights(points, means, M, o, qi, gi):
    """(sigma, w) float32 of the pairs (query qi[e], Gaussian gi[e]): the contract's weight before the keep rule."""
    with np.errstate(all="ignore"):
        d = (f32(points)[qi] - f32(means)[gi]).astype(F)
        m = M[gi]
        u = [fma32(m[:, a, 2], d[:, 2], fma32(m[:, a, 1], d[:, 1], (m[:, a, 0] * d[:, 0]).astype(F))) for a in range(3)]
        m2 = fma32(u[2], u[2], fma32(u[1], u[1], (u[0] * u[0]).astype(F)))
        sigma = (F(0.5) * m2).astype(F)
        w = (o[gi] * exp_neg(-sigma)).astype(F)
    return sigma, w


def kept(sigma, w, alpha_min=ALPHA_MIN):
    with np.errstate(invalid="ignore"):
        return (sigma <= F(80.0)) & (w >= F(alpha_min))


def candidate_pairs(points, means, r2, rows=256):
    """(qi, gi): the pairs with a finite query, a finite mean and d2 <= r2, ascending in (qi, gi)."""
    p, mu = f32(points), f32(means)
    okq, okg = finite_rows(p), finite_rows(mu)
    qs, gs = [], []
    for a in range(0, p.shape[0], rows):
        with np.errstate(all="ignore"):
            d2 = d2_f32(mu[None, :, :], p[a:a + rows, None, :])
            hit = (d2 <= F(r2)) & okq[a:a + rows, None] & okg[None, :]
        qi, gi = np.nonzero(hit)
        qs.append(qi + a)
        gs.append(gi)
    return np.concatenate(qs) if qs else np.zeros(0, np.int64), np.concatenate(gs) if gs else np.zeros(0, np.int64)


def point_gaussians(points, means, quats, scales, opacities, k, r2, alpha_min=ALPHA_MIN, live=None, packed=None):
    """(idx int32 [Q, k] tail -1, w float32 [Q, k] tail 0, n_contrib int32 [Q]) by brute force."""
    nq = np.asarray(points).shape[0]
    M, o, _ = packed if packed is not None else pack(means, quats, scales, opacities, live)
    qi, gi = candidate_pairs(points, means, r2)
    sigma, w = pair_weights(points, means, M, o, qi, gi)
    keep = kept(sigma, w, alpha_min)
    qi, gi, w = qi[keep], gi[keep], w[keep]
    idx = np.full((nq, k), -1, np.int32)
    out = np.zeros((nq, k), F)
    n_contrib = np.bincount(qi, minlength=nq).astype(np.int32)
    order = np.lexsort((gi, -w.astype(np.float64), qi))  # by query, then weight descending, then index ascending
    qi, gi, w = qi[order], gi[order], w[order]
    start = np.searchsorted(qi, np.arange(nq))
    rank = np.arange(qi.shape[0]) - start[qi]
    top = rank < k
    idx[qi[top], rank[top]] = gi[top]
    out[qi[top], rank[top]] = w[top]
    return idx, out, n_contrib


def _taking_part(idx, w, m):
    idx, w = np.asarray(idx), f32(w)
    return (idx >= 0) & (idx < m) & (w != 0)


def blend(idx, w, feats):
    """(out float32 [Q, D], wsum float32 [Q]) of gwbp_neighbor_blend."""
    idx, w, feats = np.asarray(idx), f32(w), f32(feats)
    nq, k = idx.shape
    m, d = feats.shape
    ok = _taking_part(idx, w, m)
    W = np.zeros(nq, F)
    acc = np.zeros((nq, d), F)
    with np.errstate(all="ignore"):
        for j in range(k):
            on = ok[:, j]
            rows = feats[np.where(on, idx[:, j], 0)]
            W = np.where(on, (w[:, j] + W).astype(F), W)
            acc = np.where(on[:, None], fma32(w[:, j, None], rows, acc), acc)
        any_ = ok.any(axis=1)
        out = np.where(any_[:, None], (acc / W[:, None]).astype(F), F(0.0)).astype(F)
    return out, W


def vote(idx, w, labels, num_classes):
    """(label int32 [Q], share float32 [Q]) of gwbp_weighted_vote."""
    idx, w, labels = np.asarray(idx), f32(w), np.asarray(labels)
    nq, k = idx.shape
    ok = _taking_part(idx, w, labels.shape[0])
    lab = np.where(ok, labels[np.where(ok, idx, 0)], -1)
    lab = np.where((lab >= 0) & (lab < num_classes), lab, -1)
    out_label, share = np.full(nq, -1, np.int32), np.zeros(nq, F)
    for g in range(nq):
        total, sums = F(0.0), {}
        for j in range(k):
            c = int(lab[g, j])
            if c < 0:
                continue
            total = F(w[g, j] + total)
            sums[c] = F(w[g, j] + sums.get(c, F(0.0)))
        if sums:
            best = min(sums, key=lambda c: (-float(sums[c]), c))
            with np.errstate(all="ignore"):
                out_label[g], share[g] = best, F(sums[best] / total)
    return out_label, share


def same_bits(a, b):
    a, b = f32(a), f32(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
