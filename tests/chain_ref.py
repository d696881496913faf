"""TEST SUPPORT: the exact mirror of the MFMA kernels' documented arithmetic (numpy only, no GPU).

Every kernel that computes on v_mfma_f32_16x16x4_f32 states in its header that a product sum is ONE chain of fp32 fused
multiply-adds from +0, in an order that depends on the reduction length alone.  This module restates that sentence as code:

    fma32(a, b, c)        one correctly rounded fp32 fused multiply-add, vectorised
    chain(A, B, order)    acc = fma32(A[:, k], B[:, k], acc) for k in order, from +0: [rows(A), rows(B)]
    *_order(length)       the order each header documents, as a list of indices (a permutation of range(padded length))

so that a test can ask the kernel for EQUAL BITS instead of a rounding bound.  Indices at or beyond the true length enter as
products of zeros; they are not skipped, because the kernels execute those steps (fma(0, 0, -0) is +0).
"""
import numpy as np

F = np.float32


def _fma_product(p, c):
    """float32(p + c) rounded ONCE, for an exact float64 product p of two fp32 values and an fp32 c.

    The float64 sum s = p + c is rounded to 53 bits; rounding that to 24 bits again is wrong on halfway cases.  TwoSum gives the
    rounding error of s exactly; where it is non-zero and s's last bit is even, s moves one float64 ulp towards the true value
    (round-to-odd: the inexact s now has its sticky bit set, and 53 >= 24 + 2 bits make the second rounding the only one)."""
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)  # exact: |p|, |c| < 2^257, no overflow; NaN where s is not finite
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        if fix.any():
            s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays (broadcast), correctly rounded; infinities, NaN and signed zeros as IEEE 754 fma."""
    a, b, c = (np.asarray(v, F) for v in (a, b, c))
    with np.errstate(invalid="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)  # exact: 24 x 24 bits, exponents within float64's range
    return _fma_product(p, np.broadcast_to(c, np.broadcast(p, c).shape))


def chain(A, B, order):
    """[rows(A), rows(B)] float32: acc = fma32(A[:, k], B[:, k], acc) for k in order, starting from +0.  A [n, L] and B [m, L] are
    float32; an index k >= L contributes fma32(0, 0, acc)."""
    A, B = np.asarray(A, F), np.asarray(B, F)
    assert A.ndim == 2 and B.ndim == 2 and A.shape[1] == B.shape[1]
    order = [int(k) for k in order]
    L = max(order + [A.shape[1] - 1]) + 1
    A64, B64 = np.zeros((A.shape[0], L)), np.zeros((B.shape[0], L))
    A64[:, :A.shape[1]], B64[:, :B.shape[1]] = A, B
    A64, B64 = np.ascontiguousarray(A64.T), np.ascontiguousarray(B64.T)  # [L, rows]: a step reads two contiguous rows
    acc = np.zeros((A.shape[0], B.shape[0]), F)
    with np.errstate(invalid="ignore"):
        for k in order:
            acc = _fma_product(np.multiply.outer(A64[k], B64[k]), acc)
    return acc


# ---- the orders, each written from its kernel's header ---------------------------------------------------------------------------

def knn_order(D):
    """knn_tile.h (k_knn_search, k_kmeans_assign) and pca.hip's k_pca_project ("as knn.hip's scores"): k = 32 c + 16 b + 4 q + i
    in the order (c, b, i, q) -- chunk, 16-block, MFMA step, slot; columns D .. 32 ceil(D / 32) - 1 are zero-filled."""
    return [32 * c + 16 * b + 4 * q + i for c in range(-(-D // 32)) for b in range(2) for i in range(4) for q in range(4)]


def prompt_order(D):
    """query.hip (k_prompt_scores): the dot products and the sum of squares consume k = 32 c + 16 b + 4 q + i in the order
    (c, b, i, q) -- the 32-column chunk staged per step, its two 16-column blocks, the float4 component, the quarter wave."""
    return [32 * c + 16 * b + 4 * q + i for c in range(-(-D // 32)) for b in range(2) for i in range(4) for q in range(4)]


def encode_order(K):
    """encode.hip (k_encode_map): k = 16 j + 4 q + i in the order (j, i, q); K % 16 == 0, nothing is padded."""
    assert K % 16 == 0
    return [16 * j + 4 * q + i for j in range(K // 16) for i in range(4) for q in range(4)]


def decode_y_order(d):
    """decode_loss.hip, y over k: for b, for s: k = 16 b + s, 16 b + 4 + s, 16 b + 8 + s, 16 b + 12 + s; d % 16 == 0."""
    assert d % 16 == 0
    return [16 * b + 4 * q + s for b in range(d // 16) for s in range(4) for q in range(4)]


def decode_gr_order(D):
    """decode_loss.hip, GR over j: chunks of 64 ascending, inside a chunk for t, for r: j = 64 c + 16 t + r + 0, 4, 8, 12; the
    16-column tiles at or beyond D are not executed (D % 16 == 0: the chain has length D)."""
    assert D % 16 == 0
    return [64 * c + 16 * t + 4 * q + r for c in range(-(-D // 64)) for t in range(min(4, (D - 64 * c) // 16)) for r in range(4)
            for q in range(4)]


def decode_gc_order(rows):
    """decode_loss.hip, GC over a slice's pixels: 64-pixel blocks ascending, inside a block for u, for r: pixel 16 u + r + 0, 4, 8,
    12.  rows: the slice's pixel count; the last block is executed whole (pixels beyond the image are zero rows with g = 0)."""
    return [64 * blk + 16 * u + 4 * q + r for blk in range(-(-rows // 64)) for u in range(4) for r in range(4) for q in range(4)]


DECODE_MAX_SLICES = 512  # GWBP_DECODE_MAX_SLICES


def decode_slices(P):
    """The slice plan of include/gwbp.h, a function of P alone: 64-pixel blocks, ceil(blocks / 512) blocks per slice.  Returns the
    (first pixel, end pixel) of every slice, the end clipped to P."""
    nb = -(-P // 64)
    bps = max(1, -(-nb // DECODE_MAX_SLICES))
    return [(s * bps * 64, min(P, (s + 1) * bps * 64)) for s in range(-(-nb // bps))]


# ---- whole operations built from the chains -----------------------------------------------------------------------------------------

def topk(sc, k):
    """(idx [N, k] int64, score [N, k] float32) of a score matrix by (score desc, index asc); -0 counts as +0 and is returned as +0
    (knn.hip's ORDER; finite or infinite scores, no NaN)."""
    sc = np.asarray(sc, F) + F(0.0)
    idx = np.argsort(-sc.astype(np.float64), axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(sc, idx, axis=1)


def assign(sc, bias=None):
    """(label [N] int64, best [N] float32) of cluster.hip's k_kmeans_assign from the chain's scores: ONE fp32 addition of bias[j],
    the argmax with ties to the lowest index, -0 as +0; a row whose scores are all NaN gets -1 and NaN."""
    s = np.asarray(sc, F)
    if bias is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            s = (s + np.asarray(bias, F)[None, :]).astype(F)
    nan = np.isnan(s)
    label = np.where(nan, -np.inf, s.astype(np.float64)).argmax(axis=1)
    best = np.take_along_axis(s, label[:, None], axis=1)[:, 0] + F(0.0)
    none = nan.all(axis=1)
    return np.where(none, -1, label), np.where(none, F(np.nan), best).astype(F)


def prompt_scores(X, prompts, normalize=True):
    """query.hip's scores [N, P]: the dot chains, and with normalize one fp32 sqrt of the sum-of-squares chain (same order) and one
    fp32 divide by max(norm, 1e-12)."""
    X, prompts = np.asarray(X, F), np.asarray(prompts, F)
    order = prompt_order(X.shape[1])
    dots = chain(X, prompts, order)
    if not normalize:
        return dots
    ss = np.zeros(X.shape[0], F)
    for k in order:
        col = X[:, k] if k < X.shape[1] else np.zeros(X.shape[0], F)
        ss = fma32(col, col, ss)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        den = np.maximum(np.sqrt(ss), F(1e-12))
        return (dots / den[:, None]).astype(F)


def prompt_mask(scores, n_pos, threshold=None):
    """query.hip's mask rule on finite scores: max of the first n_pos > max of the others (no others: True), and scores[:, 0] >
    float32(threshold)."""
    scores = np.asarray(scores, F)
    mask = scores[:, :n_pos].max(axis=1) > scores[:, n_pos:].max(axis=1) if n_pos < scores.shape[1] else np.ones(len(scores), bool)
    if threshold is not None:
        mask = mask & (scores[:, 0] > F(threshold))
    return mask


def pca_project(X, mean, V):
    """pca.hip's k_pca_project: Y [N, k] = the chain over c of fl(X[g, c] - mean[c]) against V[j, c], knn_order(D)."""
    X, mean, V = np.asarray(X, F), np.asarray(mean, F), np.asarray(V, F)
    return chain((X - mean[None, :]).astype(F), V, knn_order(X.shape[1]))


def decode_loss(R, C, M, loss, scale, weights=None):
    """decode_loss.hip's (GR [P, d], GC [d, D]) float32 for R [P, d], C [d, D], M [P, D] float32, weights [P] float32 or None: y by
    decode_y_order, e = y - m, w_p = fl(s c_p), g = w (e + e) | w sign(e) with sign(0) = 0, GR a chain over j, GC per-slice
    chains over the pixels added in ascending slice order in float64 and rounded once.  A pixel whose map row holds a non-finite
    value has g = 0 (it still passes through GC's chain as a product with zero) and a zero GR row."""
    R, C, M = np.asarray(R, F), np.asarray(C, F), np.asarray(M, F)
    P, d = R.shape
    D = C.shape[1]
    bad = ~np.isfinite(M).all(axis=1)
    y = chain(R, C.T, decode_y_order(d))
    with np.errstate(invalid="ignore", over="ignore"):
        e = (y - M).astype(F)
        w = np.full(P, F(scale), F) if weights is None else (F(scale) * np.asarray(weights, F)).astype(F)
        g = (w[:, None] * (e + e).astype(F)).astype(F) if loss == "l2" else (w[:, None] * np.sign(e)).astype(F)
    g[bad] = 0.0
    GR = chain(g, C, decode_gr_order(D))
    GR[bad] = 0.0
    GC = np.zeros((d, D), np.float64)
    for p0, p1 in decode_slices(P):
        GC += chain(R[p0:p1].T, g[p0:p1].T, decode_gc_order(p1 - p0)).astype(np.float64)
    return GR, GC.astype(F)
