"""TEST SUPPORT: numpy restatements of the per-view votes of create_vote_field, on the CPU oracle's projection and (Gaussian,
pixel, w) pairs, and the literal per-pixel / per-Gaussian loops they are checked against."""
import numpy as np


def binary_votes(gid, pix, w, labels, K, N, weights=None):
    """One view's binary vote: C[g, k] = 1 if g has a pair (g, p) with w > 0 and L(p) == k, n[g] = 1 if it has any pair with w > 0.
    pix = y * W + x (oracle.blend_pairs); labels, weights: [H, W] arrays (weights: the pair's weight becomes w * c(p))."""
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    w = np.asarray(w, np.float32)
    if weights is not None:
        w = w * np.asarray(weights, np.float32).reshape(-1)[pix]
    keep = w > 0
    g, p = gid[keep].astype(np.int64), pix[keep]
    C, n = np.zeros((N, K), np.float64), np.zeros(N, np.float64)
    n[np.unique(g)] += 1
    lk = lab[p]
    ok = (lk >= 0) & (lk < K)
    C.reshape(-1)[np.unique(g[ok] * K + lk[ok])] += 1
    return C, n


def binary_votes_loop(gid, pix, w, labels, K, N):
    """binary_votes as a literal loop over the pairs."""
    lab = np.asarray(labels).reshape(-1)
    seen, hit = set(), set()
    for g, p, x in zip(gid.tolist(), pix.tolist(), w.tolist()):
        if x > 0:
            seen.add(g)
            if 0 <= int(lab[p]) < K:
                hit.add((g, int(lab[p])))
    C, n = np.zeros((N, K), np.float64), np.zeros(N, np.float64)
    for g in seen:
        n[g] += 1
    for g, k in hit:
        C[g, k] += 1
    return C, n


def projection_votes(means2d, radii, labels, K, weights=None):
    """One view's projection vote (get_mask3d's "projection" with np.round): a Gaussian with radius > 0 whose rounded centre lies
    in the image votes for the label there.  means2d [N, 2] float32, radii [N]; labels, weights: [H, W]."""
    labels = np.asarray(labels)
    H, W = labels.shape
    N = means2d.shape[0]
    r = np.round(np.asarray(means2d, np.float32))  # round half to even
    x, y = r[:, 0], r[:, 1]
    ok = (np.asarray(radii).reshape(N) > 0) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    gi = np.nonzero(ok)[0]
    xi, yi = x[gi].astype(np.int64), y[gi].astype(np.int64)
    if weights is not None:
        keep = np.asarray(weights, np.float32)[yi, xi] > 0
        gi, xi, yi = gi[keep], xi[keep], yi[keep]
    C, n = np.zeros((N, K), np.float64), np.zeros(N, np.float64)
    n[gi] += 1
    lk = labels[yi, xi].astype(np.int64)
    inr = (lk >= 0) & (lk < K)
    C[gi[inr], lk[inr]] += 1
    return C, n


def projection_votes_loop(means2d, radii, labels, K):
    """projection_votes as a literal loop over the Gaussians, rounding with Python's round() (also half to even)."""
    H, W = np.asarray(labels).shape
    N = means2d.shape[0]
    C, n = np.zeros((N, K), np.float64), np.zeros(N, np.float64)
    for g in range(N):
        if int(radii[g]) <= 0:
            continue
        x, y = round(float(means2d[g, 0])), round(float(means2d[g, 1]))
        if 0 <= x < W and 0 <= y < H:
            n[g] += 1
            k = int(labels[y][x])
            if 0 <= k < K:
                C[g, k] += 1
    return C, n


def oracle_view(orc, means, quats, scales, opac, vm, K, W, H):
    """(projection dict, gid, pix, w) of one view through the CPU oracle."""
    proj = orc.project(means, quats, scales, vm, K, W, H)
    bins = orc.bin_sort(proj, W, H)
    gid, pix, w, _ = orc.blend_pairs(proj, bins, opac, W, H)
    return proj, gid, pix, w
