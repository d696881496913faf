"""numpy reference of gwbp_pixel_gaussians' outputs, built from a view's contributing (gid, pix, w) triples -- oracle.blend_pairs' or
Engine.dump_pairs' -- and, for the median, the sorted tile lists of oracle.bin_sort.  No GPU."""
import numpy as np

MEDIAN_BAND = 1e-5  # a pixel is DECIDED when no T_j lies within this relative distance of one half


def lists(gid, pix, w, n_pixels, k):
    """(ids int32 [P, k], weights float32 [P, k], n_contrib int32 [P]): per pixel the k triples of largest weight, by weight
    descending, equal weights by Gaussian id ascending; empty slots -1 / 0; n_contrib counts every triple of the pixel."""
    gid, pix, w = np.asarray(gid, np.int64), np.asarray(pix, np.int64), np.asarray(w, np.float32)
    order = np.lexsort((gid, -w.astype(np.float64), pix))  # pixel, then weight descending, then id
    g, p, ws = gid[order], pix[order], w[order]
    counts = np.bincount(p, minlength=n_pixels)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rank = np.arange(p.shape[0]) - start[p]
    keep = rank < k
    ids = np.full((n_pixels, k), -1, np.int32)
    weights = np.zeros((n_pixels, k), np.float32)
    ids[p[keep], rank[keep]] = g[keep]
    weights[p[keep], rank[keep]] = ws[keep]
    return ids, weights, counts.astype(np.int32)


def list_positions(gid, pix, bins, n_gaussians, W, tile=16):
    """The position of every triple's Gaussian in the sorted list of its pixel's tile (bins: oracle.bin_sort's result)."""
    gid, pix = np.asarray(gid, np.int64), np.asarray(pix, np.int64)
    offs = np.asarray(bins["tile_offsets"], np.int64)
    flat = np.asarray(bins["flatten_ids"], np.int64)
    tile_of_isect = np.repeat(np.arange(offs.shape[0] - 1), np.diff(offs))
    keys = tile_of_isect * n_gaussians + flat  # (a tile lists a Gaussian once)
    by_key = np.argsort(keys, kind="stable")
    tile = (pix // W // tile) * bins["tile_w"] + (pix % W) // tile
    at = np.searchsorted(keys[by_key], tile * n_gaussians + gid)
    assert np.array_equal(keys[by_key][at], tile * n_gaussians + gid), "a triple whose Gaussian is not in its tile's list"
    return by_key[at]


def median(gid, pix, w, bins, n_gaussians, W, H, tile=16):
    """(median_id int32 [P], decided bool [P], T float64 [P]) from the float64 chain T_j = T_{j-1} - w_j over a pixel's triples in list
    order (w = alpha T_{j-1}, so this is T_{j-1} (1 - alpha)): median_id is the first triple after which T_j <= 0.5, -1 without one;
    decided: no T_j of the pixel lies within MEDIAN_BAND (relative) of 0.5, so fp32 rounding cannot move the median; T: the last T_j."""
    gid, pix, w = np.asarray(gid, np.int64), np.asarray(pix, np.int64), np.asarray(w, np.float32)
    n_pixels = W * H
    pos = list_positions(gid, pix, bins, n_gaussians, W, tile)
    order = np.lexsort((pos, pix))
    g, p, ws = gid[order], pix[order], w[order].astype(np.float64)
    csum = np.cumsum(ws)
    counts = np.bincount(p, minlength=n_pixels)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    base = np.concatenate([[0.0], csum])[start]  # the running sum in front of each pixel's first triple
    T = 1.0 - (csum - base[p])
    near = np.abs(T - 0.5) <= MEDIAN_BAND * 0.5
    decided = np.ones(n_pixels, bool)
    decided[p[near]] = False
    med = np.full(n_pixels, -1, np.int32)
    below = np.nonzero(T <= 0.5)[0]
    first = np.unique(p[below], return_index=True)  # p is sorted: the first index of each pixel's run
    med[first[0]] = g[below[first[1]]]
    T_last = np.ones(n_pixels)
    has = counts > 0
    T_last[has] = T[(start + counts - 1)[has]]
    return med, decided, T_last
