"""Scenes that sit ON the size boundaries of the front stage (gwbp_project -> gwbp_bin_sort -> a blend), and their CPU-oracle results.

The geometry is plain: an identity view matrix (depth == z bit for bit), identity quaternions, Gaussians placed by the pixel their
centre projects to, with a footprint of a few pixels and a z-scale of 1e-7 (a larger one is smeared over hundreds of tiles by the pinhole
Jacobian on the very wide images).  What is chosen are COUNTS: tiles (the 1 / 2 / 3 byte-passes of the tile sort), Gaussians with tied
depths around the depth sort's path boundaries, and intersection counts on the boundaries of a 4096-key sort block.  A scene only tests its
boundary if it sits on it: tests/test_front_boundaries_cpu.py asserts every condition on the oracle alone, and the GPU tests assert them
again before they compare anything.

Every builder is deterministic from its arguments and returns a dict of numpy inputs: means, quats, scales, opac, viewmat, K, W, H.
"""
import functools

import numpy as np

from oracle import oracle as orc

TILE = 16
SORT_BLOCK = 4096       # keys per block of the radix passes (sort.hip kSortItems)
ORDER_CLAMP = 4092      # k_tile_order: lists longer than this share its last bucket (len >> 2 clamped to 1023)
SMALL_SORT = (4096, 8192, 12288)  # k_sort_small<4>, <8>, <12> take N up to these; above: the multi-block radix passes


def sort_passes(n_tiles):
    """8-bit passes of the tile sort (gwbp_dev.h sort_passes)."""
    bits = 1
    while (1 << bits) < n_tiles:
        bits += 1
    return (bits + 7) // 8


def n_tiles(W, H):
    return -(-W // TILE) * -(-H // TILE)


def _place(u, v, z, sig_x, sig_y, opac, W, H):
    """Gaussians whose centres project to pixel (u, v) at depth z with a footprint of (sig_x, sig_y) pixels (before the 0.3 blur)."""
    fx, fy, cx, cy = W / 2.0, H / 2.0, W / 2.0, H / 2.0
    u, v, z = (np.asarray(t, np.float64) for t in (u, v, z))
    az = np.abs(z)
    means = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    scales = np.stack([sig_x * az / fx, sig_y * az / fy, np.full_like(az, 1e-7)], axis=1)
    n = means.shape[0]
    quats = np.zeros((n, 4), np.float32)
    quats[:, 0] = 1.0
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
    return dict(means=means.astype(np.float32), quats=quats, scales=scales.astype(np.float32),
                opac=np.asarray(opac, np.float32), viewmat=np.eye(4, dtype=np.float32), K=K, W=int(W), H=int(H))


# ---- 1. tile counts ----------------------------------------------------------------------------------------------------------------------
# name -> (W, H, Gaussians).  Seventeen rows: the second tile row costs one pixel row.  The width of the 3-pass image is such that
# thousands of tiles have an id >= 65 536 (2 x 32 769 tiles would have two).
TILE_SCENES = {
    "t1": (16, 16, 300),
    "t256": (256, 256, 600),
    "t272": (272, 256, 600),
    "t65536": (524288, 17, 2000),
    "t80000": (640000, 17, 2000),
}
TILE_PASSES = {"t1": 1, "t256": 1, "t272": 2, "t65536": 2, "t80000": 3}
PAIRED = 300          # t80000: Gaussians forced into the left 14 000 tile columns, each with a partner 65 536 tile ids further on
PAIR_COLUMNS = 14000
LOW_IDS = 40          # ... of which this many lie in the first 256 tile columns (ids < 256)


@functools.lru_cache(maxsize=None)
def tile_scene(name):
    W, H, n = TILE_SCENES[name]
    rng = np.random.default_rng(1000 + n_tiles(W, H))
    u = rng.uniform(0, W, n)
    two_rows = H == 17
    v = rng.uniform(6, H, n) if two_rows else rng.uniform(0, H, n)
    sig_x = rng.uniform(1.0, 4.0, n)
    sig_y = rng.uniform(3.0, 6.0, n) if two_rows else rng.uniform(1.0, 4.0, n)
    z = rng.choice(np.array([1.0, 1.5, 2.0]), n)
    opac = rng.uniform(0.1, 0.9, n)
    if name == "t80000":
        # tile t of row 0, column c, and tile t + 65 536 = row 1, column c + 65 536 - tile_w differ in the third byte of the id only
        tile_w = W // TILE
        shift = 65536 - tile_w
        col = rng.choice(PAIR_COLUMNS, PAIRED, replace=False)
        col[:LOW_IDS] = rng.choice(256, LOW_IDS, replace=False)
        u[:PAIRED] = TILE * col + 8.0
        u[PAIRED:2 * PAIRED] = TILE * (col + shift) + 8.0
        v[:2 * PAIRED] = 14.0          # 3 sigma >= 9 pixels: both tile rows
    return _place(u, v, z, sig_x, sig_y, opac, W, H)


# ---- 2. depth ties -----------------------------------------------------------------------------------------------------------------------
TIE_COUNTS = (1, 64, 4096, 4097, 8192, 8193, 12288, 12289, 16384, 16385, 20481)
TIE_IMAGE = (64, 48)  # 4 x 3 tiles
# (n, image, depth values): every count on the small image, N = 12 289 also in ONE tile and on two tiles of which one holds nearly all
TIE_CASES = [(n, "small", 3) for n in TIE_COUNTS] + [(4097, "small", 1), (12289, "one_tile", 3), (12289, "crowded", 3)]
TIE_IDS = [f"N{n}-{img}-{k}depths" for n, img, k in TIE_CASES]
LONG_LIST_CASES = [(12289, "one_tile", 3), (12289, "crowded", 3)]


@functools.lru_cache(maxsize=None)
def tie_scene(n, image="small", n_depths=3):
    """Depths from a set of n_depths values; every fifth Gaussian (index % 5 == 1) lies behind the camera and must sort last."""
    rng = np.random.default_rng(7 * n + n_depths)
    W, H = {"small": TIE_IMAGE, "one_tile": (16, 16), "crowded": (32, 16)}[image]
    z = rng.choice(np.array([1.0, 1.5, 2.0])[:n_depths], n)
    z[np.arange(n) % 5 == 1] *= -1.0
    if image == "crowded":   # 3 sigma <= 3 pixels around u in [4, 11]: tile 0 only; every 997th Gaussian in tile 1 only
        u, v, sig = rng.uniform(4, 11, n), rng.uniform(4, 11, n), rng.uniform(0.3, 0.8, n)
        u[np.arange(n) % 997 == 0] += 16.0
    else:
        u, v, sig = rng.uniform(0, W, n), rng.uniform(0, H, n), rng.uniform(0.8, 2.0, n)
    opac = rng.uniform(0.005, 0.02, n)  # (the blend does not terminate at once)
    return _place(u, v, z, sig, sig, opac, W, H)


def depth_order_keys(proj):
    """The depth sort's keys in its result order: depth bits of the visible Gaussians ascending (stable), the culled ones last."""
    vis = proj["radii"] > 0
    keys = np.where(vis, proj["depths"].view(np.uint32), np.uint32(0xFFFFFFFF)).astype(np.uint64)
    return keys[np.argsort(keys, kind="stable")]


# ---- 3. intersection counts on a sort-block boundary ---------------------------------------------------------------------------------------
BLOCK_BASE = (160, 112, 24000)  # 10 x 7 tiles
BLOCK_TARGETS = (1, 4095, 4096, 4097, 8192, 28672)  # 28 672 = 7 full blocks, from more than 12 288 Gaussians (multi-block depth sort)
BIG_TARGET = 28672


@functools.lru_cache(maxsize=None)
def block_base():
    W, H, n = BLOCK_BASE
    rng = np.random.default_rng(31)
    z = rng.uniform(0.8, 3.0, n)
    z[rng.uniform(size=n) < 0.1] *= -1.0
    sig = rng.uniform(0.3, 2.5, n)
    return _place(rng.uniform(0, W, n), rng.uniform(0, H, n), z, sig, sig, rng.uniform(0.05, 0.9, n), W, H)


def subset(sc, idx):
    out = {k: sc[k] for k in ("viewmat", "K", "W", "H")}
    for k in ("means", "quats", "scales", "opac"):
        out[k] = np.ascontiguousarray(sc[k][idx])
    return out


@functools.lru_cache(maxsize=None)
def block_scene(target):
    """A subset of block_base() whose n_isect is exactly `target`: a prefix of the Gaussians, then single-tile fill-ins."""
    base = block_base()
    counts = np.bincount(front(base)[1]["flatten_ids"], minlength=base["means"].shape[0])
    cum = np.cumsum(counts)
    k = int(np.searchsorted(cum, target, side="right"))
    rest = target - (int(cum[k - 1]) if k else 0)
    singles = k + 1 + np.nonzero(counts[k + 1:] == 1)[0][:rest]
    assert len(singles) == rest, "the base scene has too few single-tile Gaussians"
    return subset(base, np.concatenate([np.arange(k), singles]))


# ---- the oracle's results (shared: nobody writes into them) --------------------------------------------------------------------------------
def front(sc):
    """(proj, bins) of the oracle, kept with the scene."""
    if "_front" not in sc:
        proj = orc.project(sc["means"], sc["quats"], sc["scales"], sc["viewmat"], sc["K"], sc["W"], sc["H"])
        sc["_front"] = (proj, orc.bin_sort(proj, sc["W"], sc["H"]))
    return sc["_front"]


def pairs(sc):
    """(sorted pair keys, their weights, alphas [H, W]) of the oracle's blend, kept with the scene."""
    if "_pairs" not in sc:
        proj, bins = front(sc)
        g, p, w, alphas = orc.blend_pairs(proj, bins, sc["opac"], sc["W"], sc["H"], want_alphas=True)
        k = g.astype(np.int64) * (1 << 32) + p.astype(np.int64)
        o = np.argsort(k, kind="stable")
        sc["_pairs"] = (k[o], w[o], alphas)
    return sc["_pairs"]


def list_lengths(bins):
    return np.diff(bins["tile_offsets"].astype(np.int64))


# ---- the conditions, asserted by the CPU test and again by the GPU tests -------------------------------------------------------------------
def check_tile_scene(name):
    sc = tile_scene(name)
    proj, bins = front(sc)
    nt = n_tiles(sc["W"], sc["H"])
    assert nt == bins["tile_w"] * bins["tile_h"] and sort_passes(nt) == TILE_PASSES[name], (name, nt)
    lens = list_lengths(bins)
    filled = np.nonzero(lens)[0]
    assert bins["n_isect"] >= 300 and int((proj["radii"] > 0).sum()) >= 0.9 * sc["means"].shape[0]
    facts = dict(tiles=nt, n_isect=bins["n_isect"], filled=len(filled))
    if nt > 1:
        assert filled.min() < 256 and filled.max() >= nt - nt // 4, "the lists do not spread over the tile ids"
    if name == "t65536":
        assert nt == 65536 and filled.max() >= 65000  # (ids that need all sixteen bits)
    if name == "t80000":
        high = filled[filled >= 65536]
        twins = np.intersect1d(filled, high - 65536)
        both_rows = int(((proj["rect"][:, 3] - proj["rect"][:, 1]) == 2).sum())
        facts.update(high=len(high), twins=len(twins), low=int((filled < 256).sum()), both_rows=both_rows)
        assert len(high) >= 1000, facts
        assert len(twins) >= 100, facts
        assert facts["low"] >= 1, facts
        assert both_rows >= 1000, facts
    return facts


def check_tie_scene(n, image, n_depths):
    sc = tie_scene(n, image, n_depths)
    proj, bins = front(sc)
    vis = proj["radii"] > 0
    behind = np.arange(n) % 5 == 1
    assert not vis[behind].any() and (n < 5 or vis.sum() >= n // 2)
    assert np.array_equal(proj["depths"][vis], sc["means"][vis, 2])  # identity view: depth == z bit for bit
    assert len(np.unique(proj["depths"][vis])) <= 3
    keys = depth_order_keys(proj)
    blocks = [keys[i:i + SORT_BLOCK] for i in range(0, n, SORT_BLOCK)]
    if n > 1:
        assert all(len(b) == 1 or len(np.unique(b)) < len(b) for b in blocks), "a block of the depth order without ties"
    straddle = [int(keys[i - 1] == keys[i]) for i in range(SORT_BLOCK, n, SORT_BLOCK)]
    assert all(straddle), "a block boundary of the depth order falls between two different keys"
    longest = int(list_lengths(bins).max())
    if (n, image, n_depths) in LONG_LIST_CASES:
        assert longest > ORDER_CLAMP, longest
        if image == "crowded":
            lens = list_lengths(bins)
            assert len(lens) == 2 and 0 < lens[1] <= 20 and lens[0] > ORDER_CLAMP, lens
    return dict(visible=int(vis.sum()), n_isect=bins["n_isect"], longest=longest)


def check_block_scene(target):
    sc = block_scene(target)
    _, bins = front(sc)
    n = sc["means"].shape[0]
    assert bins["n_isect"] == target, (bins["n_isect"], target)
    if target == BIG_TARGET:
        assert n > SMALL_SORT[-1], n
    else:
        assert n <= SMALL_SORT[-1], n
    return dict(n=n, n_isect=bins["n_isect"])
