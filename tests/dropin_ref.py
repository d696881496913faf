"""Test-only references for the options of the drop-in `rasterization()` that its defaults never reach: clip planes and
radius_clip that are guaranteed to bite, gsplat 1.4.0's packed=True meta written out from per-camera oracle results, and a
float64 spherical-harmonics colour with a derived fp32 rounding bound.  numpy (float64 where arithmetic is involved); shared
by tests/test_dropin_options_cpu.py and tests/test_gpu_dropin_options.py."""
import numpy as np
import torch

import ref_sh

U = 2.0 ** -24  # unit roundoff of fp32


def f32(x) -> float:
    """A Python float that holds exactly the fp32 value (what a c_float argument receives)."""
    return float(np.float32(x))


# ---- clip options that bite --------------------------------------------------------------------------------------------------------
def _widest_midpoint(all_depths: np.ndarray, target: float, window: int = 64):
    """The fp32 midpoint of the widest gap between two consecutive distinct depths among the `window` gaps around `target`:
    no Gaussian sits on it, and the nearest one is as far away as the scene allows."""
    z = np.unique(np.asarray(all_depths, np.float32))
    i = int(np.searchsorted(z, np.float32(target)))
    lo, hi = max(0, i - window // 2), min(len(z) - 1, i + window // 2)
    assert hi > lo, "fewer than two distinct depths"
    gaps = z[lo + 1:hi + 1].astype(np.float64) - z[lo:hi].astype(np.float64)
    j = lo + int(np.argmax(gaps))
    mid = np.float32(0.5 * (float(z[j]) + float(z[j + 1])))
    assert z[j] < mid < z[j + 1]
    return float(mid)


def clip_parameters(proj_default, all_depths=None):
    """From the oracle's default-parameter projection of a view: clip values that cut through the visible Gaussians.
    near = the median depth among the visible, far = the 75th-percentile depth, radius_clip = the median visible radius -- all
    values that OCCUR (Gaussians sit exactly on each cut); near_between / far_between = midpoints of two consecutive distinct
    sorted depths next to them (no Gaussian on a cut: a float64 reference decides every Gaussian alike).  all_depths: the camera
    depths of EVERY Gaussian (the between cuts then also keep clear of the ones the default projection culls)."""
    vis = proj_default["radii"] > 0
    z = np.sort(proj_default["depths"][vis])
    r = np.sort(proj_default["radii"][vis])
    assert z.size >= 8, "too few visible Gaussians to cut through"
    near, far = z[z.size // 2], z[(3 * z.size) // 4]
    assert z[0] < near < far < z[-1]
    pool = z if all_depths is None else np.asarray(all_depths, np.float32)
    return dict(near=float(near), far=float(far), radius_clip=float(r[r.size // 2]),
                near_between=_widest_midpoint(pool, near), far_between=_widest_midpoint(pool, far))


def exact_cut_scene():
    """A camera-space scene (identity view matrix: the camera depth of Gaussian i is means[i, 2] exactly) of 300 Gaussians, all
    on screen, whose depths sit exactly on near and on far, and one ulp to either side of each.  Returns the scene and `roles`,
    index arrays by name: on_near, below_near, above_near, on_far, above_far, below_far."""
    rng = np.random.default_rng(17)
    n, W, H = 300, 96, 64
    f = 1.2 * W
    near, far = np.float32(2.7182817), np.float32(4.6692014)
    z = rng.uniform(2.0, 6.0, n).astype(np.float32)
    roles = {k: np.arange(4 * i, 4 * i + 4) for i, k in enumerate(("on_near", "below_near", "above_near", "on_far", "above_far",
                                                                   "below_far"))}
    # (the last of each group lies past the first 256-thread block)
    for k in roles:
        roles[k][3] = 260 + roles[k][0] // 4
    z[roles["on_near"]] = near
    z[roles["below_near"]] = np.nextafter(near, np.float32(0))
    z[roles["above_near"]] = np.nextafter(near, np.float32(np.inf))
    z[roles["on_far"]] = far
    z[roles["above_far"]] = np.nextafter(far, np.float32(np.inf))
    z[roles["below_far"]] = np.nextafter(far, np.float32(0))
    means = np.stack([rng.uniform(-0.3, 0.3, n) * z, rng.uniform(-0.2, 0.2, n) * z, z], 1).astype(np.float32)
    assert np.array_equal(means[:, 2], z)
    quats = rng.standard_normal((n, 4)).astype(np.float32)
    scales = np.exp(np.log(0.05) + 0.3 * rng.standard_normal((n, 3))).astype(np.float32)
    opac = rng.uniform(0.2, 0.9, n).astype(np.float32)
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
    return dict(means=means, quats=quats, scales=scales, opac=opac, viewmat=np.eye(4, dtype=np.float32), K=K, W=W, H=H,
                near=float(near), far=float(far), roles=roles)


# ---- gsplat 1.4.0's packed meta ---------------------------------------------------------------------------------------------------
def packed_meta(per_camera, opacities=None, width=None, height=None):
    """The meta dict of gsplat 1.4.0 `rasterization(packed=True)` for C cameras, from per-camera oracle results
    [{"proj": orc.project(...), "bins": orc.bin_sort(...)}, ...]:
      camera_ids, gaussian_ids  the visible (camera, Gaussian) pairs, camera-major, Gaussians ascending      [nnz]
      radii, means2d, depths, conics (and opacities, when given)  gathered at those pairs                     [nnz, ...]
      tiles_per_gauss           the area of the tile rectangle of each pair                                   [nnz]
      isect_ids                 camera << (32 + tile_n_bits) | tile << 32 | depth bits, tile_n_bits = floor(log2(n_tiles)) + 1
      flatten_ids               the ROW of the packed arrays each intersection belongs to                     [n_isects]
      isect_offsets             [C, tile_height, tile_width] start of every tile's run in the concatenated list."""
    C = len(per_camera)
    tw, th = int(per_camera[0]["bins"]["tile_w"]), int(per_camera[0]["bins"]["tile_h"])
    n_tiles = tw * th
    tile_n_bits = 0
    while (1 << tile_n_bits) <= n_tiles:  # floor(log2(n_tiles)) + 1
        tile_n_bits += 1
    cams, gids, isect, flat, offs, tpg = [], [], [], [], [], []
    parts = {k: [] for k in ("radii", "means2d", "depths", "conics")}
    rows, n_isect = 0, 0
    for c, res in enumerate(per_camera):
        p, b = res["proj"], res["bins"]
        vis = np.nonzero(p["radii"] > 0)[0].astype(np.int64)
        cams.append(np.full(vis.size, c, np.int64))
        gids.append(vis)
        for k in parts:
            parts[k].append(p[k][vis])
        rect = p["rect"][vis].astype(np.int64)
        tpg.append(((rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])).astype(np.int32))
        row_of = np.full(p["radii"].shape[0], -1, np.int64)
        row_of[vis] = rows + np.arange(vis.size)
        ids = b["isect_ids"].astype(np.uint64)
        tile, depth_bits = ids >> np.uint64(32), ids & np.uint64(0xFFFFFFFF)
        assert int(tile.max(initial=0)) < n_tiles
        isect.append(((np.uint64(c) << np.uint64(32 + tile_n_bits)) | (tile << np.uint64(32)) | depth_bits).astype(np.int64))
        f = row_of[b["flatten_ids"].astype(np.int64)]
        assert (f >= 0).all(), "an intersection of a culled Gaussian"
        flat.append(f.astype(np.int32))
        offs.append(b["tile_offsets"][:-1].astype(np.int64) + n_isect)
        rows += vis.size
        n_isect += int(b["isect_ids"].shape[0])
    out = dict(camera_ids=np.concatenate(cams), gaussian_ids=np.concatenate(gids), tiles_per_gauss=np.concatenate(tpg),
               isect_ids=np.concatenate(isect), flatten_ids=np.concatenate(flat),
               isect_offsets=np.stack(offs).reshape(C, th, tw).astype(np.int32),
               tile_width=tw, tile_height=th, tile_size=16, n_cameras=C)
    for k in parts:
        out[k] = np.concatenate(parts[k])
    if opacities is not None:
        out["opacities"] = np.asarray(opacities, np.float32)[out["gaussian_ids"]]
    if width is not None:
        out["width"], out["height"] = int(width), int(height)
    return out


# ---- spherical harmonics -----------------------------------------------------------------------------------------------------------
def sh_reference(degree, means, coeffs, campos):
    """(colours float64 [N, 3], bound float64 [N, 3]) of gsplat's SH colour max(sum_k b_k(dir) c_k + 0.5, 0), dir = the normalised
    means - campos, evaluated in float64 on the fp32 inputs (ref_sh.spherical_harmonics).

    bound = 32 * 2^-24 * (sum_k |b_k c_k| + 0.5), per element: a chain of at most 16 fp32 fused multiply-adds errs by at most
    16 u sum_k |b_k c_k| (u = 2^-24, first order), the final + 0.5 by u times the result; the roundings of the direction (subtract,
    norm, reciprocal, scale) and of the basis polynomials enter every term b_k c_k relatively, a few u each -- the factor 2 on the
    chain's 16 u is the margin that covers them.  Derived from the operation count, not measured."""
    nb = (degree + 1) ** 2
    m = torch.from_numpy(np.asarray(means, np.float32)).double()
    c = torch.from_numpy(np.asarray(coeffs, np.float32)).double()
    dirs = m - torch.from_numpy(np.asarray(campos, np.float32)).double()
    assert c.shape[1] >= nb
    x = ref_sh.spherical_harmonics(degree, dirs, c)
    # the basis itself: the colours of the identity coefficient table, one channel per basis function
    eye = torch.eye(nb, dtype=torch.float64).expand(m.shape[0], nb, nb)
    basis = ref_sh.spherical_harmonics(degree, dirs, eye)
    mag = torch.einsum("nk,nkc->nc", basis.abs(), c[:, :nb].abs())
    return torch.clamp(x + 0.5, min=0.0).numpy(), (32.0 * U * (mag + 0.5)).numpy()


def sh_cases(degree, K, N, seed=0):
    """Inputs of the SH grid: a list of dicts (means, coeffs [N, K, 3], campos, at_camera = index of the Gaussian AT the camera
    centre or None, clamped = index of the Gaussian whose DC coefficients are -10 or None).  N > 1: one case holding both; N = 1:
    two cases, one Gaussian each."""
    rng = np.random.default_rng(1000 * degree + 10 * K + N + seed)
    campos = np.array([0.7, -1.9, 2.3], np.float32)

    def make(at_camera, clamped):
        means = rng.uniform(-1.5, 1.5, (N, 3)).astype(np.float32)
        coeffs = (0.3 * rng.standard_normal((N, K, 3))).astype(np.float32)
        if at_camera is not None:
            means[at_camera] = campos
        if clamped is not None:
            coeffs[clamped, 0] = -10.0
        return dict(means=means, coeffs=coeffs, campos=campos, at_camera=at_camera, clamped=clamped)

    if N == 1:
        return [make(0, None), make(None, 0)]
    return [make(N // 3, N - 1)]


SH_GRID = [(degree, K, N) for degree in range(4) for K in sorted({(degree + 1) ** 2, 16}) for N in (1, 257, 4000)]
