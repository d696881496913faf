"""CPU tests of the oracle's option branches (near / far planes, radius_clip, eps2d, SH degrees below 3) and of the references
in dropin_ref.py that tests/test_gpu_dropin_options.py holds the HIP kernels and the drop-in `rasterization()` against.  The
oracle is the GPU tests' yardstick, and these branches of it ran in no test: a float64 reference decides here.  No GPU needed."""
import numpy as np
import pytest

import dropin_ref as ref
import ref_np
from util import npy, scene_np

_SCENES, _DEFAULT = {}, {}


def scene(name):
    if name not in _SCENES:
        cfg, sc = scene_np(name)
        _SCENES[name] = (cfg, npy(sc))
    return _SCENES[name]


def project(orc, name, v, **kw):
    cfg, h = scene(name)
    return orc.project(h["means"], h["quats"], h["scales"], h["vms"][v], h["K"], cfg.width, cfg.height, **kw)


def depths64(name, v):
    """Camera depth of EVERY Gaussian in float64."""
    _, h = scene(name)
    vm = h["vms"][v].astype(np.float64)
    return h["means"].astype(np.float64) @ vm[2, :3] + vm[2, 3]


def default_of(orc, name, v):
    """(default projection, clip_parameters of it): computed once, read by every test."""
    if (name, v) not in _DEFAULT:
        p = project(orc, name, v)
        _DEFAULT[name, v] = (p, ref.clip_parameters(p, all_depths=depths64(name, v).astype(np.float32)))
    return _DEFAULT[name, v]


VIEWS = [("T0", 0), ("T0", 1), ("T1", 0), ("T1", 1)]


# ---- 1. between cuts: the float64 reference decides every Gaussian -----------------------------------------------------------------
@pytest.mark.parametrize("eps2d", [0.05, 0.3, 1.0])
@pytest.mark.parametrize("name,v", VIEWS)
def test_oracle_equals_the_float64_projection_under_clip_planes_and_eps2d(orc, name, v, eps2d):
    cfg, h = scene(name)
    p0, cp = default_of(orc, name, v)
    near, far = cp["near_between"], cp["far_between"]
    z = depths64(name, v)
    gap = np.minimum(np.abs(z - near), np.abs(z - far)) / np.abs(z)
    print(f"{name} view {v}: near {near} far {far}, min relative gap to a cut {gap.min():.3e}")
    assert gap.min() > 1e-4  # precondition: fp32 and float64 depths fall on the same side of both cuts
    p = project(orc, name, v, near=near, far=far, eps2d=eps2d)
    p64 = ref_np.project(h["means"], h["quats"], h["scales"], h["vms"][v], h["K"], cfg.width, cfg.height, near=near, far=far,
                         eps2d=eps2d)
    ok = p["radii"] > 0
    n_default = int((project(orc, name, v, eps2d=eps2d)["radii"] > 0).sum())
    assert 0 < int(ok.sum()) < n_default  # the cuts bite
    assert np.array_equal(ok, p64["ok"])  # every Gaussian, no case left out
    assert np.array_equal(p["radii"][ok], p64["radius"][ok])
    assert np.array_equal(p["rect"][ok], p64["rect"][ok])
    np.testing.assert_allclose(p["means2d"][ok], p64["mu"][ok], rtol=2e-6, atol=2e-5)
    np.testing.assert_allclose(p["conics"][ok], p64["conic"][ok], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(p["depths"][ok], z[ok], rtol=2e-6)
    # what is cut away leaves nothing behind
    for k in ("means2d", "depths", "conics", "rect"):
        assert not p[k][~ok].any(), k


# ---- 2. exact cuts ----------------------------------------------------------------------------------------------------------------
def test_a_gaussian_exactly_on_a_clip_plane_is_kept_and_one_ulp_outside_is_culled(orc):
    s = ref.exact_cut_scene()
    args = (s["means"], s["quats"], s["scales"], s["viewmat"], s["K"], s["W"], s["H"])
    p0 = orc.project(*args)
    z = s["means"][:, 2]
    assert (p0["radii"] > 0).all() and np.array_equal(p0["depths"], z)  # all on screen; the camera depth IS means[:, 2]
    near, far, roles = np.float32(s["near"]), np.float32(s["far"]), s["roles"]
    assert (z[roles["on_near"]] == near).all() and (z[roles["on_far"]] == far).all()          # Gaussians sit on each cut
    assert (z[roles["below_near"]] < near).all() and (z[roles["above_far"]] > far).all()
    for kw, want in ((dict(near=s["near"]), z >= near), (dict(far=s["far"]), z <= far),
                     (dict(near=s["near"], far=s["far"]), (z >= near) & (z <= far))):
        p = orc.project(*args, **kw)
        vis = p["radii"] > 0
        assert np.array_equal(vis, want), kw
        assert 0 < int(vis.sum()) < z.size
        for k in ("radii", "means2d", "depths", "conics", "rect"):  # the survivors are untouched
            assert np.array_equal(p[k][vis], p0[k][vis]), (kw, k)
    p = orc.project(*args, near=s["near"], far=s["far"])
    vis = p["radii"] > 0
    for k in ("on_near", "above_near", "on_far", "below_far"):
        assert vis[roles[k]].all(), k
    for k in ("below_near", "above_far"):
        assert not vis[roles[k]].any(), k


@pytest.mark.parametrize("name,v", VIEWS)
def test_occurring_clip_values_keep_the_gaussians_on_them(orc, name, v):
    """near = an occurring depth, far = another: `z < near || z > far` culls, so both stay."""
    p0, cp = default_of(orc, name, v)
    vis0, z = p0["radii"] > 0, p0["depths"]
    near, far = np.float32(cp["near"]), np.float32(cp["far"])
    assert int((z[vis0] == near).sum()) >= 1 and int((z[vis0] == far).sum()) >= 1  # a Gaussian on each cut
    for kw, want in ((dict(near=cp["near"]), vis0 & (z >= near)), (dict(far=cp["far"]), vis0 & (z <= far)),
                     (dict(near=cp["near"], far=cp["far"]), vis0 & (z >= near) & (z <= far))):
        p = project(orc, name, v, **kw)
        vis = p["radii"] > 0
        assert np.array_equal(vis, want), kw
        assert 0 < int(vis.sum()) < int(vis0.sum()), kw
        for k in ("radii", "means2d", "depths", "conics", "rect"):
            assert np.array_equal(p[k][vis], p0[k][vis]), (kw, k)


# ---- 3. radius_clip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,v", VIEWS)
def test_radius_clip_culls_its_own_radius_and_keeps_the_next(orc, name, v):
    p0, cp = default_of(orc, name, v)
    rc = cp["radius_clip"]
    r0 = p0["radii"]
    assert int((r0 == rc).sum()) >= 1 and int((r0 == rc + 1).sum()) >= 1  # the equality cut and its neighbour both occur
    p = project(orc, name, v, radius_clip=rc)
    assert np.array_equal(p["radii"], np.where(r0 > rc, r0, 0))
    vis = p["radii"] > 0
    assert 0 < int(vis.sum()) < int((r0 > 0).sum())
    assert not vis[r0 == rc].any() and vis[r0 == rc + 1].all()
    for k in ("means2d", "depths", "conics", "rect"):
        assert np.array_equal(p[k][vis], p0[k][vis]), k
        assert not p[k][~vis].any(), k
    # together with both planes: the intersection of the three
    z = p0["depths"]
    pa = project(orc, name, v, near=cp["near"], far=cp["far"], radius_clip=rc)
    want = (r0 > rc) & (z >= np.float32(cp["near"])) & (z <= np.float32(cp["far"]))
    assert np.array_equal(pa["radii"] > 0, want) and 0 < int(want.sum()) < int(vis.sum())


def test_bin_sort_of_a_clipped_projection_lists_only_the_survivors(orc):
    cfg, _ = scene("T1")
    p0, cp = default_of(orc, "T1", 0)
    p = project(orc, "T1", 0, near=cp["near"], far=cp["far"], radius_clip=cp["radius_clip"])
    b = orc.bin_sort(p, cfg.width, cfg.height)
    vis = p["radii"] > 0
    rect = p["rect"].astype(np.int64)
    assert b["n_isect"] == int(((rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]))[vis].sum()) > 0
    assert vis[b["flatten_ids"]].all()
    assert set(np.unique(b["flatten_ids"])) == set(np.nonzero(vis & ((rect[:, 2] > rect[:, 0]) & (rect[:, 3] > rect[:, 1])))[0])


# ---- 4. spherical harmonics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,K,N", ref.SH_GRID)
def test_oracle_sh_colors_within_the_derived_bound_of_float64(orc, degree, K, N):
    for case in ref.sh_cases(degree, K, N):
        want, bound = ref.sh_reference(degree, case["means"], case["coeffs"], case["campos"])
        got = orc.sh_colors(degree, case["means"], case["coeffs"], case["campos"])
        assert got.shape == (N, 3) and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - want)
        print(f"degree {degree} K {K} N {N}: max err / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        if case["at_camera"] is not None:  # no direction: the DC term alone
            i = case["at_camera"]
            dc = np.maximum(0.28209479177387814 * case["coeffs"][i, 0].astype(np.float64) + 0.5, 0.0)
            assert (np.abs(want[i] - dc) <= 1e-15).all() and (np.abs(got[i] - dc) <= bound[i]).all()
        if case["clamped"] is not None:
            i = case["clamped"]
            assert (want[i] == 0.0).all() and np.array_equal(got[i], np.zeros(3, np.float32))  # exactly 0.0
        assert N == 1 or (want > 0).sum() > N  # (the clamp is the exception, not the rule)


def test_sh_degree_below_the_stored_bands_reads_only_its_own(orc):
    """[N, 16, 3] stored, a lower degree asked for: the result is that of the truncated table, bit for bit, and not degree 3's."""
    case = ref.sh_cases(3, 16, 257)[0]
    full = orc.sh_colors(3, case["means"], case["coeffs"], case["campos"])
    for degree in (0, 1, 2):
        nb = (degree + 1) ** 2
        wide = orc.sh_colors(degree, case["means"], case["coeffs"], case["campos"])
        tight = orc.sh_colors(degree, case["means"], np.ascontiguousarray(case["coeffs"][:, :nb]), case["campos"])
        assert np.array_equal(wide, tight) and not np.array_equal(wide, full)


# ---- 5. the packed meta, by hand ----------------------------------------------------------------------------------------------------
def test_packed_meta_on_a_case_written_out_by_hand():
    """2 cameras, 3 Gaussians, 2 x 1 tiles (32 x 16 pixels): tile_n_bits = floor(log2(2)) + 1 = 2, the camera sits at bit 34."""
    f = np.float32
    one, two, half, three = 0x3F800000, 0x40000000, 0x3F000000, 0x40400000  # depth bits of 1.0, 2.0, 0.5, 3.0
    cam0 = dict(
        proj=dict(radii=np.array([2, 0, 3], np.int32), depths=np.array([1.0, 0.0, 2.0], f),
                  means2d=np.array([[5, 6], [0, 0], [16, 8]], f), conics=np.array([[1, 0, 1], [0, 0, 0], [2, 0.5, 2]], f),
                  rect=np.array([[0, 0, 1, 1], [0, 0, 0, 0], [0, 0, 2, 1]], np.int32)),
        bins=dict(isect_ids=np.array([(0 << 32) | one, (0 << 32) | two, (1 << 32) | two], np.int64),
                  flatten_ids=np.array([0, 2, 2], np.int32), tile_offsets=np.array([0, 2, 3], np.int32), n_isect=3,
                  tile_w=2, tile_h=1))
    cam1 = dict(
        proj=dict(radii=np.array([0, 4, 1], np.int32), depths=np.array([0.0, 0.5, 3.0], f),
                  means2d=np.array([[0, 0], [15, 7], [30, 3]], f), conics=np.array([[0, 0, 0], [3, 0, 3], [4, -1, 4]], f),
                  rect=np.array([[0, 0, 0, 0], [0, 0, 2, 1], [1, 0, 2, 1]], np.int32)),
        bins=dict(isect_ids=np.array([(0 << 32) | half, (1 << 32) | half, (1 << 32) | three], np.int64),
                  flatten_ids=np.array([1, 1, 2], np.int32), tile_offsets=np.array([0, 1, 3], np.int32), n_isect=3,
                  tile_w=2, tile_h=1))
    m = ref.packed_meta([cam0, cam1], opacities=np.array([0.1, 0.2, 0.3], f), width=32, height=16)
    want = dict(
        camera_ids=[0, 0, 1, 1], gaussian_ids=[0, 2, 1, 2], radii=[2, 3, 4, 1], depths=[1.0, 2.0, 0.5, 3.0],
        means2d=[[5, 6], [16, 8], [15, 7], [30, 3]], conics=[[1, 0, 1], [2, 0.5, 2], [3, 0, 3], [4, -1, 4]],
        opacities=[f(0.1), f(0.3), f(0.2), f(0.3)], tiles_per_gauss=[1, 2, 2, 1],
        isect_ids=[one, two, (1 << 32) | two, (1 << 34) | half, (1 << 34) | (1 << 32) | half, (1 << 34) | (1 << 32) | three],
        flatten_ids=[0, 1, 1, 2, 2, 3], isect_offsets=[[[0, 2]], [[3, 4]]],
        tile_width=2, tile_height=1, tile_size=16, n_cameras=2, width=32, height=16)
    assert set(m) == set(want)
    for k, v in want.items():
        assert np.array_equal(np.asarray(m[k]), np.asarray(v)), k
    assert m["isect_offsets"].shape == (2, 1, 2) and m["isect_ids"].dtype == np.int64 and m["gaussian_ids"].dtype == np.int64
    # 16 tiles are a power of two: floor(log2(16)) + 1 = 5 tile bits, not 4
    cam0["bins"].update(tile_w=4, tile_h=4, tile_offsets=np.array([0, 2] + [3] * 15, np.int32))
    cam1["bins"].update(tile_w=4, tile_h=4, tile_offsets=np.array([0, 1] + [3] * 15, np.int32))
    m16 = ref.packed_meta([cam0, cam1])
    assert int(m16["isect_ids"][3]) == (1 << 37) | half and m16["isect_offsets"].shape == (2, 4, 4)
