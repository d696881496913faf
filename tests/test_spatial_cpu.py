"""Spatial k-NN without a GPU: the float32 mirror of the kernel's grid walk and stop rule (spatial_ref.grid_knn_ref) against brute
force on lattice sets where fp32 is exact; plan_grid; the host logic of remove_outliers / init_scales; the C ABI's validation."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib, spatial
from gsbp_amd._lib import GwbpError

import spatial_ref as ref

KS = (1, 4, 32)
SETS = {off: ref.lattice_sets(8, off) for off in (0.0, 1024.0)}
NAMES = sorted(SETS[0.0])
_BRUTE = {}


def brute(off, name, k):
    if (off, name) not in _BRUTE:  # one search at k = 32 serves every k: a row's first k entries are its k nearest
        _BRUTE[off, name] = ref.brute(SETS[off][name], 32)
    d, i = _BRUTE[off, name]
    return d[:, :k], i[:, :k]


def same(got, want):
    (gd, gi), (wd, wi) = got, want
    # (the float64 distance rounded to the float32 it is returned in: sqrt in 53 bits, rounded again to 24, is the correctly
    # rounded float32 sqrt of the exact squared distance)
    return np.array_equal(gi, wi) and np.array_equal(gd, wd.astype(np.float32))


@pytest.mark.parametrize("off", [0.0, 1024.0])
@pytest.mark.parametrize("name", NAMES)
def test_grid_walk_equals_brute_force_on_lattice_sets(name, off):
    """cell_size = 1/16 puts points exactly on cell faces; with the common offset of 1024 the cell assignment works at 2^10 times
    the magnitude of the cell size.  Indices and distances equal float64 brute force bit for bit, ties included -- and so do the
    same searches with one cell, 2 cells per axis and about one point per cell."""
    pts = SETS[off][name]
    grids = ref.grids_for(pts, 4.0 / 64.0 if name != "clusters_floaters" else 0.5)
    for k in KS:
        want = brute(off, name, k)
        assert (want[1] >= 0).all()
        for gname, (lo, h, dims) in grids.items():
            got = ref.grid_knn_ref(pts, k, lo, h, dims)
            assert same(got, want), (name, off, k, gname)


def test_the_walk_stops_early_and_self_comes_first():
    """The stop rule does stop: on the 8^3 lattice with cells of one lattice step, k = 1 needs the query's cell and at most one ring
    (a point ON a face has a zero bound towards that side), far fewer than the grid's 8; and every point finds itself at distance 0."""
    pts = SETS[0.0]["lattice"]
    lo, h, dims = ref.grids_for(pts, 4.0 / 64.0)["one_per_cell"]
    d, i, rings = ref.grid_knn_ref(pts, 1, lo, h, dims, return_rings=True)
    assert np.array_equal(i[:, 0], np.arange(pts.shape[0])) and (d == 0).all()
    assert rings.max() <= 2
    d, i, rings = ref.grid_knn_ref(pts, 4, lo, h, dims, return_rings=True)
    assert rings.max() <= 3 and same((d, i), brute(0.0, "lattice", 4))


@pytest.mark.parametrize("k", KS)
def test_n_equals_k_and_a_box_without_points(k):
    pts = SETS[1024.0]["duplicates"][:k]
    want = ref.brute(pts, k)
    for lo, h, dims in (((1024.0, 1024.0, 1024.0), 1.0 / 16.0, (8, 8, 8)), ((0.0, 0.0, 0.0), 1.0, (1, 1, 1)),
                        ((-500.0, 3000.0, 77.0), 1.0 / 16.0, (4, 5, 6))):  # the last box contains no point at all
        assert same(ref.grid_knn_ref(pts, k, lo, h, dims), want)
    big = SETS[0.0]["lattice"]
    assert same(ref.grid_knn_ref(big, k, (-500.0, 3000.0, 77.0), 1.0 / 16.0, (4, 5, 6)), brute(0.0, "lattice", k))


def test_separate_queries_non_finite_points_and_short_rows():
    pts = SETS[0.0]["lattice"][:40].copy()
    pts[3, 1], pts[17, 0], pts[30, 2] = np.nan, np.inf, -np.inf
    q = np.concatenate([SETS[0.0]["lattice"][100:110], np.array([[64.0, -64.0, 0.25], [np.nan, 0, 0]], np.float32)])
    want = ref.brute(pts, 4, q)
    got = ref.grid_knn_ref(pts, 4, (0.0, 0.0, 0.0), 1.0 / 16.0, (7, 7, 7), q)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0].astype(np.float32), equal_nan=True)
    assert (got[1][-1] == -1).all() and np.isnan(got[0][-1]).all() and not np.isin(got[1], [3, 17, 30]).any()
    few = np.full((5, 3), np.nan, np.float32)
    few[1], few[4] = (0.5, 0.25, 0), (0.5, 0.25, 0)
    d, i = ref.grid_knn_ref(few, 4, (0.0, 0.0, 0.0), 1.0 / 16.0, (3, 3, 3))
    assert i[1].tolist() == [1, 4, -1, -1] and d[1].tolist() == [0, 0, np.inf, np.inf] and (i[0] == -1).all() and np.isnan(d[0]).all()


HAZARDS = [  # (lo, h, face index m, x just below face m, query, second point): found by a seeded search, checked below
    (-1.1381540298461914, 0.17724692821502686, 17, 1.8750436305999756, 1.8740670680999756, 1.873090386390686),
    (-1.4807161092758179, 0.08888853341341019, 37, 1.808159589767456, 1.807183027267456, 1.8062063455581665),
    (-1.6465290784835815, 0.09576337039470673, 20, 0.2687382996082306, 0.2677617371082306, 0.2667851150035858),
    (-1.4331964254379272, 0.1359615921974182, 22, 1.5579584836959839, 1.5569819211959839, 1.5560052394866943)]


@pytest.mark.parametrize("lo, h, m, x, q, s", HAZARDS)
def test_the_bound_needs_its_rounding_margin(lo, h, m, x, q, s):
    """The hazard of a rounded cell assignment: x lies strictly BELOW face m = lo + m h in exact arithmetic, but fl(fl(x - lo) / h)
    rounds up to m and the point is assigned to cell m.  The query sits in cell m - 1, 2^-10 from x; the second point s sits in the
    query's cell, farther from it than x but nearer than the distance to face m computed without a margin.  After ring 0 the
    search holds s; the bare bound KH - A says nothing beyond the face can beat it and stops with the wrong neighbour; the bound
    with the margin goes one ring further and finds x.  Brute force says x."""
    from fractions import Fraction as Fr
    f32 = np.float32
    assert all(float(f32(v)) == v for v in (lo, h, x, q, s))
    assert Fr(x) < Fr(lo) + m * Fr(h) and int(ref.cell_axis(x, lo, h, 64)) == m             # mis-assigned across the face
    assert int(ref.cell_axis(q, lo, h, 64)) == m - 1 and int(ref.cell_axis(s, lo, h, 64)) == m - 1
    assert Fr(x) - Fr(q) < Fr(q) - Fr(s) < Fr(float(f32(f32(f32(m) * f32(h)) - f32(f32(q) - f32(lo)))))
    pts, qq = np.array([[x, 0, 0], [s, 0, 0]], f32), np.array([[q, 0, 0]], f32)
    grid = ((lo, -1.0, -1.0), h, (64, 1, 1))
    want = ref.brute(pts, 1, qq)
    assert want[1].tolist() == [[0]]
    assert same(ref.grid_knn_ref(pts, 1, *grid, queries=qq), want)
    assert ref.grid_knn_ref(pts, 1, *grid, queries=qq, margin=False)[1].tolist() == [[1]]


# ---- plan_grid ---------------------------------------------------------------------------------------------------------------------

def check_plan(g):
    assert g.h > 0 and np.isfinite(g.h) and float(np.float32(g.h)) == g.h
    assert all(1 <= d <= spatial.MAX_DIM for d in g.dims) and g.cells <= spatial.MAX_CELLS
    assert all(np.isfinite(v) for v in g.lo)


def test_plan_grid():
    gen = torch.Generator().manual_seed(0)
    cube = torch.rand(100_000, 3, generator=gen)
    g = spatial.plan_grid(cube)
    check_plan(g)
    assert g == spatial.plan_grid(cube.clone())  # a pure function of the input
    assert 2.0 < 100_000 * g.h ** 3 < 8.0 and 20_000 < g.cells < 60_000  # about four points per cell of the occupied box
    floaters = cube.clone()
    floaters[::1000] = 1e4
    assert spatial.plan_grid(floaters).cells < 2 * g.cells  # 0.1 % far floaters do not stretch the grid
    for pts in (torch.zeros(1, 3), torch.full((50, 3), 7.0), torch.full((9, 3), float("nan")),       # N = 1, no extent, no finite
                torch.cat([torch.rand(500, 1, generator=gen), torch.zeros(500, 2)], 1),               # a line
                torch.cat([torch.rand(500, 2, generator=gen), torch.full((500, 1), 1024.0)], 1),      # a plane
                torch.rand(3000, 3, generator=gen) * torch.tensor([1e-9, 1e6, 1.0]),                  # very unequal extents
                torch.rand(3000, 3, generator=gen) * 1e-20 + 1.0):                                    # an extent below an ulp
        check_plan(spatial.plan_grid(pts))
    assert spatial.plan_grid(torch.full((50, 3), 7.0)).dims == (1, 1, 1)
    assert spatial.plan_grid(torch.full((9, 3), float("nan"))).dims == (1, 1, 1)
    line = spatial.plan_grid(torch.cat([torch.rand(500, 1, generator=gen), torch.zeros(500, 2)], 1))
    assert line.dims[1:] == (1, 1) and 50 < line.dims[0] <= 500
    # a given cell size is kept; a box that needs more cells than the caps allow is cut down, h is not changed
    g = spatial.plan_grid(cube, cell_size=1.0 / 16.0)
    check_plan(g)
    assert g.h == 1.0 / 16.0 and g.dims == (16, 16, 16)
    tiny = spatial.plan_grid(cube, cell_size=1e-4)
    check_plan(tiny)
    assert tiny.h == float(np.float32(1e-4))
    with pytest.raises(GwbpError, match="cell_size"):
        spatial.plan_grid(cube, cell_size=0.0)


def test_plan_grid_ten_million_points_in_a_unit_box():
    pts = torch.rand(10_000_000, 3, generator=torch.Generator().manual_seed(1))
    g = spatial.plan_grid(pts)
    check_plan(g)
    assert 2.0 < 1e7 * g.h ** 3 < 8.0 and g.cells > 1_000_000


# ---- host logic --------------------------------------------------------------------------------------------------------------------

def test_outlier_statistics_and_scale_formula_against_numpy():
    rng = np.random.default_rng(3)
    dist = np.sort(rng.random((200, 9)).astype(np.float32), axis=1)
    dist[:, 0] = 0
    dist[:5, 1:] += 3.0            # five rows far from their neighbours
    dist[7, 6:] = np.inf           # a short row: the mean runs over its finite distances
    dist[9, 1:] = np.inf           # a row without neighbours goes
    dist[11] = np.nan              # a non-finite point goes
    d = dist[:, 1:].astype(np.float64)
    ok = np.isfinite(d)
    md = np.array([r[m].mean() if m.any() else np.nan for r, m in zip(d, ok)])
    vals = md[~np.isnan(md)]
    want = ~np.isnan(md) & ~(md > vals.mean() + 2.0 * vals.std(ddof=1))
    got = spatial.outlier_keep(torch.from_numpy(dist), 2.0).numpy()
    assert np.array_equal(got, want) and not got[:5].any() and not got[9] and not got[11] and got[7] and got.sum() == 193
    assert spatial.outlier_keep(torch.from_numpy(dist), 1e9).sum() == 198

    dist4 = np.sort(rng.random((50, 4)), axis=1).astype(np.float32)
    want = np.log(np.sqrt((dist4[:, 1:].astype(np.float64) ** 2).mean(axis=1)) * 0.5)
    got = spatial.scales_from_distances(torch.from_numpy(dist4), 0.5).numpy()
    assert got.shape == (50, 3) and (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()
    assert np.abs(got[:, 0] - want).max() < 1e-5


def test_python_api_refuses_host_tensors_and_bad_arguments():
    p = torch.zeros(8, 3)
    with pytest.raises(GwbpError, match="HIP tensor"):
        gsbp_amd.spatial_knn(p, 2)
    with pytest.raises(GwbpError, match="HIP tensor"):
        gsbp_amd.knn_distances(p)
    with pytest.raises(GwbpError, match="HIP tensor"):
        gsbp_amd.init_scales(p)
    for fn, args in ((gsbp_amd.smooth_labels, (p, torch.zeros(8, dtype=torch.int64), 2)), (gsbp_amd.smooth_mask, (p, torch.zeros(8).bool())),
                     (gsbp_amd.remove_outliers, (p,)), (gsbp_amd.smooth_features, (p, torch.zeros(8, 4)))):
        with pytest.raises(GwbpError, match="HIP tensors"):
            fn(*args)


def test_new_symbols_are_exported_and_bound():
    names = {"gwbp_spatial_cell_keys", "gwbp_spatial_build", "gwbp_spatial_knn", "gwbp_neighbor_mean"}
    assert names <= set(_lib.EXPORTS)
    gsbp_amd.build()
    for n in names:
        assert getattr(_lib.lib(), n) is not None


P1, P2, P3, P4, P5 = (1 << 12), (1 << 13), (1 << 14), (1 << 15), (1 << 16)  # fake, aligned, never dereferenced


def _keys(n=4, points=P1, ldp=3, lo=(0.0, 0.0, 0.0), h=1.0, dims=(2, 2, 2), keys=P2):
    return _lib.lib().gwbp_spatial_cell_keys(n, points, ldp, *lo, h, *dims, keys, None)


def _build(n=4, points=P1, ldp=3, skeys=P2, perm=P3, cells=8, out=P4, cell_start=P5):
    return _lib.lib().gwbp_spatial_build(n, points, ldp, skeys, perm, cells, out, cell_start, None)


def _knn(n=40, pts=P1, cell_start=P2, lo=(0.0, 0.0, 0.0), h=1.0, dims=(2, 2, 2), q=4, queries=P3, ldq=3, order=P4, k=2, idx=P5,
         dist=P5 << 1):
    return _lib.lib().gwbp_spatial_knn(n, pts, cell_start, *lo, h, *dims, q, queries, ldq, order, k, idx, dist, None)


def _mean(n=4, m=8, D=16, k=2, idx=P1, feats=P2, ldf=16, out=P3, ldo=16):
    return _lib.lib().gwbp_neighbor_mean(n, m, D, k, idx, feats, ldf, out, ldo, None)


def _err():
    return _lib.lib().gwbp_last_error_string().decode()


def test_abi_argument_validation_needs_no_gpu():
    """Every new entry point refuses null pointers, k = 0, k = 33, n < 0, bad grids and bad strides with GWBP_EINVAL and a message
    before any HIP call (the pointers are fake and never dereferenced)."""
    nan, inf = float("nan"), float("inf")
    bad_grids = [(dict(h=0.0), "cell size"), (dict(h=nan), "cell size"), (dict(h=inf), "cell size"), (dict(h=-1.0), "cell size"),
                 (dict(dims=(0, 2, 2)), "grid dimensions"), (dict(dims=(2, 1025, 2)), "grid dimensions"),
                 (dict(dims=(1024, 1024, 17)), "grid dimensions"), (dict(lo=(0.0, nan, 0.0)), "origin")]
    for kw, word in bad_grids + [(dict(n=-1), "bad number"), (dict(n=1 << 31), "bad number"), (dict(ldp=2), "stride"),
                                 (dict(points=None), "null"), (dict(keys=None), "null"), (dict(points=P1 + 2), "aligned")]:
        assert _keys(**kw) == -1, kw
        assert word in _err(), (kw, _err())
    for kw, word in [(dict(n=-1), "bad number"), (dict(ldp=1), "stride"), (dict(cells=0), "n_cells"), (dict(cells=(1 << 24) + 1), "n_cells"),
                     (dict(points=None), "null"), (dict(skeys=None), "null"), (dict(perm=None), "null"), (dict(out=None), "null"),
                     (dict(cell_start=None), "null"), (dict(out=P4 + 4), "16-B")]:
        assert _build(**kw) == -1, kw
        assert word in _err(), (kw, _err())
    for kw, word in bad_grids + [(dict(k=0), "k must be"), (dict(k=33), "k must be"), (dict(k=9, n=8), "exceeds"), (dict(n=-1), "bad number"),
                                 (dict(n=0), "bad number"), (dict(q=-1), "bad number"), (dict(ldq=2), "stride"), (dict(pts=None), "null"),
                                 (dict(cell_start=None), "null"), (dict(queries=None), "null"), (dict(order=None), "null"),
                                 (dict(idx=None), "null"), (dict(dist=None), "null"), (dict(pts=P1 + 4), "16-B")]:
        assert _knn(**kw) == -1, kw
        assert word in _err(), (kw, _err())
    for kw, word in [(dict(k=0), "k must be"), (dict(k=33), "k must be"), (dict(n=-1), "bad sizes"), (dict(m=0), "bad sizes"),
                     (dict(D=0), "bad sizes"), (dict(ldf=15), "strides"), (dict(ldo=15), "strides"), (dict(idx=None), "null"),
                     (dict(feats=None), "null"), (dict(out=None), "null"), (dict(out=P2), "must not be"), (dict(feats=P2 + 2), "aligned")]:
        assert _mean(**kw) == -1, kw
        assert word in _err(), (kw, _err())


def test_cli_parser_and_seeded_inputs():
    import run_clean
    a = run_clean.build_parser().parse_args(["--synthetic", "C1", "--k", "8", "--remove-outliers", "--out", "x"])
    assert a.synthetic == "C1" and a.k == 8 and a.remove_outliers and a.std_ratio == 2.0 and a.min_fraction == 0.5 and a.iterations == 1
    means = torch.rand(500, 3, generator=torch.Generator().manual_seed(0))
    (noisy, clean), (noisy2, _) = spatial.synthetic_labels(means), spatial.synthetic_labels(means)
    assert torch.equal(noisy, noisy2) and 5 <= int((noisy != clean).sum()) <= 60 and int(clean.max()) < 6
    (mask, cm), (mask2, _) = spatial.synthetic_mask(means), spatial.synthetic_mask(means)
    assert torch.equal(mask, mask2) and int(cm.sum()) == 125 and bool((mask | ~cm).all()) and int((mask & ~cm).sum()) >= 1
    pts = spatial.clustered_points(20_000)
    assert torch.equal(pts, spatial.clustered_points(20_000)) and 5 <= int((pts.abs() > 2).any(dim=1).sum()) <= 50
