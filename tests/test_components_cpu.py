"""Radius components without a GPU: the brute-force reference (components_ref.components) against sklearn's DBSCAN where fp32 and
float64 agree exactly; the float32 mirror of the kernel's ring walk and stop rule (components_ref.radius_walk_ref) against the
brute-force neighbour sets; the chain cases; the host logic of gsbp_amd.components; the C ABI's validation.  Every comparison is of
integers and exact."""
import numpy as np
import pytest
import torch
from sklearn.cluster import DBSCAN

import gsbp_amd
from gsbp_amd import _lib, components as comp, spatial
from gsbp_amd._lib import GwbpError

import components_ref as cref
import spatial_ref as ref

OFFSETS = (0.0, 1024.0)


def thinned(off, keep=0.33):
    lat = ref.lattice(16, 0, off)
    return lat[np.random.default_rng(3).random(len(lat)) < keep]


def same_partition(a, b):
    """Two labelings of the same items are the same partition: the pairs (a, b) are a bijection between the labels."""
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs})


def against_sklearn(p, radius, min_points, got):
    """The core set, the noise set and the partition of the core points equal sklearn's; a border point lies in the component of one
    of its core neighbours, and in sklearn's where those all lie in one component.  Returns the number of border points left out of
    that last, exact comparison."""
    sk = DBSCAN(eps=radius, min_samples=min_points, algorithm="kd_tree").fit(p.astype(np.float64))
    core = np.zeros(len(p), bool)
    core[sk.core_sample_indices_] = True
    assert np.array_equal(core, got["core"])
    assert np.array_equal(sk.labels_ == -1, got["labels"] == -1)
    assert same_partition(sk.labels_[core], got["labels"][core])
    nb, _ = cref.neighbour_matrix(p, radius)
    for i in np.nonzero(got["border"])[0]:
        assert got["labels"][i] in set(got["labels"][nb[i] & core].tolist())
    exact = core | (got["border"] & ~got["ambiguous"])
    assert same_partition(sk.labels_[exact], got["labels"][exact])
    return int(got["ambiguous"].sum())


# min_points -> (components, largest, border points, ambiguous border points) of the thinned 16^3 lattice at radius 1/16, N = 1389:
# counts of a prototype with the contract's definitions, which the reference must reproduce at both offsets
LATTICE_COUNTS = {1: (223, 901, None, None), 3: (48, None, 309, 0), 4: (98, None, 471, 75)}


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("min_points", sorted(LATTICE_COUNTS))
def test_reference_equals_sklearn_on_the_thinned_lattice(off, min_points):
    """radius = 1/16 is the lattice step: d2 == r2 occurs exactly, in fp32 and in float64 alike, so the <= is on trial."""
    p = thinned(off)
    assert p.shape[0] == 1389
    got = cref.components(p, 1.0 / 16.0, min_points)
    n_comp, largest, n_border, n_ambiguous = LATTICE_COUNTS[min_points]
    assert got["sizes"].shape[0] == n_comp and int(got["sizes"].sum()) == int((got["labels"] >= 0).sum())
    if largest is not None:
        assert int(got["sizes"].max()) == largest and got["core"].all() and not got["border"].any()
    else:
        assert int(got["border"].sum()) == n_border and int(got["ambiguous"].sum()) == n_ambiguous
    left_out = against_sklearn(p, 1.0 / 16.0, min_points, got)
    assert left_out == (n_ambiguous or 0)
    # the numbering: components in ascending order of their smallest core member
    firsts = [int(np.nonzero(got["core"] & (got["labels"] == c))[0][0]) for c in range(n_comp)]
    assert firsts == sorted(firsts)


@pytest.mark.parametrize("off", OFFSETS)
def test_reference_equals_sklearn_at_a_radius_that_is_no_lattice_distance(off):
    p = thinned(off, 0.12)
    assert p.shape[0] == 547
    got = cref.components(p, 0.09, 1)
    assert got["sizes"].shape[0] == 116
    sk = DBSCAN(eps=0.09, min_samples=1, algorithm="kd_tree").fit(p.astype(np.float64))
    assert same_partition(sk.labels_, got["labels"]) and (got["labels"] >= 0).all()


def gap_radius(p, r0):
    """The midpoint of the widest gap between consecutive sorted pair distances in [r0, 1.1 r0]: no pair sits on the boundary."""
    p64 = p.astype(np.float64)
    d = np.sqrt(((p64[:, None, :] - p64[None, :, :]) ** 2).sum(-1))[np.triu_indices(len(p), 1)]
    d = np.sort(d[(d >= r0) & (d <= 1.1 * r0)])
    at = int(np.argmax(np.diff(d)))
    return float(np.float32(0.5 * (d[at] + d[at + 1]))), p64


@pytest.mark.parametrize("min_points", [1, 5])
def test_reference_equals_sklearn_on_random_floats(min_points):
    p = spatial.clustered_points(3000).numpy()
    radius, p64 = gap_radius(p, 0.01)
    nb, _ = cref.neighbour_matrix(p, radius)
    d64 = np.sqrt(((p64[:, None, :] - p64[None, :, :]) ** 2).sum(-1))
    assert np.array_equal(nb, d64 <= radius)  # the two precisions agree on every pair
    got = cref.components(p, radius, min_points)
    assert 10 < got["sizes"].shape[0] < 3000
    against_sklearn(p, radius, min_points, got)


# ---- the walk ------------------------------------------------------------------------------------------------------------------------

def fine_grid(points, radius):
    """(lo, h, dims): cells of radius / 8 on the box of the points that lie together, cut down to 2^20 cells."""
    lo, _, _ = ref.grids_for(points, 1.0)["one_cell"]
    p = np.asarray(points, np.float64)
    p = p[(np.abs(p - np.median(p, axis=0)) < 100).all(axis=1)]
    h = radius / 8.0
    dims = [int(min(max(np.ceil(e / h), 1), 1024)) for e in p.max(axis=0) - p.min(axis=0)]
    while dims[0] * dims[1] * dims[2] > 1 << 20:
        a = dims.index(max(dims))
        dims[a] = (dims[a] + 1) // 2
    return lo, h, tuple(dims)


def walk_sets(off):
    sets = dict(ref.lattice_sets(8, off))
    sets["thinned"] = thinned(off)
    return sets


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("name", sorted(walk_sets(0.0)))
def test_radius_walk_finds_exactly_the_brute_force_neighbour_sets(name, off):
    pts = walk_sets(off)[name]
    radius = 0.5 if name == "clusters_floaters" else 1.0 / 16.0
    r2 = cref.r2_of(radius)
    nb, _ = cref.neighbour_matrix(pts, radius)
    want = [np.nonzero(row)[0] for row in nb]
    grids = ref.grids_for(pts, 0.5 if name == "clusters_floaters" else 4.0 / 64.0)
    grids["fine"] = fine_grid(pts, radius)
    for gname, (lo, h, dims) in grids.items():
        found, rings = cref.radius_walk_ref(pts, r2, lo, h, dims)
        assert all(np.array_equal(f, w) for f, w in zip(found, want)), (name, off, gname)
        assert rings.max() < max(dims) + 1  # the trip bound
        if gname == "fine" and max(dims) > 16:
            # the stop rule fires: the radius is 8 cells, a bound clears it after ring 8, or 9 for a query on a cell face
            assert rings.max() <= 11, (name, off, int(rings.max()))


def test_radius_walk_with_separate_queries_and_non_finite_rows():
    pts = ref.lattice(8, 0, 0.0)[:200].copy()
    pts[3, 1], pts[17, 0] = np.nan, np.inf
    q = np.concatenate([ref.lattice(8, 1, 0.0)[:20], np.array([[64.0, -64.0, 0.25], [np.nan, 0, 0]], np.float32)])
    nb, _ = cref.neighbour_matrix(pts, 0.125, queries=q)
    found, rings = cref.radius_walk_ref(pts, cref.r2_of(0.125), (0.0, 0.0, 0.0), 1.0 / 16.0, (7, 7, 7), queries=q)
    assert all(np.array_equal(f, np.nonzero(row)[0]) for f, row in zip(found, nb))
    assert found[-1].size == 0 and found[-2].size == 0 and rings[-1] == 0 and max(f.size for f in found) > 1


# ---- the chain -----------------------------------------------------------------------------------------------------------------------

def chain_points():
    pos = np.random.default_rng(5).permutation(2048)
    pts = np.zeros((2048, 3), np.float32)
    pts[:, 0] = pos / 16.0
    return pts, pos


def test_chain():
    pts, pos = chain_points()
    one = cref.components(pts, 1.0 / 16.0)
    assert one["sizes"].tolist() == [2048] and (one["labels"] == 0).all()
    none = cref.components(pts, 0.99 / 16.0)
    assert none["sizes"].tolist() == [1] * 2048 and np.array_equal(none["labels"], np.arange(2048))
    eight = cref.components(pts, 1.0 / 16.0, group=pos // 256)
    assert eight["sizes"].tolist() == [256] * 8 and same_partition(eight["labels"], pos // 256)
    assert cref.components(pts, 1.0 / 16.0, 3)["core"].sum() == 2046  # the two ends have two neighbours, themselves included


# ---- host logic ------------------------------------------------------------------------------------------------------------------------

def result_of(labels, n_comp):
    labels = torch.tensor(labels, dtype=torch.int32)
    return comp.Components(labels, torch.bincount(labels[labels >= 0].long(), minlength=n_comp), labels >= 0)


def test_select_components():
    #                 0  1  2  3   4  5  6  7  8   9
    res = result_of([2, 0, 0, 1, -1, 1, 3, 3, 0, -1], 4)  # sizes 3, 2, 1, 2
    sel = comp.select_components
    assert sel(res, seeds=[3]).tolist() == [False, False, False, True, False, True, False, False, False, False]
    assert sel(res, seeds=[4]).sum() == 0 and sel(res, seeds=[]).sum() == 0                      # a noise seed selects nothing
    assert sel(res, seeds=torch.tensor([0, 6])).nonzero().flatten().tolist() == [0, 6, 7]
    assert sel(res, largest=1).nonzero().flatten().tolist() == [1, 2, 8]
    assert sel(res, largest=2).nonzero().flatten().tolist() == [1, 2, 3, 5, 8]                    # 1 and 3 tie: the smaller id
    assert sel(res, largest=0).sum() == 0 and sel(res, largest=9).sum() == 8
    assert sel(res, min_size=2).nonzero().flatten().tolist() == [1, 2, 3, 5, 6, 7, 8]
    assert sel(res, min_size=4).sum() == 0
    assert sel(res, seeds=[0], largest=1, min_size=3).nonzero().flatten().tolist() == [0, 1, 2, 8]  # the union
    assert sel(res, largest=1).dtype == torch.bool
    with pytest.raises(GwbpError, match="seeds, largest or min_size"):
        sel(res)
    with pytest.raises(GwbpError, match="indices"):
        sel(res, seeds=[10])
    with pytest.raises(GwbpError, match="largest"):
        sel(res, largest=-1)


def test_rank_components_orders_by_size_then_id():
    res = result_of([2, 0, 0, 1, -1, 1, 3, 3, 0, -1], 4)
    inst, order = comp.rank_components(res.labels, res.sizes, 1)
    assert order.tolist() == [0, 1, 3, 2] and inst.tolist() == [3, 0, 0, 1, -1, 1, 2, 2, 0, -1] and inst.dtype == torch.int32
    inst, order = comp.rank_components(res.labels, res.sizes, 2)
    assert order.tolist() == [0, 1, 3] and inst.tolist() == [-1, 0, 0, 1, -1, 1, 2, 2, 0, -1]
    inst, order = comp.rank_components(res.labels, res.sizes, 4)
    assert order.numel() == 0 and (inst == -1).all()


def test_dense_labels_and_empty_results():
    root = torch.tensor([5, -1, 2, 2, 5, 9, -1, 2], dtype=torch.int32)
    labels, sizes = comp.dense_labels(root)
    assert labels.tolist() == [1, -1, 0, 0, 1, 2, -1, 0] and sizes.tolist() == [3, 2, 1] and sizes.dtype == torch.int64
    for root in (torch.full((4,), -1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)):
        labels, sizes = comp.dense_labels(root)
        assert labels.shape == root.shape and (labels == -1).all() and sizes.shape == (0,)
        res = comp.Components(labels, sizes, labels >= 0)
        assert comp.select_components(res, largest=3, min_size=1, seeds=[]).sum() == 0
        inst, order = comp.rank_components(labels, sizes)
        assert inst.shape == root.shape and order.numel() == 0


def test_radius_from_distances_against_numpy():
    rng = np.random.default_rng(8)
    dist = np.sort(rng.random((201, 9)).astype(np.float32), axis=1)
    dist[4, -1], dist[9, -1] = np.inf, np.nan
    col = dist[:, -1].astype(np.float64)
    col = np.sort(col[np.isfinite(col)])
    want = 2.5 * col[(col.size - 1) // 2]
    assert comp.radius_from_distances(torch.from_numpy(dist), 2.5) == want
    assert comp.radius_from_distances(torch.full((3, 2), float("inf"))) == 0.0


def test_python_api_refuses_host_tensors_and_bad_arguments():
    p = torch.zeros(8, 3)
    for fn, args in ((gsbp_amd.radius_count, (p, 0.1)), (gsbp_amd.radius_components, (p, 0.1))):
        with pytest.raises(GwbpError, match="HIP tensor"):
            fn(*args)
    for fn, args in ((gsbp_amd.suggest_radius, (p,)), (gsbp_amd.split_instances, (p, torch.ones(8, dtype=torch.bool)))):
        with pytest.raises(GwbpError, match="HIP tensors"):
            fn(*args)
    for radius in (-1.0, float("nan"), float("inf")):
        with pytest.raises(GwbpError, match="radius"):
            gsbp_amd.radius_components(p, radius)
        with pytest.raises(GwbpError, match="radius"):
            gsbp_amd.radius_count(p, radius)
    with pytest.raises(GwbpError, match="min_points"):
        gsbp_amd.radius_components(p, 0.1, 0)
    with pytest.raises(GwbpError, match="cap"):
        gsbp_amd.radius_count(p, 0.1, cap=0)
    assert comp._r2(0.09) == float(np.float32(0.09) * np.float32(0.09)) and comp._r2(1.0 / 16.0) == 1.0 / 256.0


def test_new_symbols_are_exported_and_bound():
    names = {"gwbp_radius_count", "gwbp_radius_union", "gwbp_radius_attach", "gwbp_components_flatten"}
    assert names <= set(_lib.EXPORTS)
    gsbp_amd.build()
    for n in names:
        assert getattr(_lib.lib(), n) is not None
    for fn in ("radius_count", "radius_components", "suggest_radius", "select_components", "split_instances"):
        assert callable(getattr(gsbp_amd, fn))


P1, P2, P3, P4, P5, P6, P7 = (1 << 12), (1 << 13), (1 << 14), (1 << 15), (1 << 16), (1 << 17), (1 << 18)  # fake, aligned, never dereferenced
GRID = dict(lo=(0.0, 0.0, 0.0), h=1.0, dims=(2, 2, 2))


def _walk(n, pts, cell_start, lo, h, dims, group, r2):
    return (n, pts, cell_start, *lo, h, *dims, group, r2)


def _count(n=40, pts=P1, cell_start=P2, lo=GRID["lo"], h=1.0, dims=GRID["dims"], group=None, r2=1.0, q=4, queries=P3, ldq=3, order=P4,
           qgroup=None, cap=5, count=P5, visited=None):
    return _lib.lib().gwbp_radius_count(*_walk(n, pts, cell_start, lo, h, dims, group, r2), q, queries, ldq, order, qgroup, cap, count,
                                        visited, None)


def _union(n=40, pts=P1, cell_start=P2, lo=GRID["lo"], h=1.0, dims=GRID["dims"], group=None, r2=1.0, count=P5, min_points=2, parent=P6,
           status=P7):
    return _lib.lib().gwbp_radius_union(*_walk(n, pts, cell_start, lo, h, dims, group, r2), count, min_points, parent, status, None)


def _attach(n=40, pts=P1, cell_start=P2, lo=GRID["lo"], h=1.0, dims=GRID["dims"], group=None, r2=1.0, count=P5, min_points=2, attach=P6):
    return _lib.lib().gwbp_radius_attach(*_walk(n, pts, cell_start, lo, h, dims, group, r2), count, min_points, attach, None)


def _flatten(n=40, count=P5, min_points=2, attach=None, parent=P6, root=P3, status=P7):
    return _lib.lib().gwbp_components_flatten(n, count, min_points, attach, parent, root, status, None)


def _err():
    return _lib.lib().gwbp_last_error_string().decode()


def test_abi_argument_validation_needs_no_gpu():
    """Every new entry point refuses bad sizes, radii, grids, strides and null or misaligned pointers with GWBP_EINVAL and a message
    before any HIP call (the pointers are fake and never dereferenced)."""
    nan, inf = float("nan"), float("inf")
    walk = [(dict(h=0.0), "cell size"), (dict(h=nan), "cell size"), (dict(dims=(0, 2, 2)), "grid dimensions"),
            (dict(dims=(1024, 1024, 17)), "grid dimensions"), (dict(lo=(0.0, inf, 0.0)), "origin"), (dict(n=0), "bad number"),
            (dict(n=1 << 31), "bad number"), (dict(r2=-1.0), "r2"), (dict(r2=nan), "r2"), (dict(pts=None), "null"),
            (dict(cell_start=None), "null"), (dict(pts=P1 + 4), "16-B"), (dict(group=P3 + 2), "aligned")]
    for kw, word in walk + [(dict(cap=0), "cap"), (dict(q=-1), "bad number"), (dict(ldq=2), "stride"), (dict(queries=None), "null"),
                            (dict(order=None), "null"), (dict(count=None), "null"), (dict(order=P4 + 4), "aligned"),
                            (dict(visited=P6 + 1), "aligned")]:
        assert _count(**kw) == -1, kw
        assert word in _err(), (kw, _err())
    for kw, word in walk + [(dict(min_points=0), "min_points"), (dict(count=None), "null"), (dict(parent=None), "null"),
                            (dict(status=None), "null"), (dict(parent=P6 + 2), "aligned")]:
        assert _union(**kw) == -1, kw
        assert word in _err(), (kw, _err())
    for kw, word in walk + [(dict(min_points=0), "min_points"), (dict(count=None), "null"), (dict(attach=None), "null"),
                            (dict(attach=P6 + 2), "aligned")]:
        assert _attach(**kw) == -1, kw
        assert word in _err(), (kw, _err())
    for kw, word in [(dict(n=0), "bad number"), (dict(min_points=0), "min_points"), (dict(count=None), "null"), (dict(parent=None), "null"),
                     (dict(root=None), "null"), (dict(status=None), "null"), (dict(root=P6), "must not be"), (dict(attach=P4 + 1), "aligned")]:
        assert _flatten(**kw) == -1, kw
        assert word in _err(), (kw, _err())


def test_cli_parser_and_seeded_inputs():
    import run_instances
    ap = run_instances.build_parser()
    a = ap.parse_args(["--synthetic", "C1", "--radius-factor", "2", "--min-points", "4", "--keep-largest", "2", "--seed-index", "5",
                       "--seed-index", "9", "--frames", "--out", "x"])
    assert a.synthetic == "C1" and a.radius is None and a.radius_factor == 2.0 and a.min_points == 4 and a.min_size == 1
    assert a.keep_largest == 2 and a.seed_index == [5, 9] and a.frames
    with pytest.raises(SystemExit):
        ap.parse_args(["--synthetic", "C1", "--radius", "0.1", "--radius-factor", "2", "--out", "x"])
    with pytest.raises(SystemExit):
        ap.parse_args(["--synthetic", "C1", "--mask", "m.pt", "--labels", "l.pt", "--out", "x"])
    means = torch.rand(4000, 3, generator=torch.Generator().manual_seed(0))
    (mask, ball), (mask2, ball2) = comp.synthetic_instances(means), comp.synthetic_instances(means)
    assert torch.equal(mask, mask2) and torch.equal(ball, ball2) and int(ball.max()) == 2
    sizes = torch.bincount(ball[ball >= 0])
    assert sizes[0] == 500 and sizes[0] > sizes[1] > sizes[2] > 0 and bool((mask | (ball < 0)).all()) and int((mask & (ball < 0)).sum()) >= 5
