"""Spatial k-NN on the GPU (csrc/spatial.hip) against float64 brute force, and what is built on it: knn_distances / init_scales,
smooth_labels / smooth_mask, smooth_features (k_neighbor_mean) and remove_outliers.  N <= 4096 everywhere."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import spatial
from gsbp_amd._lib import GwbpError

import spatial_ref as ref

pytestmark = pytest.mark.gpu

KS = (1, 4, 8, 32)
SETS = {off: ref.lattice_sets(8, off) for off in (0.0, 1024.0)}
SETS[0.0]["lattice"] = ref.lattice(16, 0, 0.0)          # the first set on the GPU: a 16^3 lattice
SETS[1024.0]["lattice"] = ref.lattice(16, 0, 1024.0)
NAMES = sorted(SETS[0.0])
_BRUTE = {}


def brute(off, name, k):
    if (off, name) not in _BRUTE:  # computed once at k = 32 and shared: a row's first k entries are its k nearest
        _BRUTE[off, name] = ref.brute(SETS[off][name], 32)
    d, i = _BRUTE[off, name]
    return d[:, :k].astype(np.float32), i[:, :k]


def one_per_cell(name):
    return 0.5 if name == "clusters_floaters" else 4.0 / 64.0


@pytest.mark.parametrize("off", [0.0, 1024.0])
@pytest.mark.parametrize("name", NAMES)
def test_lattice_sets_equal_brute_force_exactly_whatever_the_grid(dev, name, off):
    """Every difference, square and sum is exact in fp32 on these sets, so idx and dist (the float64 distance rounded to the float32
    it is returned in) must match bit for bit, ties included -- with the automatic grid, one cell, cells of 1/16 (points on cell
    faces; with the offset, at 2^10 times the cell size) and about one point per cell, which must also agree with each other."""
    pts = torch.from_numpy(SETS[off][name]).to(dev)
    for k in KS:
        wd, wi = brute(off, name, k)
        for cell in (None, 1e6, 1.0 / 16.0, one_per_cell(name)):
            d, i = gsbp_amd.spatial_knn(pts, k, cell_size=cell)
            assert i.dtype == torch.int32 and d.dtype == torch.float32 and i.shape == (pts.shape[0], k)
            assert np.array_equal(i.cpu().numpy(), wi), (name, off, k, cell)
            assert np.array_equal(d.cpu().numpy(), wd), (name, off, k, cell)


@pytest.mark.parametrize("k", KS)
def test_n_equals_k_and_a_box_without_points(dev, k):
    pts = SETS[1024.0]["duplicates"][:k]
    wd, wi = ref.brute(pts, k)
    for grid in (None, spatial.Grid((-500.0, 3000.0, 77.0), 1.0 / 16.0, (4, 5, 6))):  # the box contains no point at all
        d, i = gsbp_amd.spatial_knn(torch.from_numpy(pts).to(dev), k, grid=grid)
        assert np.array_equal(i.cpu().numpy(), wi) and np.array_equal(d.cpu().numpy(), wd.astype(np.float32))
    big = torch.from_numpy(SETS[0.0]["lattice"]).to(dev)
    d, i = gsbp_amd.spatial_knn(big, k, grid=spatial.Grid((-500.0, 3000.0, 77.0), 1.0 / 16.0, (4, 5, 6)))
    wd, wi = brute(0.0, "lattice", k)
    assert np.array_equal(i.cpu().numpy(), wi) and np.array_equal(d.cpu().numpy(), wd)


def d2_torch(p, q):
    """fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32 -- torch.addcmul is not promised to fuse, so the fused steps are float64 products
    and sums (exact products; the sum rounds once to 53 bits and once more to 24, which differs from one rounding only when
    the 53-bit sum is a tie of the 24-bit grid: the test's random floats do not produce one, and a mismatch would fail loudly)."""
    d = (p - q).double()
    t = (d[..., 0].float() * d[..., 0].float()).double()
    t = (d[..., 1] * d[..., 1] + t).float().double()
    return (d[..., 2] * d[..., 2] + t).float()


def test_random_floats_with_separate_queries(dev):
    """N = 3001 uniform random floats, k = 5, Q = 777 queries of which some lie far outside the box: fp32 and float64 may order
    near-ties differently, so three properties instead of indices, no row excluded."""
    g = torch.Generator().manual_seed(5)
    n, nq, k = 3001, 777, 5
    p = torch.rand(n, 3, generator=g)
    q = torch.rand(nq, 3, generator=g)
    q[::50] = q[::50] * 40.0 - 20.0
    q[7] = torch.tensor([1e4, -3e3, 0.5])
    for queries in (q, None):
        d, i = gsbp_amd.spatial_knn(p.to(dev), k, queries=None if queries is None else queries.to(dev))
        d, i = d.cpu(), i.cpu().long()
        qq = p if queries is None else queries
        assert int(i.min()) >= 0 and int(i.max()) < n
        # (1) dist is the contract's fp32 expression for the returned index, exactly
        # (the correctly rounded fp32 sqrt as a float64 sqrt rounded once more -- 53 bits are enough for that to be innocuous;
        # torch's float32 sqrt on the host is not correctly rounded)
        assert torch.equal(d, torch.sqrt(d2_torch(p[i], qq[:, None, :]).double()).float())
        # (2) rows sorted by (dist, idx), no index twice
        assert bool(((d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (i[:, 1:] > i[:, :-1]))).all())
        # (3) the k-th distance is the true k-th distance up to fp32 rounding
        true_k = torch.cdist(qq.double(), p.double()).kthvalue(k, dim=1).values
        assert bool((d[:, -1].double() <= true_k * (1 + 2.0 ** -20)).all())
        if queries is None:
            assert torch.equal(i[:, 0], torch.arange(n)) and bool((d[:, 0] == 0).all())


def test_non_finite_points_short_rows_and_k_above_n(dev):
    pts = SETS[0.0]["duplicates"][:600].copy()
    bad = [3, 17, 30, 599]
    pts[3, 1], pts[17, 0], pts[30, 2], pts[599] = np.nan, np.inf, -np.inf, np.nan
    q = np.concatenate([SETS[0.0]["lattice"][100:140], np.array([[64.0, -64.0, 0.25], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)])
    for queries in (None, q):
        wd, wi = ref.brute(pts, 8, queries)
        d, i = gsbp_amd.spatial_knn(torch.from_numpy(pts).to(dev), 8, queries=None if queries is None else torch.from_numpy(queries).to(dev))
        d, i = d.cpu().numpy(), i.cpu().numpy()
        assert np.array_equal(i, wi) and np.array_equal(d, wd.astype(np.float32), equal_nan=True)
        assert not np.isin(i, bad).any()
        rows = bad if queries is None else [41, 42]
        assert (i[rows] == -1).all() and np.isnan(d[rows]).all()
    few = np.full((9, 3), np.nan, np.float32)
    few[1], few[4], few[8] = (0.5, 0.25, 0), (0.5, 0.25, 0), (0.5, 0.25, 1.0)
    d, i = gsbp_amd.spatial_knn(torch.from_numpy(few).to(dev), 5)
    assert i[1].tolist() == [1, 4, 8, -1, -1] and d[1].tolist() == [0, 0, 1, np.inf, np.inf]
    assert i[8].tolist() == [8, 1, 4, -1, -1] and (i[0] == -1).all() and bool(torch.isnan(d[0]).all())
    with pytest.raises(GwbpError, match="exceeds"):
        gsbp_amd.spatial_knn(torch.zeros(4, 3, device=dev), 5)
    with pytest.raises(GwbpError, match="k must be"):
        gsbp_amd.spatial_knn(torch.zeros(40, 3, device=dev), 33)


def test_two_runs_give_equal_bits_and_a_strided_slice_is_read_in_place(dev):
    g = torch.Generator().manual_seed(9)
    wide = torch.randn(2500, 7, generator=g).to(dev)
    view = wide[:, :3]
    assert not view.is_contiguous()
    a, b, c = (gsbp_amd.spatial_knn(x, 6) for x in (view, view, view.contiguous()))
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x[1], y[1]) and torch.equal(x[0].view(torch.int32), y[0].view(torch.int32))
    q = wide[:300, 2:5]
    a, c = gsbp_amd.spatial_knn(view, 6, queries=q), gsbp_amd.spatial_knn(view.contiguous(), 6, queries=q.contiguous())
    assert torch.equal(a[1], c[1]) and torch.equal(a[0], c[0])
    _, _, stats = gsbp_amd.spatial_knn(view, 6, return_stats=True)
    assert stats["cells"] == int(np.prod(stats["dims"])) and 0 < stats["occupied_cells"] <= stats["cells"]
    assert stats["points_in_cells"] == 2500 and 1 <= stats["p99_occupancy"] <= stats["max_occupancy"] <= 2500


def test_knn_distances_and_init_scales(dev):
    """On points with exact squared distances (distinct random lattice sites, i / 64) the budget against float64 is one correctly
    rounded sqrt for knn_distances, and then a mean of three squares, a sqrt and a log, each at most an ulp: 4 * 2^-24 relative.
    (The sites are a fraction of a unit apart, so the log is not near 0, where a relative bound would mean nothing.)"""
    rng = np.random.default_rng(11)
    sites = rng.choice(48 ** 3, 3000, replace=False)
    pts = (np.stack([sites % 48, (sites // 48) % 48, sites // (48 * 48)], 1) / 64.0).astype(np.float32)
    wd, _ = ref.brute(pts, 4)
    d = gsbp_amd.knn_distances(torch.from_numpy(pts).to(dev), 4)
    assert d.shape == (3000, 4) and bool((d[:, 0] == 0).all())
    tol = 4 * 2.0 ** -24
    assert np.abs(d.cpu().numpy().astype(np.float64) - wd).max() <= tol * wd.max() and \
        (np.abs(d.cpu().numpy().astype(np.float64) - wd) <= tol * wd).all()
    for init_scale in (1.0, 0.25):
        want = np.log(np.sqrt((wd[:, 1:] ** 2).mean(axis=1)) * init_scale)
        assert np.abs(want).min() > 1.0
        got = gsbp_amd.init_scales(torch.from_numpy(pts).to(dev), init_scale)
        assert got.shape == (3000, 3) and torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2])
        assert (np.abs(got[:, 0].cpu().numpy().astype(np.float64) - want) <= tol * np.abs(want)).all()


@pytest.mark.parametrize("iterations", [1, 2])
def test_smooth_labels_and_mask_are_the_majority_over_the_brute_force_neighbours(dev, iterations):
    pts = SETS[0.0]["duplicates"]
    n, k, nc = pts.shape[0], 8, 5
    _, wi = ref.brute(pts, k)
    rng = np.random.default_rng(13)
    labels = rng.integers(0, nc, n)
    labels[rng.random(n) < 0.3] = -1
    labels[wi[5]] = -1                       # a Gaussian whose neighbours are all ignored keeps -1
    labels[wi[9]] = [3, 3, 1, 1, 4, 4, 2, 0]  # a three-way tie goes to the smallest label
    want = labels.copy()
    for _ in range(iterations):
        prev = want.copy()
        for r in range(n):
            lab = prev[wi[r]]
            lab = lab[lab >= 0]
            want[r] = np.bincount(lab).argmax() if lab.size else -1
    means = torch.from_numpy(pts).to(dev)
    got = gsbp_amd.smooth_labels(means, torch.from_numpy(labels).to(dev), nc, k=k, iterations=iterations)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    if iterations == 1:
        assert want[5] == -1 and want[9] == 1
    idx = gsbp_amd.spatial_knn(means, k)[1]
    assert torch.equal(got, gsbp_amd.smooth_labels(means, torch.from_numpy(labels), nc, iterations=iterations, neighbors=idx))

    mask = rng.random(n) < 0.5
    for frac in (0.5, 0.75):
        want_m = mask.copy()
        for _ in range(iterations):
            want_m = want_m[wi].sum(axis=1).astype(np.float64) >= frac * k
        got_m = gsbp_amd.smooth_mask(means, torch.from_numpy(mask).to(dev), k=k, min_fraction=frac, iterations=iterations)
        assert got_m.dtype == torch.bool and np.array_equal(got_m.cpu().numpy(), want_m)


@pytest.mark.parametrize("D", [4, 68, 512])
def test_smooth_features_is_the_neighbour_mean(dev, D):
    g = torch.Generator().manual_seed(D)
    n, k = 700, 8
    pts = torch.rand(n, 3, generator=g)
    idx = gsbp_amd.spatial_knn(pts.to(dev), k)[1]
    idx[::7, 3] = -1
    idx[5, :] = -1                                   # a row without a valid neighbour is zero
    idx[6, 1:] = -1
    padded = torch.randn(n, D + 12, generator=g).to(dev)
    feats = padded[:, 4:4 + D] if D != 68 else padded[:, 3:3 + D]  # a padded row stride; at D = 68 also rows that are not 16-B aligned
    out = spatial.neighbor_mean(feats, idx)
    assert out.shape == (n, D) and out.is_contiguous() and bool((out[5] == 0).all())
    assert torch.equal(out, gsbp_amd.smooth_features(pts.to(dev), feats, neighbors=idx))
    f64, ii = feats.double().cpu(), idx.cpu().long()
    valid = (ii >= 0)
    gathered = f64[ii.clamp(min=0)] * valid[..., None]
    nv = valid.sum(1).clamp(min=1)[:, None]
    want = gathered.sum(1) / nv
    bound = (k + 1) * 2.0 ** -24 * gathered.abs().sum(1) / nv
    assert bool(((out.double().cpu() - want).abs() <= bound).all())
    for r in (0, 6, 7, n - 1):                       # exactly the fp32 sum in list order, divided by the count
        acc = torch.zeros(D, device=dev)
        for j in idx[r].tolist():
            if j >= 0:
                acc = acc + feats[j]
        count = torch.tensor(float(max(int((idx[r] >= 0).sum()), 1)), device=dev)  # (a device tensor: a true division)
        assert torch.equal(out[r], acc / count)


def test_remove_outliers_drops_exactly_the_floaters(dev):
    g = torch.Generator().manual_seed(17)
    a = 0.02 * torch.randn(400, 3, generator=g)
    b = 0.02 * torch.randn(400, 3, generator=g) + torch.tensor([1.0, 0.0, 0.5])
    floaters = torch.tensor([[5.0, 5.0, 5.0], [-4.0, 2.0, 0.0], [0.5, 0.0, 6.0], [9.0, -9.0, 1.0], [0.5, 3.0, 0.25]])
    pts = torch.cat([a, floaters[:2], b, floaters[2:]])
    is_floater = torch.zeros(805, dtype=torch.bool)
    is_floater[400:402] = is_floater[802:] = True
    keep = gsbp_amd.remove_outliers(pts.to(dev), k=8, std_ratio=2.0)
    assert keep.dtype == torch.bool and torch.equal(keep.cpu(), ~is_floater)
    # within a mask: the search runs on the subset, Gaussians outside stay outside, and the second cluster is not there to be near
    mask = torch.ones(805, dtype=torch.bool)
    mask[402:802] = False
    mask[0:10] = False
    keep = gsbp_amd.remove_outliers(pts.to(dev), mask.to(dev), k=8, std_ratio=2.0)
    assert torch.equal(keep.cpu(), mask & ~is_floater)
    assert int(gsbp_amd.remove_outliers(pts.to(dev), torch.zeros(805, dtype=torch.bool, device=dev)).sum()) == 0
