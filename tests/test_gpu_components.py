"""Radius components on the GPU (csrc/components.hip) against the brute-force reference in the contract's own fp32 arithmetic
(components_ref): labels, sizes, core and counts, exactly, whatever the grid; and the instance layer on top.  N <= 4096 everywhere;
every case runs twice and the two runs give identical tensors."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import spatial
from gsbp_amd._lib import GwbpError

import components_ref as cref
import spatial_ref as ref

pytestmark = pytest.mark.gpu

OFFSETS = (0.0, 1024.0)
_CACHE = {}


def thinned(off, keep=0.33, seed=3):
    lat = ref.lattice(16, 0, off)
    return lat[np.random.default_rng(seed).random(len(lat)) < keep]


def cached(key, make):
    if key not in _CACHE:  # a reference is computed once, shared, and left unchanged
        _CACHE[key] = make()
    return _CACHE[key]


def twice(fn):
    """fn() run two times: the results (a tensor, or a tuple whose tensors count) are identical; returns the first."""
    a, b = fn(), fn()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        if torch.is_tensor(x):
            assert x.dtype == y.dtype and torch.equal(x, y)
    return a


def check(got, want):
    assert got.labels.dtype == torch.int32 and got.sizes.dtype == torch.int64 and got.core.dtype == torch.bool
    assert np.array_equal(got.core.cpu().numpy(), want["core"])
    assert np.array_equal(got.labels.cpu().numpy(), want["labels"])
    assert np.array_equal(got.sizes.cpu().numpy(), want["sizes"])


def components(dev, pts, radius, min_points=1, **kw):
    kw = {k: (torch.from_numpy(np.asarray(v)).to(dev) if k in ("group", "mask") and v is not None else v) for k, v in kw.items()}
    t = pts if torch.is_tensor(pts) else torch.from_numpy(pts).to(dev)
    return twice(lambda: gsbp_amd.radius_components(t, radius, min_points, **kw))


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("radius", [1.0 / 16.0, 0.09])
@pytest.mark.parametrize("min_points", [1, 3, 4, 6])
def test_thinned_lattice_equals_the_reference_whatever_the_grid(dev, min_points, radius, off):
    """The automatic grid, one cell, cells of 1/16 (points on cell faces; with the offset, at 2^10 times the cell size) and cells of
    radius / 8 (many rings): each equals the reference, hence each other.  At radius 1/16, d2 == r2 occurs exactly."""
    pts = thinned(off)
    want = cached(("thin", off, radius, min_points), lambda: cref.components(pts, radius, min_points))
    for cell in (None, 1e6, 1.0 / 16.0, radius / 8.0):
        check(components(dev, pts, radius, min_points, cell_size=cell), want)
        count = twice(lambda: gsbp_amd.radius_count(torch.from_numpy(pts).to(dev), radius, cell_size=cell))
        assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), want["count"])


def test_full_lattice_under_a_radius_that_covers_everything_is_one_component(dev):
    pts = ref.lattice(16, 0, 0.0)
    for min_points, cell in ((1, None), (4096, None), (1, 1.0 / 16.0)):  # every lane hooks towards index 0
        got = components(dev, pts, 100.0, min_points, cell_size=cell)
        assert got.sizes.tolist() == [4096] and bool((got.labels == 0).all()) and bool(got.core.all())
    got = components(dev, pts, 100.0, 4097)
    assert got.sizes.numel() == 0 and bool((got.labels == -1).all()) and not bool(got.core.any())


def test_chain(dev):
    """2048 collinear points at spacing 1/16 in permuted order: the deepest parent chains, over 16 workgroups."""
    pos = np.random.default_rng(5).permutation(2048)
    pts = np.zeros((2048, 3), np.float32)
    pts[:, 0] = pos / 16.0
    for cell in (None, 1.0 / 16.0, 1e6):
        one = components(dev, pts, 1.0 / 16.0, cell_size=cell)
        assert one.sizes.tolist() == [2048] and bool((one.labels == 0).all())
        none = components(dev, pts, 0.99 / 16.0, cell_size=cell)
        assert none.sizes.tolist() == [1] * 2048 and none.labels.tolist() == list(range(2048))
        eight = components(dev, pts, 1.0 / 16.0, group=(pos // 256).astype(np.int32), cell_size=cell)
        check(eight, cached("chain8", lambda: cref.components(pts, 1.0 / 16.0, group=pos // 256)))
        assert eight.sizes.tolist() == [256] * 8
        check(components(dev, pts, 1.0 / 16.0, 3, cell_size=cell), cached("chain3", lambda: cref.components(pts, 1.0 / 16.0, 3)))
    srt = np.zeros((2048, 3), np.float32)  # in index order every hook is i -> i - 1: the longest chain a find can meet
    srt[:, 0] = np.arange(2048) / 16.0
    assert components(dev, srt, 1.0 / 16.0).sizes.tolist() == [2048]


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("name", ["duplicates", "identical"])
def test_radius_zero_joins_exact_duplicates(dev, name, off):
    pts = ref.lattice_sets(8, off)[name]
    for min_points in (1, 2, 3):
        want = cached((name, off, min_points), lambda: cref.components(pts, 0.0, min_points))
        for cell in (None, 1.0 / 16.0):
            check(components(dev, pts, 0.0, min_points, cell_size=cell), want)
    if name == "duplicates":
        assert cached((name, off, 2), None)["sizes"].tolist() == [2] * 512 and cached((name, off, 3), None)["sizes"].size == 0


@pytest.mark.parametrize("off", OFFSETS)
def test_floaters_in_border_cells_are_noise(dev, off):
    """Ten floaters at +-1024 around two 3^3 clusters.  The set draws two of its floaters twice, so at min_points = 2 the six single
    ones are noise and the two pairs are components of two; at min_points = 3 all ten are noise."""
    pts = ref.lattice_sets(8, off)["clusters_floaters"]
    far = (np.abs(pts - off) > 100).any(axis=1)
    assert far.sum() == 10
    single = far & (cref.radius_count_ref(pts, 0.0) == 1)
    want2 = cached(("floaters", off, 2), lambda: cref.components(pts, 0.5, 2))
    want3 = cached(("floaters", off, 3), lambda: cref.components(pts, 0.5, 3))
    assert single.sum() == 6 and (want2["labels"][single] == -1).all() and sorted(want2["sizes"].tolist()) == [2, 2, 27, 27]
    assert (want3["labels"][far] == -1).all() and want3["sizes"].tolist() == [27, 27]
    for cell in (None, 0.5, 1e6):
        check(components(dev, pts, 0.5, 2, cell_size=cell), want2)
        check(components(dev, pts, 0.5, 3, cell_size=cell), want3)
    alone = components(dev, pts, 0.5, 1)
    assert alone.sizes.tolist().count(1) == 6


@pytest.mark.parametrize("min_points", [1, 5])
def test_random_floats_equal_the_reference_bit_for_bit(dev, min_points):
    """The contract is written in fp32, so there is no band: any radius, exact equality."""
    pts = spatial.clustered_points(4096).numpy()
    radius = 0.0123
    want = cached(("random", min_points), lambda: cref.components(pts, radius, min_points))
    assert 10 < want["sizes"].size < 4096 and (min_points == 1 or want["border"].sum() > 10)
    for cell in (None, radius / 4.0):
        check(components(dev, pts, radius, min_points, cell_size=cell), want)
    count = twice(lambda: gsbp_amd.radius_count(torch.from_numpy(pts).to(dev), radius))
    assert np.array_equal(count.cpu().numpy(), want["count"])


def test_groups_masks_non_finite_rows_and_a_strided_view(dev):
    a = thinned(0.0)
    b = (thinned(0.0, seed=4) + np.float32(1.0 / 32.0)).astype(np.float32)  # a second lattice inside the first, sqrt(3)/32 away
    pts = np.concatenate([a, b])
    group = np.concatenate([np.zeros(len(a), np.int32), np.full(len(b), 7, np.int32)])
    order = np.random.default_rng(6).permutation(len(pts))
    pts, group = pts[order], group[order]
    for min_points in (1, 4):
        want = cached(("groups", min_points), lambda: cref.components(pts, 1.0 / 16.0, min_points, group=group))
        got = components(dev, pts, 1.0 / 16.0, min_points, group=group)
        check(got, want)
        lab = got.labels.cpu().numpy()
        for c in range(want["sizes"].size):  # two groups never merge
            assert np.unique(group[lab == c]).size == 1
        merged = cached(("nogroups", min_points), lambda: cref.components(pts, 1.0 / 16.0, min_points))
        assert merged["sizes"].size < want["sizes"].size
        check(components(dev, pts, 1.0 / 16.0, min_points), merged)
    # a mask is the group where(mask, 0, -1); a negative group excludes
    mask = group == 7
    want = cached("mask", lambda: cref.components(pts, 1.0 / 16.0, 3, mask=mask))
    got = components(dev, pts, 1.0 / 16.0, 3, mask=mask)
    check(got, want)
    check(components(dev, pts, 1.0 / 16.0, 3, group=np.where(mask, 0, -1)), want)
    assert bool((got.labels.cpu()[torch.from_numpy(~mask)] == -1).all())
    with pytest.raises(GwbpError, match="not both"):
        gsbp_amd.radius_components(torch.from_numpy(pts).to(dev), 0.1, group=torch.zeros(len(pts), dtype=torch.int32), mask=torch.from_numpy(mask))
    # non-finite rows are -1 and join nothing
    bad = pts.copy()
    rows = [3, 17, 30, len(pts) - 1]
    bad[3, 1], bad[17, 0], bad[30, 2], bad[-1] = np.nan, np.inf, -np.inf, np.nan
    want = cached("bad", lambda: cref.components(bad, 1.0 / 16.0, 2, group=group))
    got = components(dev, bad, 1.0 / 16.0, 2, group=group)
    check(got, want)
    assert (got.labels.cpu().numpy()[rows] == -1).all() and not got.core.cpu().numpy()[rows].any()
    count = gsbp_amd.radius_count(torch.from_numpy(bad).to(dev), 1.0 / 16.0, group=torch.from_numpy(group).to(dev))
    assert np.array_equal(count.cpu().numpy(), want["count"]) and (count.cpu().numpy()[rows] == 0).all()
    # a strided [:, :3] view of a [N, 7] tensor is read in place
    wide = torch.zeros(len(pts), 7)
    wide[:, :3] = torch.from_numpy(pts)
    wide[:, 3:] = 99.0
    view = wide.to(dev)[:, :3]
    assert not view.is_contiguous()
    check(components(dev, view, 1.0 / 16.0, 4, group=group), cached(("groups", 4), None))


def test_radius_count_with_separate_queries_caps_and_query_groups(dev):
    pts = thinned(1024.0)
    rng = np.random.default_rng(9)
    q = np.concatenate([ref.lattice(16, 1, 1024.0)[:300], (1024.0 + rng.random((40, 3)) * 40.0 - 20.0).astype(np.float32),
                        np.array([[1e4, -3e3, 0.5], [np.nan, 1024.0, 1024.0], [1024.5, np.inf, 1024.5]], np.float32)])
    group = rng.integers(-1, 3, len(pts)).astype(np.int32)
    qgroup = rng.integers(-1, 3, len(q)).astype(np.int32)
    P, Q = torch.from_numpy(pts).to(dev), torch.from_numpy(q).to(dev)
    G, QG = torch.from_numpy(group).to(dev), torch.from_numpy(qgroup).to(dev)
    for radius in (1.0 / 16.0, 0.2):
        for cell in (None, 1.0 / 16.0, 1e6):
            got = twice(lambda: gsbp_amd.radius_count(P, radius, Q, cell_size=cell))
            assert got.shape == (len(q),) and np.array_equal(got.cpu().numpy(), cref.radius_count_ref(pts, radius, q))
            assert got[-3:].tolist() == [0, 0, 0]
            got = twice(lambda: gsbp_amd.radius_count(P, radius, Q, group=G, query_group=QG, cell_size=cell))
            want = cref.radius_count_ref(pts, radius, q, group, qgroup)
            assert np.array_equal(got.cpu().numpy(), want) and (want[qgroup < 0] == 0).all() and want.max() >= 2
            for cap in (1, 3):
                got = twice(lambda: gsbp_amd.radius_count(P, radius, Q, group=G, query_group=QG, cap=cap, cell_size=cell))
                assert np.array_equal(got.cpu().numpy(), np.minimum(want, cap))
    got = gsbp_amd.radius_count(P, 0.2, group=G, cap=5)
    assert np.array_equal(got.cpu().numpy(), cref.radius_count_ref(pts, 0.2, None, group, None, 5))
    with pytest.raises(GwbpError, match="query_group"):
        gsbp_amd.radius_count(P, 0.2, query_group=QG)


def test_small_sizes(dev):
    empty = gsbp_amd.radius_components(torch.zeros(0, 3, device=dev), 0.5)
    assert empty.labels.shape == (0,) and empty.sizes.shape == (0,) and empty.core.shape == (0,) and empty.labels.dtype == torch.int32
    assert gsbp_amd.radius_count(torch.zeros(0, 3, device=dev), 0.5).shape == (0,)
    assert gsbp_amd.radius_count(torch.zeros(0, 3, device=dev), 0.5, torch.zeros(5, 3, device=dev)).tolist() == [0] * 5
    assert gsbp_amd.radius_count(torch.zeros(5, 3, device=dev), 0.5, torch.zeros(0, 3, device=dev)).shape == (0,)
    one = torch.tensor([[0.25, 1.0, -3.0]], device=dev)
    for radius in (0.0, 0.5):
        got = twice(lambda: gsbp_amd.radius_components(one, radius))
        assert got.labels.tolist() == [0] and got.sizes.tolist() == [1] and got.core.tolist() == [True]
    got = gsbp_amd.radius_components(one, 0.5, 2)
    assert got.labels.tolist() == [-1] and got.sizes.shape == (0,) and got.core.tolist() == [False]
    pts = torch.from_numpy(ref.lattice(8, 0, 0.0)).to(dev)
    n = pts.shape[0]
    for kw in (dict(mask=torch.zeros(n, dtype=torch.bool, device=dev)), dict(group=torch.full((n,), -5, dtype=torch.int64, device=dev))):
        got = twice(lambda: gsbp_amd.radius_components(pts, 1.0, **kw))
        assert bool((got.labels == -1).all()) and got.sizes.shape == (0,) and not bool(got.core.any())
    got = twice(lambda: gsbp_amd.radius_components(pts, 100.0, n + 1))  # min_points > N: everything is noise
    assert bool((got.labels == -1).all()) and got.sizes.shape == (0,) and not bool(got.core.any())
    stats = gsbp_amd.radius_components(pts, 1.0 / 16.0, return_stats=True).grid_stats
    assert stats["points_in_cells"] == n and stats["cell_size"] >= 1.0 / 16.0 and stats["cells"] == int(np.prod(stats["dims"]))


def test_split_instances_and_select_components_on_three_balls_and_floaters(dev):
    g = torch.Generator().manual_seed(21)
    centres = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0, -0.5]])
    sizes = (900, 600, 300)
    balls = [c + 0.1 * (torch.rand(m, 3, generator=g) - 0.5) for c, m in zip(centres, sizes)]
    floaters = torch.tensor([[5.0, 5.0, 5.0], [-4.0, 2.0, 0.0], [0.5, 0.5, 6.0], [9.0, -9.0, 1.0], [0.5, 3.0, 0.25], [0.5, 3.0, 0.27]])
    rest = torch.rand(700, 3, generator=g) * 2.0 - 0.5  # Gaussians outside the mask, some of them inside the balls
    pts = torch.cat(balls + [floaters, rest])
    truth = torch.cat([torch.full((m,), b) for b, m in enumerate(sizes)] + [torch.full((6,), -1), torch.full((700,), -1)])
    mask = torch.cat([torch.ones(1806, dtype=torch.bool), torch.zeros(700, dtype=torch.bool)])
    perm = torch.randperm(pts.shape[0], generator=g)
    pts, truth, mask = pts[perm].to(dev), truth[perm].to(dev), mask[perm].to(dev)
    inst = twice(lambda: tuple(gsbp_amd.split_instances(pts, mask, radius=0.05, min_size=3)))
    inst = gsbp_amd.components.Instances(*inst)
    assert inst.instances.dtype == torch.int32 and torch.equal(inst.instances, truth.to(torch.int32))  # balls 0 .. 2 by size, the rest -1
    assert inst.sizes.tolist() == list(sizes) and inst.classes.tolist() == [0, 0, 0] and inst.radius == 0.05
    keep_all = gsbp_amd.split_instances(pts, mask, radius=0.05)
    assert keep_all.sizes.tolist() == list(sizes) + [2] + [1] * 4          # the floaters: a pair and four singles
    ball2 = int(torch.nonzero(truth == 2)[0])
    assert torch.equal(gsbp_amd.select_components(inst, seeds=[ball2]), truth == 2)
    assert torch.equal(gsbp_amd.select_components(inst, largest=2), (truth == 0) | (truth == 1))
    assert torch.equal(gsbp_amd.select_components(keep_all, min_size=3), truth >= 0)
    # the automatic radius finds the same instances; as labels, two balls of one class and one of another
    auto = gsbp_amd.split_instances(pts, mask, min_size=10)
    assert 0.0 < auto.radius < 0.2 and torch.equal(auto.instances, truth.to(torch.int32))
    labels = torch.where(truth == 1, 4, torch.where(truth >= 0, 1, -1))
    by_class = gsbp_amd.split_instances(pts, labels, radius=0.05, min_size=3, num_classes=6)
    assert torch.equal(by_class.instances, truth.to(torch.int32)) and by_class.classes.tolist() == [1, 4, 1]
    assert gsbp_amd.suggest_radius(pts, mask=mask) == auto.radius
