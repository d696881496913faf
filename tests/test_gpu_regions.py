"""Regions on the GPU (csrc/regions.hip) against the contract in numpy float32 (regions_ref): sim, live, labels and sizes EXACTLY, NaN
positions included, no tolerance.  N <= 4096 everywhere; every case runs twice and the two runs give identical tensors; a union-find
loop that reached its trip cap (status != 0) raises, so every passing call also says that status stayed 0."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import regions

import components_ref as cref
import regions_ref as ref

pytestmark = pytest.mark.gpu
F = np.float32
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:  # a reference is computed once, shared, and left unchanged
        _CACHE[key] = make()
    return _CACHE[key]


def same(x, y):
    """Identical tensors, NaN positions included."""
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    if not x.is_floating_point():
        return torch.equal(x, y)
    return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0))


def twice(fn):
    """fn() run two times: the tensors of the two results (a tuple or a Components) are identical; returns the first."""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert same(x, y)
    return a


def field(n, d, seed, dead=True):
    """Rows around four directions (so that the cosines spread over (-1, 1)), with a zero row, a NaN row and an infinite row."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((4, d))[rng.integers(0, 4, n)] + 0.7 * rng.standard_normal((n, d))).astype(F)
    if dead and n > 12:
        X[5] = 0.0
        X[9, d // 2] = np.nan
        X[11, 0] = np.inf
    return X


def lists(n, k, seed):
    idx = ref.random_lists(n, k, seed)
    idx[np.random.default_rng(seed + 1).random(idx.shape) < 0.05] = -1
    return idx


def on(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_case(dev, X, idx, want, *, feats=None, dist=None, group=None, mask=None, sim_min=0.3, radius=None):
    """neighbor_similarity and similarity_components, each twice, against the reference's dict."""
    n = idx.shape[0]
    f = on(dev, X) if feats is None else feats
    tidx = on(dev, idx)
    sim, live = twice(lambda: gsbp_amd.neighbor_similarity(f, tidx))
    assert sim.dtype == torch.float32 and live.dtype == torch.bool
    assert ref.same_bits(sim.cpu().numpy(), want["sim"]) and np.array_equal(live.cpu().numpy(), want["live"])
    means = torch.zeros(n, 3, device=dev)  # (not looked at when the neighbours are given)
    res = twice(lambda: gsbp_amd.similarity_components(means, f, sim_min=sim_min, radius=radius, group=on(dev, group), mask=on(dev, mask),
                                                       neighbors=(on(dev, dist), tidx)))
    assert res.labels.dtype == torch.int32 and res.sizes.dtype == torch.int64 and res.core.dtype == torch.bool
    assert np.array_equal(res.labels.cpu().numpy(), want["labels"]) and np.array_equal(res.sizes.cpu().numpy(), want["sizes"])
    assert np.array_equal(res.core.cpu().numpy(), want["core"])
    return res


@pytest.mark.parametrize("d", [1, 3, 64, 255, 256, 260, 2048])
def test_every_width_equals_the_reference(dev, d):
    """Lanes without channels (1, 3, 64), the tail step (255, 256, 260), all eight steps (2048); 257 rows: 65 workgroups, the last
    one with a single wave at work."""
    n, k = 257, 8
    X, idx = field(n, d, d), lists(n, k, d)
    want = cached(("width", d), lambda: ref.components(X, idx, sim_min=0.3))
    res = run_case(dev, X, idx, want)
    assert int(res.sizes.numel()) > 1 and int((res.labels < 0).sum()) >= 3


def test_the_element_wise_path_equals_the_reference(dev):
    """D = 514 at a row stride of 515 floats from a base one float past an aligned address: no row is 16-B aligned."""
    n, k, d = 257, 8, 514
    X, idx = field(n, d, 77), lists(n, k, 77)
    want = cached("strided", lambda: ref.components(X, idx, sim_min=0.3))
    base = torch.zeros(n * 515 + 1, device=dev)
    f = base[1:].view(n, 515)[:, :d]
    f.copy_(on(dev, X))
    assert f.data_ptr() % 16 == 4 and f.stride(0) == 515
    run_case(dev, X, idx, want, feats=f)
    run_case(dev, X, idx, want)  # and the 16-B path of the same field: the same bits


@pytest.mark.parametrize("k", [1, 16, 64])
def test_every_list_length_equals_the_reference(dev, k):
    n, d = 130, 70
    X, idx = field(n, d, k), lists(n, k, 100 + k)
    want = cached(("k", k), lambda: ref.components(X, idx, sim_min=0.5))
    run_case(dev, X, idx, want, sim_min=0.5)


def test_special_entries_and_a_one_directional_list(dev):
    """-1, >= N, self and repeated entries; 7 lists 2 but 2 does not list 7, and they are joined all the same."""
    X = np.ones((8, 5), F)
    X[3] = 0.0
    X[5, 2] = np.nan
    idx = np.array([[1, -1, 1], [0, 1, 0], [8, 2, 2], [2, 4, 4], [3, 6, 3], [4, 6, 6], [7, 7, 7], [7, 2, 2]], np.int32)
    group = np.array([0, 0, 0, 0, 0, 0, -1, 0], np.int32)
    want = ref.components(X, idx, group=group, sim_min=0.99)
    assert want["root"].tolist() == [0, 0, 2, -1, 4, -1, -1, 2]
    res = run_case(dev, X, idx, want, group=group, sim_min=0.99)
    assert res.labels.tolist() == [0, 0, 1, -1, 2, -1, -1, 1]
    mask = group >= 0
    run_case(dev, X, idx, ref.components(X, idx, group=np.where(mask, 0, -1), sim_min=0.99), mask=mask, sim_min=0.99)
    other = np.array([0, 1, 0, 0, 0, 0, 0, 2], np.int32)
    run_case(dev, X, idx, ref.components(X, idx, group=other, sim_min=0.99), group=other, sim_min=0.99)


@pytest.mark.parametrize("t", [0.5, 0.75])
def test_the_tie_set_at_a_threshold_on_the_tie(dev, t):
    X, idx = ref.binary_rows(), ref.random_lists(96, 6, 1)
    want = cached(("tie", t), lambda: ref.components(X, idx, sim_min=t))
    assert int((want["sim"] == F(t)).sum()) >= 2
    run_case(dev, X, idx, want, sim_min=t)


def test_a_chain_of_2048_is_one_component_and_breaks_at_a_zero_row(dev):
    """Every point lists only its successor and all rows are identical: the deepest parent chain the union can build."""
    n = 2048
    means = torch.zeros(n, 3, device=dev)
    means[:, 0] = torch.arange(n, device=dev)
    idx = torch.arange(1, n + 1, dtype=torch.int32, device=dev).reshape(n, 1)  # (the last entry is n: no neighbour)
    row = torch.from_numpy(field(1, 48, 3, dead=False)).to(dev)
    f = row.repeat(n, 1)
    res = twice(lambda: gsbp_amd.similarity_components(means, f, sim_min=0.999, neighbors=(None, idx)))
    assert res.labels.tolist() == [0] * n and res.sizes.tolist() == [n] and bool(res.core.all())
    f[1000] = 0.0
    res = twice(lambda: gsbp_amd.similarity_components(means, f, sim_min=0.999, neighbors=(None, idx)))
    assert res.labels.tolist() == [0] * 1000 + [-1] + [1] * 1047 and res.sizes.tolist() == [1000, 1047]
    assert res.core.tolist() == [True] * 1000 + [False] + [True] * 1047


def scene(dev, n=1000):
    means = torch.rand(n, 3, generator=torch.Generator().manual_seed(11))
    feats, sets, _ = regions.synthetic_regions(means, d=64, noise=0.5)
    return means.to(dev), feats.to(dev), sets


def test_the_search_s_own_lists_groups_masks_and_the_cut(dev):
    means, feats, _ = scene(dev)
    n = means.shape[0]
    res, sim, (dist, idx) = gsbp_amd.similarity_components(means, feats, k=8, sim_min=0.8, return_similarity=True)
    again = gsbp_amd.similarity_components(means, feats, k=8, sim_min=0.8, return_similarity=True)
    assert all(same(x, y) for x, y in zip((*res[:3], sim, dist, idx), (*again[0][:3], again[1], *again[2])))
    d2, i2 = gsbp_amd.spatial_knn(means, 9)
    assert idx.shape == (n, 9) and torch.equal(idx, i2) and torch.equal(dist, d2)
    X, I, Dm = feats.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
    sl = cached("scene-sim", lambda: ref.similarity(X, I))
    assert ref.same_bits(sim.cpu().numpy(), sl[0])
    run_case(dev, X, I, ref.components(X, I, sim_min=0.8, sim_live=sl), dist=Dm, sim_min=0.8)
    assert np.array_equal(res.labels.cpu().numpy(), ref.components(X, I, sim_min=0.8, sim_live=sl)["labels"])
    # the cut at a distance that occurs in the list: dist == max_dist passes
    # (the first such distance from the median of the fifth column on whose own edges matter to the labels)
    for cut in np.sort(Dm[:, 4])[n // 2: n // 2 + 50].tolist():
        want = ref.components(X, I, dist=Dm, sim_min=0.8, max_dist=cut, sim_live=sl)
        below = ref.components(X, I, dist=Dm, sim_min=0.8, max_dist=np.nextafter(F(cut), F(0)), sim_live=sl)
        if not np.array_equal(want["labels"], below["labels"]):
            break
    else:
        raise AssertionError("no distance of the list decides a label")
    run_case(dev, X, I, want, dist=Dm, sim_min=0.8, radius=cut)
    # groups and a mask
    rng = np.random.default_rng(4)
    group = rng.integers(-1, 3, n).astype(np.int32)
    run_case(dev, X, I, ref.components(X, I, group=group, sim_min=0.8, sim_live=sl), group=group, sim_min=0.8)
    mask = rng.random(n) < 0.7
    run_case(dev, X, I, ref.components(X, I, group=np.where(mask, 0, -1), sim_min=0.8, sim_live=sl), mask=mask, sim_min=0.8)
    # min_size: the small regions become -1, the others keep their order
    big = twice(lambda: gsbp_amd.similarity_components(means, feats, sim_min=0.8, neighbors=(dist, idx), min_size=5))
    keep = (res.sizes >= 5)
    assert torch.equal(big.sizes, res.sizes[keep]) and int(keep.sum()) < res.sizes.numel()
    renum = torch.full((res.sizes.numel() + 1,), -1, dtype=torch.int32, device=dev)
    renum[:-1][keep] = torch.arange(int(keep.sum()), dtype=torch.int32, device=dev)
    assert torch.equal(big.labels, renum[res.labels.long()])


def test_levels_are_nested_and_equal_separate_calls(dev):
    means, feats, _ = scene(dev)
    nb = gsbp_amd.spatial_knn(means, 9)
    ts = [0.5, 0.7, 0.8, 0.9]
    levels, = twice(lambda: (gsbp_amd.similarity_levels(means, feats, ts, neighbors=nb),))
    assert levels.shape == (4, means.shape[0]) and levels.dtype == torch.int32
    for row, t in zip(levels, ts):
        assert torch.equal(row, gsbp_amd.similarity_components(means, feats, sim_min=t, neighbors=nb).labels)
    given = gsbp_amd.neighbor_similarity(feats, nb[1])  # the pass handed in: the same labels without a second [N, D] pass
    assert torch.equal(levels, gsbp_amd.similarity_levels(means, feats, ts, neighbors=nb, similarity=given))
    assert torch.equal(levels[2], gsbp_amd.similarity_components(means, feats, sim_min=0.8, neighbors=nb, similarity=given).labels)
    lv = levels.cpu().numpy()
    for fine, coarse in zip(lv[1:], lv[:-1]):
        live = fine >= 0
        assert np.array_equal(live, coarse >= 0)
        pairs = set(zip(fine[live].tolist(), coarse[live].tolist()))
        assert len(pairs) == len({a for a, _ in pairs}) and fine.max() >= coarse.max()  # every finer region lies in ONE coarser
    assert lv[-1].max() > lv[0].max()


def test_radius_components_on_the_same_means_is_unchanged(dev):
    """The union-find moved into a shared header; the radius components still equal their brute-force reference."""
    means, _, _ = scene(dev)
    p = means.cpu().numpy()
    for min_points in (1, 4):
        want = cached(("radius", min_points), lambda: cref.components(p, 0.08, min_points))
        got = twice(lambda: gsbp_amd.radius_components(means, 0.08, min_points))
        assert np.array_equal(got.labels.cpu().numpy(), want["labels"]) and np.array_equal(got.sizes.cpu().numpy(), want["sizes"])
        assert np.array_equal(got.core.cpu().numpy(), want["core"])


def test_region_prompt_mask_is_the_composition_and_constant_per_region(dev):
    means = torch.rand(1000, 3, generator=torch.Generator().manual_seed(11))
    feats, sets, _ = regions.synthetic_regions(means, d=64)
    means, feats = means.to(dev), feats.to(dev)
    labels = twice(lambda: gsbp_amd.similarity_components(means, feats, sim_min=0.9)).labels
    c = int(labels.max()) + 1
    prompts = torch.stack([feats[sets.to(dev) == 2].mean(0), feats[sets.to(dev) == 0].mean(0), feats[sets.to(dev) == 1].mean(0)])
    got, = twice(lambda: (gsbp_amd.region_prompt_mask(feats, labels, prompts, 1),))
    protos, _ = gsbp_amd.class_prototypes(feats, labels, c)
    assert got.dtype == torch.bool and torch.equal(got, gsbp_amd.codebook_prompt_mask(protos, labels, prompts, 1))
    per = torch.zeros(c, dtype=torch.int64, device=dev).index_add_(0, labels[labels >= 0].long(), got[labels >= 0].long())
    sizes = torch.bincount(labels[labels >= 0].long(), minlength=c)
    assert bool(((per == 0) | (per == sizes)).all()) and not bool(got[labels < 0].any())
    in_balls = (sets.to(dev) >= 2)
    assert int(got.sum()) > 0 and bool(in_balls[got].all())  # the prompt of the balls' prototype selects regions of the balls only


def test_edge_strength_equals_numpy(dev):
    means, feats, sets = scene(dev)
    idx = gsbp_amd.spatial_knn(means, 9)[1]
    sim, live = twice(lambda: gsbp_amd.neighbor_similarity(feats, idx))
    for how in ("min", "mean"):
        e = gsbp_amd.regions.edge_strength(sim, how)
        assert e.shape == (means.shape[0],) and not bool(torch.isnan(e).any()) and bool((e[~live] == 0).all())
    want = 1.0 - np.nanmin(np.where(np.isnan(sim.cpu().numpy()), np.inf, sim.cpu().numpy()), axis=1)
    got = gsbp_amd.regions.edge_strength(sim).cpu().numpy()
    rows = live.cpu().numpy() & np.isfinite(want)
    assert np.array_equal(got[rows], want[rows].astype(F))
