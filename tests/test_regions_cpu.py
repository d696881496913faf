"""Regions without a GPU: the float32 reference of the contract (regions_ref) against an independent float64 formulation where the two
agree exactly; the contract's properties on the reference; the seeded planted regions; the C ABI's validation; the symbols; the
command line's parser.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib, regions
from gsbp_amd._lib import GwbpError

import regions_ref as ref

F = np.float32


# ---- an independent formulation: float64 cosines, a breadth-first search ---------------------------------------------------------------

def cos64(X):
    X = np.asarray(X, np.float64)
    nrm = np.sqrt((X * X).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (X @ X.T) / np.outer(nrm, nrm), nrm


def labels64(X, idx, sim_min, group=None, dist=None, max_dist=np.inf):
    """Components by breadth-first search over the symmetrised edge lists, numbered in the order of their first (smallest) member."""
    n, k = idx.shape
    cos, nrm = cos64(X)
    grp = np.zeros(n, int) if group is None else np.asarray(group)
    live = np.isfinite(nrm) & (nrm >= 1e-12) & (grp >= 0)
    adj = [[] for _ in range(n)]
    for i in range(n):
        for c in range(k):
            j = int(idx[i, c])
            if 0 <= j < n and j != i and live[i] and live[j] and grp[i] == grp[j] and cos[i, j] >= sim_min \
                    and (dist is None or dist[i, c] <= max_dist):
                adj[i].append(j)
                adj[j].append(i)
    labels, nxt = np.full(n, -1, np.int32), 0
    for s in range(n):
        if not live[s] or labels[s] >= 0:
            continue
        labels[s], todo = nxt, [s]
        while todo:
            for v in adj[todo.pop()]:
                if labels[v] < 0:
                    labels[v] = nxt
                    todo.append(v)
        nxt += 1
    return labels


binary_rows, random_lists = ref.binary_rows, ref.random_lists


def test_reference_equals_float64_on_exact_cosines_with_ties():
    """sim == sim_min occurs exactly (0.75 = 3/4 = 6/8 = 12/16; 0.5 likewise), so the >= is on trial."""
    X, idx = binary_rows(), random_lists(96, 6, 1)
    sim, live = ref.similarity(X, idx)
    cos, _ = cos64(X)
    assert live.all() and np.array_equal(sim.astype(np.float64), cos[np.arange(96)[:, None], idx])
    for t in (0.5, 0.75):
        assert int((sim == F(t)).sum()) >= 2, t  # the tie is there
        got = ref.components(X, idx, sim_min=t)
        assert np.array_equal(got["labels"], labels64(X, idx, t))
        assert not np.array_equal(got["labels"], labels64(X, idx, np.nextafter(t, 2.0)))  # and it matters
    assert ref.components(X, idx, sim_min=0.5)["sizes"].max() > 4


@pytest.mark.parametrize("d", [3, 70, 300])
def test_reference_equals_float64_on_random_rows_inside_a_gap(d):
    rng = np.random.default_rng(d)
    n, k = 120, 5
    protos = rng.standard_normal((4, d))
    X = (protos[rng.integers(0, 4, n)] + 0.6 * rng.standard_normal((n, d))).astype(F)
    X[7] = 0.0
    idx = random_lists(n, k, d + 1)
    cos, _ = cos64(X)
    pair = np.sort(cos[np.arange(n)[:, None], idx].ravel())
    pair = pair[np.isfinite(pair)]
    mid = pair[len(pair) // 2: 9 * len(pair) // 10]
    at = int(np.argmax(np.diff(mid)))
    assert mid[at + 1] - mid[at] > 1e-4  # wider than any float32 rounding of a cosine by orders of magnitude
    t = float(F(0.5 * (mid[at] + mid[at + 1])))
    got = ref.components(X, idx, sim_min=t)
    assert np.array_equal(got["labels"], labels64(X, idx, t)) and got["labels"][7] == -1
    assert len(got["sizes"]) < n and (pair < t).any() and (pair > t).any() and np.abs(got["sim"][~np.isnan(got["sim"])] - cos[np.arange(n)[:, None], idx][~np.isnan(got["sim"])]).max() < 1e-5


# ---- properties of the contract, on the reference ---------------------------------------------------------------------------------------

def test_similarity_is_symmetric_bit_for_bit():
    rng = np.random.default_rng(5)
    n, d = 64, 300
    X = rng.standard_normal((n, d)).astype(F)
    idx = np.stack([(np.arange(n) + 1) % n, (np.arange(n) - 1) % n], axis=1).astype(np.int32)  # i lists i + 1 and i - 1
    sim, _ = ref.similarity(X, idx)
    assert ref.same_bits(sim[:, 0], np.roll(sim[:, 1], -1))  # sim(i, i + 1) from row i and from row i + 1
    assert ref.same_bits(ref.dots(X, X[::-1]), ref.dots(X[::-1], X)[::-1])


def test_levels_are_nested():
    X, _, _ = (t.numpy() for t in regions.synthetic_regions(torch.rand(600, 3, generator=torch.Generator().manual_seed(2)), d=16, noise=0.6))
    idx = random_lists(600, 4, 9)
    sl = ref.similarity(X, idx)
    prev = None
    for t in (0.2, 0.5, 0.7, 0.9):
        lab = ref.components(X, idx, sim_min=t, sim_live=sl)["labels"]
        if prev is not None:
            live = lab >= 0
            assert np.array_equal(live, prev >= 0)
            pairs = set(zip(lab[live].tolist(), prev[live].tolist()))
            assert len(pairs) == len({a for a, _ in pairs})  # every finer region lies inside ONE coarser region
            assert lab.max() >= prev.max()
        prev = lab
    assert prev.max() > 3


def test_special_entries_behave_as_the_contract_says():
    X = np.ones((8, 5), F)
    X[3] = 0.0          # a zero row: dead
    X[5, 2] = np.nan    # a NaN row: dead
    idx = np.array([[1, -1], [0, 1], [8, 2], [2, 4], [3, 6], [4, 6], [7, 7], [7, 2]], np.int32)
    group = np.array([0, 0, 0, 0, 0, 0, -1, 0])
    got = ref.components(X, idx, group=group, sim_min=0.99)
    sim, live = got["sim"], got["live"]
    assert live.tolist() == [True, True, True, False, True, False, True, True]
    assert got["core"].tolist() == [True, True, True, False, True, False, False, True]  # 6: feature-live, excluded by its group
    assert np.isnan(sim[0, 1]) and np.isnan(sim[2, 0])       # -1 and >= N: no neighbour
    assert np.isnan(sim[3]).all() and np.isnan(sim[4, 0]) and np.isnan(sim[5]).all()  # a dead row on either side
    assert sim[1, 1] == sim[0, 0] and not np.isnan(sim[6, 0])  # a self entry has a similarity like any other ...
    # ... and is ignored by the union: 0 - 1 by 0's list; 2 - 7 by 7's list alone; 4 lists only dead or excluded rows
    assert got["root"].tolist() == [0, 0, 2, -1, 4, -1, -1, 2]
    assert got["labels"].tolist() == [0, 0, 1, -1, 2, -1, -1, 1] and got["sizes"].tolist() == [2, 2, 1]
    # different groups never join, the same lists otherwise
    assert ref.components(X, idx, group=np.array([0, 1, 0, 0, 0, 0, 0, 2]), sim_min=0.99)["root"].tolist() == [0, 1, 2, -1, 4, -1, 4, 7]
    # the cut: dist == max_dist passes, the next float does not
    dist = np.full(idx.shape, 0.5, F)
    assert ref.components(X, idx, dist=dist, sim_min=0.99, max_dist=0.5)["root"].tolist()[:2] == [0, 0]
    assert ref.components(X, idx, dist=dist, sim_min=0.99, max_dist=np.nextafter(F(0.5), F(0)))["root"].tolist()[:2] == [0, 1]


def test_labels_do_not_depend_on_the_order_of_the_columns():
    X, idx = binary_rows(seed=3), random_lists(96, 6, 4)
    want = ref.components(X, idx, sim_min=0.5)
    perm = np.random.default_rng(0).permutation(6)
    got = ref.components(X, idx[:, perm], sim_min=0.5)
    assert np.array_equal(got["labels"], want["labels"]) and ref.same_bits(got["sim"], want["sim"][:, perm])


def test_identical_rows_need_not_have_similarity_one():
    """The contract pins what the expression gives; for these rows it is not 1."""
    X = np.tile(np.random.default_rng(1).standard_normal((1, 37)).astype(F), (2, 1))
    sim, _ = ref.similarity(X, np.array([[1], [0]], np.int32))
    sq = ref.dots(X, X)
    assert sim[0, 0] == sim[1, 0] == (sq[0] / (np.sqrt(sq[0]) * np.sqrt(sq[0])).astype(F)).astype(F) and abs(float(sim[0, 0]) - 1) < 3e-7


# ---- the seeded planted regions --------------------------------------------------------------------------------------------------------

def knn_lists(p, k):
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    return np.argsort(d2, axis=1, kind="stable")[:, :k + 1].astype(np.int32)


def test_synthetic_regions_are_found_by_the_reference():
    """With the helper's default noise, at the default threshold: the touching half-spaces split, the two separated balls of one
    prototype stay two regions, and every region is pure (all members share one generating set)."""
    means = torch.rand(1500, 3, generator=torch.Generator().manual_seed(0))
    out = regions.synthetic_regions(means)
    again = regions.synthetic_regions(means)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    X, sets, proto = (t.numpy() for t in out)
    assert proto.tolist() == [0, 1, 2, 2] and X.shape == (1500, 64) and X.dtype == F
    counts = np.bincount(sets[sets >= 0], minlength=4)
    assert (counts > 40).all() and 10 <= int((sets < 0).sum()) <= 60 and not X[sets < 0].any()
    m = means.numpy()
    gap = np.sqrt(((m[sets == 2][:, None] - m[sets == 3][None]) ** 2).sum(-1)).min()
    idx = knn_lists(m, 8)
    assert not (np.isin(idx[sets == 2], np.nonzero(sets == 3)[0])).any() and gap > 0.2  # separated: no list crosses
    assert np.isin(idx[sets == 0], np.nonzero(sets == 1)[0]).any()                       # touching: lists do cross
    got = ref.components(X, idx, sim_min=regions.DEFAULT_SIM_MIN)
    lab = got["labels"]
    assert np.array_equal(lab >= 0, sets >= 0)
    pairs = set(zip(lab[lab >= 0].tolist(), sets[lab >= 0].tolist()))
    assert len(pairs) == len({a for a, _ in pairs})  # pure: one generating set per region
    big = [int(np.bincount(lab[sets == s]).max()) for s in range(4)]
    assert all(b >= 0.9 * c for b, c in zip(big, counts))  # and each set is essentially one region, not dust


def test_quantiles_of_more_values_than_torch_quantile_takes():
    """18 M values (torch.quantile refuses more than 2^24), unsorted, with NaN among them: the quantiles of 0 .. m - 1 are q (m - 1)."""
    m = 18_000_000
    v = torch.arange(m, dtype=torch.float64).flip(0).reshape(-1, 9)
    v = torch.cat([v, torch.full((5, 9), float("nan"), dtype=torch.float64)])
    qs = (0.0, 0.01, 0.25, 0.5, 0.99, 1.0)
    got = regions.similarity_quantiles(v, qs)
    assert got == [q * (m - 1) for q in qs]
    small = torch.tensor([[0.5, float("nan"), 0.1], [0.9, 0.3, float("nan")]])
    want = torch.quantile(small[~torch.isnan(small)].double(), torch.tensor([0.0, 0.5, 1.0 / 3.0], dtype=torch.float64)).tolist()
    assert regions.similarity_quantiles(small, (0.0, 0.5, 1.0 / 3.0)) == pytest.approx(want, rel=1e-12)  # (the same interpolation)
    assert regions.similarity_quantiles(torch.full((3, 2), float("nan")), (0.5,)) == []


def test_edge_strength_and_host_checks():
    sim = torch.tensor([[0.9, float("nan"), 0.5], [float("nan")] * 3, [1.0, 1.0, 0.25]])
    assert torch.allclose(regions.edge_strength(sim), torch.tensor([0.5, 0.0, 0.75]))
    assert torch.allclose(regions.edge_strength(sim, "mean"), torch.tensor([0.3, 0.0, 0.25]))
    with pytest.raises(GwbpError, match="reduce"):
        regions.edge_strength(sim, "max")
    p, f = torch.zeros(8, 3), torch.zeros(8, 4)
    for fn, args in ((gsbp_amd.similarity_components, (p, f)), (gsbp_amd.similarity_levels, (p, f, [0.5]))):
        with pytest.raises(GwbpError, match="HIP tensors"):
            fn(*args)
    with pytest.raises(GwbpError, match="HIP tensor"):
        gsbp_amd.neighbor_similarity(f, torch.zeros(8, 2, dtype=torch.int32))
    with pytest.raises(GwbpError, match="NaN"):
        regions._sim_min(float("nan"))
    for radius in (-1.0, float("nan"), float("inf")):
        with pytest.raises(GwbpError, match="radius"):
            regions._max_dist(radius)
    assert regions._max_dist(None) == float("inf") and regions._max_dist(0.1) == float(F(0.1))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------

NAMES = {"gwbp_neighbor_similarity", "gwbp_edge_union"}


def test_new_symbols_are_in_the_map_the_header_and_the_binding():
    import fnmatch
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert NAMES <= set(_lib.EXPORTS)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gwbp.h")).read(), flags=re.S)
    assert NAMES <= set(re.findall(r"\b(gwbp_[a-z_]+)\s*\(", header))
    vmap = re.sub(r"/\*.*?\*/", "", open(os.path.join(_lib.CSRC, "gwbp.map")).read(), flags=re.S)
    pattern = re.search(r"global:\s*([^;]+);", vmap).group(1).strip()
    assert all(fnmatch.fnmatchcase(n, pattern) for n in NAMES)
    gsbp_amd.build()
    for n in NAMES:
        assert getattr(_lib.lib(), n) is not None
    for fn in ("neighbor_similarity", "similarity_components", "similarity_levels", "edge_strength", "region_prompt_mask",
               "synthetic_regions"):
        assert callable(getattr(gsbp_amd, fn))


P1, P2, P3, P4, P5, P6, P7, P8 = ((1 << s) for s in range(12, 20))  # fake, aligned, never dereferenced


def _sim(n=40, D=16, k=4, idx=P1, feats=P2, ldf=16, sim=P3, live=P4):
    return _lib.lib().gwbp_neighbor_similarity(n, D, k, idx, feats, ldf, sim, live, None)


def _union(n=40, k=4, idx=P1, sim=P3, live=P4, dist=None, group=None, sim_min=0.5, max_dist=float("inf"), count=P5, parent=P6, status=P7):
    return _lib.lib().gwbp_edge_union(n, k, idx, sim, live, dist, group, sim_min, max_dist, count, parent, status, None)


def _err():
    return _lib.lib().gwbp_last_error_string().decode()


def test_abi_argument_validation_needs_no_gpu():
    """Both entry points refuse each kind of bad argument with GWBP_EINVAL and a message before any HIP call (the pointers are fake
    and never dereferenced)."""
    gsbp_amd.build()
    nan = float("nan")
    shared = [(dict(n=0), "bad number"), (dict(n=-3), "bad number"), (dict(n=1 << 31), "bad number"), (dict(k=0), "k must"),
              (dict(k=65), "k must"), (dict(idx=None), "null"), (dict(sim=None), "null"), (dict(idx=P1 + 2), "aligned"),
              (dict(sim=P3 + 1), "aligned")]
    for kw, word in shared + [(dict(D=0), "D must"), (dict(D=2049, ldf=4096), "D must"), (dict(ldf=15), "stride"),
                              (dict(feats=None), "null"), (dict(live=None), "null"), (dict(feats=P2 + 2), "aligned"),
                              (dict(live=P4 + 1), "aligned"), (dict(sim=P2), "must not be"), (dict(live=P1), "must not be"),
                              (dict(live=P3), "same array")]:
        assert _sim(**kw) == -1, kw
        assert word in _err(), (kw, _err())
    for kw, word in shared + [(dict(sim_min=nan), "sim_min"), (dict(max_dist=-1.0), "max_dist"), (dict(max_dist=nan), "max_dist"),
                              (dict(live=None), "null"), (dict(count=None), "null"), (dict(parent=None), "null"),
                              (dict(status=None), "null"), (dict(parent=P6 + 2), "aligned"), (dict(dist=P8 + 1), "aligned"),
                              (dict(group=P8 + 2), "aligned"), (dict(count=P6), "same array"), (dict(status=P6), "same array"),
                              (dict(count=P4), "must not be"), (dict(parent=P3), "must not be"), (dict(parent=P1), "must not be"),
                              (dict(parent=P4), "must not be"), (dict(parent=P8, dist=P8), "must not be"),
                              (dict(status=P8, group=P8), "must not be")]:
        assert _union(**kw) == -1, kw
        assert word in _err(), (kw, _err())


# ---- the command line ----------------------------------------------------------------------------------------------------------------

def test_cli_help_parser_and_argument_checks(capsys):
    import run_regions
    ap = run_regions.build_parser()
    with pytest.raises(SystemExit) as e:
        ap.parse_args(["--help"])
    assert e.value.code == 0 and "--levels" in capsys.readouterr().out
    a = ap.parse_args(["--synthetic", "C1", "--levels", "0.8,0.9, 0.95", "--radius-factor", "2", "--min-size", "5", "--frames",
                       "--save-similarity", "--out", "x"])
    assert a.levels == [0.8, 0.9, 0.95] and a.sim_min is None and a.radius is None and a.radius_factor == 2.0 and a.k == 8
    assert a.min_size == 5 and a.frames and a.save_similarity and a.features is None
    run_regions.check_args(ap, a)
    bad = (["--sim-min", "0.9", "--levels", "0.5"], ["--radius", "0.1", "--radius-factor", "2"], ["--levels", "a,b"], ["--levels", ""],
           ["--levels", "nan"])
    for extra in bad:
        with pytest.raises(SystemExit):
            ap.parse_args(["--synthetic", "C1", "--out", "x"] + extra)
    for extra in (["--k", "0"], ["--k", "32"], ["--min-size", "0"], ["--sim-min", "nan"], ["--radius", "-1"], ["--radius-factor", "inf"]):
        with pytest.raises(SystemExit):
            run_regions.check_args(ap, ap.parse_args(["--synthetic", "C1", "--out", "x"] + extra))
    with pytest.raises(SystemExit):  # a scene needs --features
        run_regions.check_args(ap, ap.parse_args(["--checkpoint", __file__, "--out", "x"]))
    with pytest.raises(SystemExit):
        run_regions.check_args(ap, ap.parse_args(["--checkpoint", "/nonexistent/ckpt.pt", "--features", "f.pt", "--out", "x"]))
