"""Clustering without a GPU: the C ABI's names and argument validation, the package's Lloyd loop run over the numpy mirror's
primitives (tests/cluster_ref.py) against the mirror's own loop, the empty-cluster rule, the seeding, and the codebook functions."""
import os

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib, cluster
from gsbp_amd._lib import GwbpError

import cluster_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gwbp_kmeans_assign", "gwbp_cluster_sums", "gwbp_cluster_workspace_size")


def test_header_map_bindings_and_makefile_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "gwbp.h")).read()
    vmap = open(os.path.join(_lib.CSRC, "gwbp.map")).read()
    capi = open(os.path.join(_lib.CSRC, "capi.hip")).read()
    for n in NAMES:
        assert f"GWBP_API int {n}(" in header and n in vmap and f"int {n}(" in capi and n in _lib.EXPORTS
    assert "cluster.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "GWBP_CLUSTER_MAX_K (1 << 20)" in header and cluster.MAX_K == 1 << 20 >= 65536
    assert f"GWBP_CLUSTER_RUN {cluster.RUN}" in header
    gsbp_amd.build()
    for n in NAMES:
        assert getattr(_lib.lib(), n) is not None


P1, P2, P3, P4, P5, P6, P7 = (1 << 12), (1 << 13), (1 << 14), (1 << 15), (1 << 16), (1 << 17), (1 << 18)  # fake, never dereferenced


def _assign(N=4, K=3, D=8, X=P1, ldx=8, C=P2, ldc=8, b=None, label=P3, best=P4):
    return _lib.lib().gwbp_kmeans_assign(N, K, D, X, ldx, C, ldc, b, label, best, None)


def _sums(N=4, D=8, K=3, X=P1, ldx=8, w=None, order=P2, start=P3, sums=P4, wsum=P5, ws=P6, nbytes=1 << 30):
    return _lib.lib().gwbp_cluster_sums(N, D, K, X, ldx, w, order, start, sums, wsum, ws, nbytes, None)


def _err():
    return _lib.lib().gwbp_last_error_string().decode()


def test_abi_argument_validation_needs_no_gpu():
    """Every listed bad argument returns GWBP_EINVAL with a message before any HIP call (the pointers are fake)."""
    big = cluster.MAX_K + 1
    for kw, word in [(dict(N=-1), "N must not"), (dict(K=0), "K must be"), (dict(K=big), "K must be"), (dict(D=0), "D must be"),
                     (dict(ldx=7), "stride"), (dict(ldc=7), "ldc"), (dict(X=None), "null"), (dict(C=None), "null"),
                     (dict(label=None), "null"), (dict(best=None), "null"), (dict(X=P1 + 2), "aligned"), (dict(C=P2 + 1), "aligned"),
                     (dict(b=P5 + 2), "aligned"), (dict(label=P3 + 2), "aligned"), (dict(best=P4 + 2), "aligned")]:
        assert _assign(**kw) == -1, kw
        assert word in _err(), (kw, _err())
    for kw, word in [(dict(N=-1), "N must not"), (dict(K=0), "K must be"), (dict(K=big), "K must be"), (dict(D=0), "D must be"),
                     (dict(ldx=7), "stride"), (dict(X=None), "null"), (dict(order=None), "null"), (dict(start=None), "null"),
                     (dict(sums=None), "null"), (dict(wsum=None), "null"), (dict(ws=None), "null"), (dict(X=P1 + 2), "aligned"),
                     (dict(w=P7 + 2), "aligned"), (dict(order=P2 + 4), "aligned"), (dict(start=P3 + 4), "aligned"),
                     (dict(sums=P4 + 4), "aligned"), (dict(wsum=P5 + 4), "aligned"), (dict(ws=P6 + 4), "aligned")]:
        assert _sums(**kw) == -1, kw
        assert word in _err(), (kw, _err())
    assert _sums(nbytes=8) == -2 and "workspace" in _err()
    import ctypes as C
    nbytes = C.c_size_t(0)
    size = _lib.lib().gwbp_cluster_workspace_size
    for args in ((-1, 8, 3), (4, 0, 3), (4, 8, 0), (4, 8, big)):
        assert size(*args, C.byref(nbytes)) == -1
    assert size(4, 8, 3, None) == -1 and "null" in _err()
    assert size(1_000_000, 512, 256, C.byref(nbytes)) == 0
    slots = -(-1_000_000 // cluster.RUN) + 256
    assert slots * 513 * 8 <= nbytes.value <= slots * 513 * 8 + 257 * 8 + 1024
    assert size(3, 8, 1000, C.byref(nbytes)) == 0 and nbytes.value < 3 * 9 * 8 + 1001 * 8 + 1024  # no more runs than rows


def test_python_api_refuses_host_tensors_and_bad_arguments():
    x, c = torch.zeros(8, 4), torch.zeros(2, 4)
    with pytest.raises(GwbpError, match="HIP tensor"):
        gsbp_amd.kmeans_assign(x, c)
    with pytest.raises(GwbpError, match="HIP tensor"):
        gsbp_amd.cluster_sums(x, torch.zeros(8, dtype=torch.int64), 2)
    with pytest.raises(GwbpError, match="HIP tensor"):
        gsbp_amd.fit_kmeans(x, 2)
    with pytest.raises(GwbpError, match="metric"):
        cluster.centroid_bias(c, "manhattan")


# ---- the Lloyd loop over the numpy primitives ------------------------------------------------------------------------------------------

def mirror_callables(X, k, metric, w=None):
    """The package's two callables, computed by the numpy mirror on CPU tensors."""
    Xn = X.numpy()

    def assign(c):
        lab, best = ref.assign_rows(Xn, c.numpy(), metric)
        return torch.from_numpy(lab.astype(np.int32)), torch.from_numpy(best.astype(np.float32))

    def sums(labels):
        s, ws, cnt = ref.sums(Xn, labels.numpy(), k, None if w is None else w.numpy())
        return torch.from_numpy(s), torch.from_numpy(ws), torch.from_numpy(cnt)

    return assign, sums


def run_loop(X, c0, metric, iters=25, tol=0.0, w=None):
    assign, sums = mirror_callables(X, c0.shape[0], metric, w)
    sq = (X.double() ** 2).sum(dim=1)
    return cluster.lloyd(X, c0.clone(), assign, sums, metric, iters, tol, sq, w)


def eps_sum(X, C, metric, w=None):
    e = ref.eps(X, C, ref.bias_of(C, metric))
    e = e * (1.0 if metric == "cosine" else 2.0)  # the inertia term is 1 - best, or |x|^2 - 2 best
    return float((e if w is None else e * np.abs(w)).sum())


@pytest.mark.parametrize("metric", ref.METRICS)
def test_planted_partition_is_recovered_and_inertia_never_increases(metric):
    X, planted, _ = cluster.synthetic_clusters(2000, 6, 32, 0.3, seed=0)
    first = torch.stack([torch.nonzero(planted == j)[0, 0] for j in range(6)])
    c0 = X[first].clone()
    km = run_loop(X, c0, metric)
    assert km.converged and km.n_iter <= 3 and km.n_iter == len(km.history) and km.reseeds == 0
    assert torch.equal(km.labels.long(), planted), "the planted partition is not recovered exactly"
    assert torch.equal(km.counts, torch.bincount(planted, minlength=6))
    mine = ref.lloyd(X.numpy(), c0.numpy(), metric)
    assert np.array_equal(mine["labels"], km.labels.numpy()) and mine["n_iter"] == km.n_iter
    assert np.array_equal(mine["centroids"], km.centroids.numpy())
    # from a poor start: more steps, and no step's inertia above the one before by more than the step's sum of w eps
    c0 = X[:6].clone()
    km = run_loop(X, c0, metric, iters=12)
    # every centroid of every step is a unit row, a unit-normalised sum or a mean of unit rows: |c| <= 1 = |c0[j]|, |b| <= 1 / 2, so
    # eps against c0 bounds every step's eps; the mirror's scores are float64, so what is left is the centroids' fp32 rounding
    bound = eps_sum(X.numpy(), c0.numpy(), metric)
    h = km.history
    print(f"{metric}: history {h}, eps sum {bound:.3e}")
    assert len(h) >= 2 and all(h[i + 1] <= h[i] + bound for i in range(len(h) - 1))


@pytest.mark.parametrize("metric", ref.METRICS)
def test_duplicate_init_leaves_a_cluster_empty_and_it_is_reseeded(metric):
    X, planted, _ = cluster.synthetic_clusters(500, 3, 16, 0.3, seed=1)
    a, b = int(torch.nonzero(planted == 0)[0, 0]), int(torch.nonzero(planted == 1)[0, 0])
    c0 = torch.stack([X[a], X[a], X[b]])
    assign, sums = mirror_callables(X, 3, metric)
    lab0, best0 = assign(c0)
    assert int((lab0 == 1).sum()) == 0, "the bit-equal duplicate must lose every tie to the lower index"
    worst = int(torch.sort(best0, stable=True)[1][0])
    labels, best, new_c, counts, e = cluster.lloyd_step(X, c0, assign, sums, metric)
    assert e == 1 and int(labels[worst]) == 1 and int(counts[1]) == 1 and torch.equal(best, best0)
    assert torch.equal(labels[torch.arange(500) != worst], lab0[torch.arange(500) != worst])
    want = X[worst].double()
    want = (want / want.norm()).float() if metric == "cosine" else X[worst]
    assert torch.allclose(new_c[1], want, rtol=0, atol=1e-7)  # its only member: the mean of one row, rounded once
    mine = ref.lloyd_step(X.numpy(), c0.numpy(), metric)
    assert np.array_equal(mine[0], labels.numpy()) and np.array_equal(mine[2], new_c.numpy()) and mine[4] == 1
    km = run_loop(X, c0, metric)
    assert km.reseeds >= 1 and int((km.counts == 0).sum()) == 0


def test_zero_rows_get_minus_one_and_enter_no_sum():
    X, planted, _ = cluster.synthetic_clusters(300, 4, 8, 0.3, seed=2)
    X[7], X[100] = 0.0, 0.0
    first = torch.stack([torch.nonzero((planted == j) & (X.norm(dim=1) > 0))[0, 0] for j in range(4)])
    for metric in ref.METRICS:
        km = run_loop(X, X[first].clone(), metric)
        assert int(km.labels[7]) == -1 and int(km.labels[100]) == -1 and int(km.counts.sum()) == 298
        s, ws, cnt = ref.sums(X.numpy(), km.labels.numpy(), 4)
        assert cnt.sum() == 298 and ws.sum() == 298.0


def test_seeding_is_a_function_of_the_seed():
    X, _, _ = cluster.synthetic_clusters(400, 5, 8, 0.3, seed=3)
    X[3] = 0.0
    valid = torch.nonzero(X.norm(dim=1) > 0).squeeze(1)

    def distance(xc, centre):
        return ((xc.double() - centre.double()) ** 2).sum(dim=1)

    def picks(seed):
        g = torch.Generator().manual_seed(seed)
        a = cluster.init_sample(valid, 5, g)
        b = cluster.init_kmeanspp(X, valid, 5, "euclidean", torch.Generator().manual_seed(seed), distance)
        return a, b

    (a0, b0), (a1, b1), (a2, b2) = picks(0), picks(0), picks(1)
    assert torch.equal(a0, a1) and torch.equal(b0, b1)
    assert not torch.equal(a0, a2) and not torch.equal(b0, b2)
    for p in (a0, b0, a2, b2):
        assert p.shape == (5,) and 3 not in p.tolist() and len(set(p.tolist())) == 5
    with pytest.raises(GwbpError, match="non-zero rows"):
        cluster.init_sample(valid[:3], 5, torch.Generator().manual_seed(0))


def test_mirror_recipes_leave_no_row_undecided():
    rng = np.random.default_rng(0)
    for metric in ref.METRICS:
        for D, K, N in ((64, 129, 1000), (36, 300, 257), (3, 2, 127)):
            X, C = ref.make_case(metric, D, K, N, rng)
            b = ref.bias_of(C, metric)
            sc = ref.scores64(X, C, b)
            assert ref.decided_rows(sc, ref.eps(X, C, b)).all(), (metric, D, K, N)
            lab, best = ref.assign(X, C, b, sc)
            assert np.array_equal(best, sc.max(axis=1)) and (lab >= 0).all()
    sc = np.array([[np.nan, 1.0, 1.0], [np.nan, np.nan, np.nan], [2.0, -np.inf, np.nan]])
    lab, best = ref.assign(None, None, None, sc)
    assert lab.tolist() == [1, -1, 0] and best[0] == 1.0 and np.isnan(best[1])


# ---- the codebook ------------------------------------------------------------------------------------------------------------------

def test_dequantize_and_the_minus_one_code():
    book = torch.arange(12, dtype=torch.float32).reshape(3, 4) + 1.0
    codes = torch.tensor([2, -1, 0, 0, 1, 3, -7], dtype=torch.int32)
    out = cluster.dequantize_field(book, codes)
    assert out.shape == (7, 4) and out.dtype == torch.float32
    assert torch.equal(out[0], book[2]) and torch.equal(out[2], book[0]) and torch.equal(out[4], book[1])
    assert not out[1].any() and not out[5].any() and not out[6].any()
    assert torch.equal(cluster._codes(book, codes), torch.tensor([2, 3, 0, 0, 1, 3, 3]))
    assert torch.equal(cluster._with_zero_row(book)[:3], book) and not cluster._with_zero_row(book)[3].any()
    with pytest.raises(GwbpError, match="integer"):
        cluster.dequantize_field(book, torch.zeros(3))
    with pytest.raises(GwbpError, match="HIP tensor"):  # the codebook functions score on the device only
        cluster.codebook_prompt_scores(book, codes, torch.ones(1, 4))
    with pytest.raises(GwbpError, match="HIP tensor"):
        cluster.codebook_prompt_mask(book, codes, torch.ones(2, 4), 1)


def test_update_and_means_in_float64():
    s = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1.0, 1.0]], dtype=torch.float64)
    ws = torch.tensor([2.0, 0.0, 4.0], dtype=torch.float64)
    prev = torch.full((3, 2), 9.0)
    assert torch.equal(cluster.update_centroids(s, ws, prev, "cosine"), torch.tensor([[0.6, 0.8], [9.0, 9.0], [0.5 ** 0.5, 0.5 ** 0.5]]))
    assert torch.equal(cluster.update_centroids(s, ws, prev, "euclidean"), torch.tensor([[1.5, 2.0], [9.0, 9.0], [0.25, 0.25]]))
    assert torch.equal(cluster._means(s, ws, False).float(), torch.tensor([[1.5, 2.0], [0.0, 0.0], [0.25, 0.25]]))
    assert torch.equal(cluster._means(s, ws, True).float(), torch.tensor([[0.6, 0.8], [0.0, 0.0], [0.5 ** 0.5, 0.5 ** 0.5]]))


def test_cli_parser_and_synthetic_clusters():
    import run_cluster
    a = run_cluster.build_parser().parse_args(["--synthetic", "C1", "--k", "8", "--iters", "5", "--smooth-k", "4", "--frames", "--out", "x"])
    assert a.synthetic == "C1" and a.k == 8 and a.iters == 5 and a.smooth_k == 4 and a.frames and a.metric == "cosine"
    assert a.init == "kmeans++" and a.seed == 0 and a.weights is None and a.tol == 0.0
    with pytest.raises(SystemExit):
        run_cluster.build_parser().parse_args(["--k", "8"])  # --out is required
    assert torch.equal(run_cluster.palette_of(8), run_cluster.palette_of(8))
    x, lab, dirs = cluster.synthetic_clusters(100, 6, 32, 0.3, seed=0)
    x2, lab2, _ = cluster.synthetic_clusters(100, 6, 32, 0.3, seed=0)
    assert torch.equal(x, x2) and torch.equal(lab, lab2) and x.dtype == torch.float32 and lab.dtype == torch.int64
    assert sorted(set(lab.tolist())) == list(range(6)) and dirs.shape == (6, 32)
    assert torch.allclose(x.norm(dim=1), torch.ones(100), atol=1e-6)
    assert not torch.equal(x, cluster.synthetic_clusters(100, 6, 32, 0.3, seed=1)[0])
