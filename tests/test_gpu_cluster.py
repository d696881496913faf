"""gwbp_kmeans_assign / gwbp_cluster_sums and the layers above them on the GPU against the float64 mirror of tests/cluster_ref.py.

Let u = 2^-24 and eps(x) = 2 (D + 1) u |x| max|c| + 4 u (|x| max|c| + max|b|): twice the worst-case error of an fp32 dot product of
length D in any order plus one fp32 addition of the bias.  Every row's best lies within eps / 2 of the float64 score of its label,
every label's float64 score is at least the float64 maximum - eps, and on rows whose float64 gap between the best and the second
best exceeds eps the label equals the reference's.  The sums: every entry within n_k 2^-53 sum |w x| of np.add.at in float64 (the
any-order bound for n_k exact terms)."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import cluster

import cluster_ref as ref

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def raw_assign(dev, X, C, b=None):
    lab, best = cluster._assign(t(X, dev), t(C, dev), None if b is None else t(b, dev))
    assert lab.dtype == torch.int32 and best.dtype == torch.float32
    return lab.cpu().numpy(), best.cpu().numpy()


def check_assign(X, C, b, lab, best, sc=None):
    sc = ref.scores64(X, C, b) if sc is None else sc
    e = ref.eps(X, C, b)
    assert lab.min() >= 0 and lab.max() < C.shape[0]
    own = sc[np.arange(sc.shape[0]), lab]
    err = np.abs(best.astype(np.float64) - own)
    print(f"assign check: max |best - f64| = {err.max():.3e}, min eps / 2 = {e.min() / 2:.3e}, max ratio {(err / (e / 2 + 1e-300)).max():.3e}")
    assert (err <= e / 2).all(), "best outside one score's bound"
    assert (own >= sc.max(axis=1) - e).all(), "label is not the best within eps"
    return sc, e


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("D,K,N", [(64, 129, 1000), (36, 300, 257), (1028, 5, 130), (3, 2, 127), (32, 1, 64)])
def test_assignment_against_float64(dev, D, K, N, metric):
    rng = np.random.default_rng(1000 * D + K)
    X, C = ref.make_case(metric, D, K, N, rng)
    b = ref.bias_of(C, metric)
    sc = ref.scores64(X, C, b)
    decided = ref.decided_rows(sc, ref.eps(X, C, b))
    print(f"undecided rows: {100 * (1 - decided.mean()):.2f} %")
    assert 1.0 - decided.mean() <= 0.01  # on the reference alone
    lab, best = raw_assign(dev, X, C, b)
    check_assign(X, C, b, lab, best, sc)
    want, _ = ref.assign(X, C, b, sc)
    assert np.array_equal(lab[decided], want[decided])
    # the public function: the same labels, its bias computed on the device
    lab2, best2 = gsbp_amd.kmeans_assign(t(X, dev), t(C, dev), metric)
    assert np.array_equal(lab2.cpu().numpy(), lab) and np.array_equal(best2.cpu().numpy(), best)


@pytest.mark.parametrize("D,K,N", [(30, 257, 4097), (1024, 129, 130)])
def test_without_bias_equals_knn_search_bit_for_bit(dev, D, K, N):
    rng = np.random.default_rng(D)
    X, C = ref.make_case("cosine", D, K, N, rng)
    score, idx = gsbp_amd.knn_search(t(X, dev), t(C, dev), 1)
    lab, best = raw_assign(dev, X, C)
    assert np.array_equal(lab, idx[:, 0].cpu().numpy())
    assert np.array_equal(best.view(np.uint32), score[:, 0].cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("N", [1, 127, 129])
@pytest.mark.parametrize("K", [1, 128, 129])
@pytest.mark.parametrize("D", [1, 30, 1028])
def test_assignment_off_every_tile_edge(dev, N, K, D):
    rng = np.random.default_rng(N * 7 + K * 3 + D)
    for metric in ref.METRICS:
        X, C = ref.make_case(metric, D, K, N, rng)
        b = ref.bias_of(C, metric)
        lab, best = raw_assign(dev, X, C, b)
        check_assign(X, C, b, lab, best)


def test_strided_field_and_row_permutation(dev):
    rng = np.random.default_rng(5)
    X, C = ref.make_case("euclidean", 36, 140, 517, rng)
    b = ref.bias_of(C, "euclidean")
    lab, best = raw_assign(dev, X, C, b)
    wide = torch.zeros(517, 45, device=dev)  # an odd row stride, a column slice that starts off a 16-B boundary
    wide[:, 5:41] = t(X, dev)
    view = wide[:, 5:41]
    assert view.stride(0) == 45 and not view.is_contiguous()
    lab_s, best_s = cluster._assign(cluster.rows(view, "x"), t(C, dev), t(b, dev))
    assert np.array_equal(lab_s.cpu().numpy(), lab) and np.array_equal(best_s.cpu().numpy().view(np.uint32), best.view(np.uint32))
    lab_p, best_p = gsbp_amd.kmeans_assign(view, t(C, dev), "euclidean")
    assert np.array_equal(lab_p.cpu().numpy(), lab)
    perm = rng.permutation(517)
    lab_q, best_q = raw_assign(dev, X[perm], C, b)
    assert np.array_equal(lab_q, lab[perm]) and np.array_equal(best_q.view(np.uint32), best[perm].view(np.uint32))


def test_ties_nan_and_zero_rows(dev):
    rng = np.random.default_rng(6)
    X, C = ref.make_case("cosine", 20, 70, 200, rng)
    dup = np.concatenate([C, C[:70]])              # every centroid twice: 0..69 and 70..139, the second copy in the upper tile
    lab, best = raw_assign(dev, X, dup)
    assert lab.max() < 70, "a duplicate centroid must lose the tie to the lower index"
    lab1, best1 = raw_assign(dev, X, C)
    assert np.array_equal(lab, lab1) and np.array_equal(best.view(np.uint32), best1.view(np.uint32))
    # the tie inside one half of one tile, and across the halves
    lab, _ = raw_assign(dev, X, np.concatenate([C[:3], C[:3], C[3:70], C[:3]]))
    assert (lab[lab1 < 3] == lab1[lab1 < 3]).all()
    # a NaN row gets -1 / NaN; a NaN centroid is never chosen over a number
    Xn = X.copy()
    Xn[17, 3] = np.nan
    Cn = C.copy()
    Cn[int(lab1[0]), 0] = np.nan                   # row 0's own centroid
    lab, best = raw_assign(dev, Xn, Cn)
    assert lab[17] == -1 and np.isnan(best[17])
    assert lab[0] != lab1[0] and lab[0] >= 0 and not np.isnan(best).sum() > 1
    keep = (np.arange(200) != 17) & (lab1 != lab1[0])
    assert np.array_equal(lab[keep], lab1[keep])
    lab, best = raw_assign(dev, X, np.full((3, 20), np.nan, np.float32))
    assert (lab == -1).all() and np.isnan(best).all()
    # a zero row scores +0 against every centroid (label 0 from the kernel) and gets -1 through kmeans_assign; -0 counts as +0
    Xz = X.copy()
    Xz[5] = 0.0
    Xz[6] = -0.0
    lab, best = raw_assign(dev, Xz, C)
    assert lab[5] == 0 and lab[6] == 0 and best[5:7].view(np.uint32).tolist() == [0, 0]
    lab, best = gsbp_amd.kmeans_assign(t(Xz, dev), t(C, dev))
    assert lab[5] == -1 and lab[6] == -1 and int((lab < 0).sum()) == 2


# ---- sums ------------------------------------------------------------------------------------------------------------------------------

def sums_case(D, K, N, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)).astype(np.float32)
    labels = rng.integers(-1, K + 1, N)          # -1 and K included: they take no part
    if N >= 600:
        labels[:2 * cluster.RUN + 37] = np.where(labels[:2 * cluster.RUN + 37] < 0, -1, 1 % K)  # one cluster longer than one run
    w = (rng.random(N) * 2.0).astype(np.float32)
    return X, labels, w


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("D,K,N", [(64, 5, 1000), (30, 300, 257), (1028, 3, 130)])
def test_sums_against_float64(dev, D, K, N, weighted):
    X, labels, w = sums_case(D, K, N, 10 * D + K)
    w = w if weighted else None
    want, want_ws, want_cnt = ref.sums(X, labels, K, w)
    assert want_cnt.max() > cluster.RUN or N < 600
    xs, ls, wt = t(X, dev), t(labels, dev), None if w is None else t(w, dev)
    s, ws, cnt = gsbp_amd.cluster_sums(xs, ls, K, wt)
    assert s.dtype == torch.float64 and ws.dtype == torch.float64 and cnt.dtype == torch.int64 and s.shape == (K, D)
    got = s.cpu().numpy()
    bound = want_cnt[:, None] * U53 * ref.abs_sums(X, labels, K, w)
    err = np.abs(got - want)
    print(f"sums check: max err {err.max():.3e}, max err / bound {(err / (bound + 1e-300)).max():.3e}")
    assert (err <= bound).all()
    assert np.array_equal(cnt.cpu().numpy(), want_cnt)
    if w is None:
        assert np.array_equal(ws.cpu().numpy(), want_cnt.astype(np.float64))  # exact
    else:
        wb = want_cnt * U53 * ref.sums(np.ones((N, 1), np.float32), labels, K, w)[1]
        assert (np.abs(ws.cpu().numpy() - want_ws) <= wb).all()
    assert not got[want_cnt == 0].any(), "a cluster with no member gives a zero row"
    # two runs, another stream, a strided copy of the field: equal bits
    s2, ws2, _ = gsbp_amd.cluster_sums(xs, ls, K, wt)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        s3, ws3, _ = gsbp_amd.cluster_sums(xs, ls, K, wt)
    side.synchronize()
    wide = torch.zeros(N, D + 7, device=dev)
    wide[:, 3:3 + D] = xs
    s4, ws4, _ = gsbp_amd.cluster_sums(wide[:, 3:3 + D], ls, K, wt)
    for a, b in ((s2, ws2), (s3, ws3), (s4, ws4)):
        assert torch.equal(a, s) and torch.equal(b, ws)


def test_sums_of_small_integers_are_exact(dev):
    rng = np.random.default_rng(11)
    N, D, K = 1500, 70, 4
    X = rng.integers(-8, 9, (N, D)).astype(np.float32)
    w = rng.integers(0, 5, N).astype(np.float32)
    labels = rng.integers(0, K - 1, N)           # cluster K - 1 stays empty
    labels[:700] = 2                              # longer than two runs
    want, want_ws, want_cnt = ref.sums(X, labels, K, w)
    s, ws, cnt = gsbp_amd.cluster_sums(t(X, dev), t(labels, dev), K, t(w, dev))
    assert np.array_equal(s.cpu().numpy(), want) and np.array_equal(ws.cpu().numpy(), want_ws)
    assert np.array_equal(cnt.cpu().numpy(), want_cnt) and want_cnt[K - 1] == 0 and not s[K - 1].any() and float(ws[K - 1]) == 0.0
    # int32 labels, all of them out of range: zero sums
    s, ws, cnt = gsbp_amd.cluster_sums(t(X, dev), torch.full((N,), -1, dtype=torch.int32, device=dev), K)
    assert not s.any() and not ws.any() and not cnt.any()


def test_class_prototypes(dev):
    X, labels, w = sums_case(48, 6, 900, 12)
    labels = np.where(labels == 4, -1, labels)    # class 4 has no member
    want, want_ws, want_cnt = ref.sums(X, labels, 6, w)
    proto, cnt = gsbp_amd.class_prototypes(t(X, dev), t(labels, dev), 6, t(w, dev))
    assert proto.dtype == torch.float32 and np.array_equal(cnt.cpu().numpy(), want_cnt) and not proto[4].any()
    on = want_cnt > 0
    mean = want[on] / want_ws[on, None]
    unit = mean / np.linalg.norm(mean, axis=1, keepdims=True)
    # the sums bound relative to the norm of the sum, doubled for the normalisation, plus one fp32 rounding
    rel = (want_cnt[on, None] * U53 * ref.abs_sums(X, labels, 6, w)[on]).max(axis=1) / np.linalg.norm(want[on], axis=1)
    tol = 2.0 * np.sqrt(48) * rel[:, None] + 2.0 ** -24
    assert (np.abs(proto.cpu().numpy()[on].astype(np.float64) - unit) <= tol).all()
    plain, _ = gsbp_amd.class_prototypes(t(X, dev), t(labels, dev), 6, t(w, dev), normalize=False)
    assert np.abs(plain.cpu().numpy()[on] - mean).max() <= np.abs(mean).max() * 2.0 ** -23


# ---- the step and the fit ----------------------------------------------------------------------------------------------------------------

def kernel_callables(x, k, metric, w=None):
    zero = torch.linalg.vector_norm(x, dim=1) == 0

    def assign(c):
        labels, best = cluster._assign(x, c, cluster.centroid_bias(c, metric))
        labels[zero] = -1
        return labels, best

    return assign, (lambda labels: cluster._sums(x, labels, k, w))


@pytest.mark.parametrize("metric", ref.METRICS)
def test_one_lloyd_step_equals_the_mirror(dev, metric):
    rng = np.random.default_rng(21)
    X, C = ref.make_case(metric, 40, 9, 1500, rng)
    C = (C + 0.05 * rng.standard_normal(C.shape)).astype(np.float32)  # not yet the fixed point
    x = t(X, dev)
    assign, sums = kernel_callables(x, 9, metric)
    labels, best, new_c, counts, e = cluster.lloyd_step(x, t(C, dev), assign, sums, metric)
    m_lab, m_best, m_c, m_cnt, m_e = ref.lloyd_step(X, C, metric)
    b = ref.bias_of(C, metric)
    decided = ref.decided_rows(ref.scores64(X, C, b), ref.eps(X, C, b))
    assert decided.mean() >= 0.99 and e == m_e == 0
    lab = labels.cpu().numpy()
    assert np.array_equal(lab[decided], m_lab[decided])
    if decided.all():
        assert np.array_equal(lab, m_lab) and np.array_equal(counts.cpu().numpy(), m_cnt)
        # equal labels: the centroids differ by the sums bound, carried through the division, and one fp32 rounding
        s, ws, cnt = ref.sums(X, m_lab, 9)
        scale = np.linalg.norm(s, axis=1) if metric == "cosine" else ws
        rel = (cnt[:, None] * U53 * ref.abs_sums(X, m_lab, 9)).max(axis=1) / scale
        tol = 2.0 * np.sqrt(40) * rel[:, None] * np.maximum(np.abs(m_c), 1.0) + np.abs(m_c) * 2.0 ** -23 + 1e-45
        err = np.abs(new_c.cpu().numpy().astype(np.float64) - m_c)
        print(f"step check ({metric}): max centroid err {err.max():.3e}, max err / tol {(err / tol).max():.3e}")
        assert (err <= tol).all()


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("k,D,N", [(6, 32, 2000), (16, 512, 4096)])
def test_fit_kmeans_recovers_the_planted_partition(dev, k, D, N, metric):
    X, planted, _ = cluster.synthetic_clusters(N, k, D, 0.3, seed=0)
    x = X.to(dev)
    first = torch.stack([torch.nonzero(planted == j)[0, 0] for j in range(k)])
    km = gsbp_amd.fit_kmeans(x, k, metric=metric, init=X[first])
    assert km.converged and km.n_iter <= 3 and km.n_iter == len(km.history) and km.reseeds == 0 and km.inertia == km.history[-1]
    assert torch.equal(km.labels.cpu().long(), planted), "the planted partition is not recovered exactly"
    assert torch.equal(km.counts.cpu(), torch.bincount(planted, minlength=k))
    # every seeded init: the same bits twice, a partition of the rows, history that does not rise beyond the steps' eps sum
    for init in ("kmeans++", "sample"):
        a = gsbp_amd.fit_kmeans(x, k, metric=metric, init=init, seed=3)
        b = gsbp_amd.fit_kmeans(x, k, metric=metric, init=init, seed=3)
        assert torch.equal(a.centroids, b.centroids) and torch.equal(a.labels, b.labels) and torch.equal(a.counts, b.counts)
        assert a.history == b.history and a.n_iter == b.n_iter and a.converged == b.converged and a.reseeds == b.reseeds
        assert int(a.labels.min()) >= 0 and int(a.counts.sum()) == N
        # rows and centroids have |.| <= 1 (unit rows; unit-normalised sums or means of unit rows), |b| <= 1 / 2: eps against unit
        # centroids bounds every step's; the inertia term is 1 - best (cosine) or |x|^2 - 2 best (euclidean)
        unit = X[:1].numpy()
        bound = float(ref.eps(X.numpy(), unit, ref.bias_of(unit, metric)).sum()) * (1.0 if metric == "cosine" else 2.0)
        h = a.history
        print(f"{metric} {init}: history {h}, eps sum {bound:.3e}")
        assert all(h[i + 1] <= h[i] + bound for i in range(len(h) - 1))

@pytest.mark.parametrize("metric", ref.METRICS)
def test_duplicate_init_reseeds_as_the_mirror_does(dev, metric):
    X, planted, _ = cluster.synthetic_clusters(500, 3, 16, 0.3, seed=1)
    a, b = int(torch.nonzero(planted == 0)[0, 0]), int(torch.nonzero(planted == 1)[0, 0])
    c0 = torch.stack([X[a], X[a], X[b]])
    x = X.to(dev)
    assign, sums = kernel_callables(x, 3, metric)
    labels, best, new_c, counts, e = cluster.lloyd_step(x, c0.to(dev), assign, sums, metric)
    m_lab, m_best, m_c, m_cnt, m_e = ref.lloyd_step(X.numpy(), c0.numpy(), metric)
    assert e == m_e == 1 and int(counts[1]) == 1
    # the row of lowest best is decided by more than eps in the mirror, so the kernel's choice is the mirror's
    order = np.sort(m_best)
    assert order[1] - order[0] > ref.eps(X.numpy(), c0.numpy(), ref.bias_of(c0.numpy(), metric)).max()
    assert np.array_equal(labels.cpu().numpy(), m_lab) and np.array_equal(counts.cpu().numpy(), m_cnt)
    assert torch.allclose(new_c[1].cpu(), torch.from_numpy(m_c[1]), rtol=0, atol=2.0 ** -23)
    km = gsbp_amd.fit_kmeans(x, 3, metric=metric, init=c0)
    mine = ref.lloyd(X.numpy(), c0.numpy(), metric)
    assert km.reseeds == mine["reseeds"] >= 1 and km.n_iter == mine["n_iter"]
    assert np.array_equal(km.labels.cpu().numpy(), mine["labels"]) and int((km.counts == 0).sum()) == 0


# ---- the codebook ------------------------------------------------------------------------------------------------------------------

def test_codebook_queries_equal_the_dequantised_field(dev):
    X, planted, dirs = cluster.synthetic_clusters(3000, 12, 64, 0.3, seed=4)
    X[11] = 0.0
    x = X.to(dev)
    book, codes = gsbp_amd.quantize_field(x, 12, seed=1)
    assert book.shape == (12, 64) and book.dtype == torch.float32 and codes.dtype == torch.int32 and int(codes[11]) == -1
    assert int((codes < 0).sum()) == 1 and int(codes.max()) < 12
    field = gsbp_amd.dequantize_field(book, codes)
    assert field.shape == (3000, 64) and not field[11].any() and torch.equal(field[0], book[int(codes[0])])
    prompts = dirs[:5].to(dev) + 0.1
    for normalize in (True, False):
        want = gsbp_amd.prompt_scores(field, prompts, normalize)
        got = gsbp_amd.codebook_prompt_scores(book, codes, prompts, normalize)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    for n_pos, thr in ((2, None), (1, 0.3), (5, 0.5)):
        assert torch.equal(gsbp_amd.codebook_prompt_mask(book, codes, prompts, n_pos, thr), gsbp_amd.prompt_mask(field, prompts, n_pos, thr))
    assert bool(gsbp_amd.codebook_prompt_mask(book, codes, prompts, 2).any())
