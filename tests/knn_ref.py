"""TEST SUPPORT: float64 numpy restatement of the inner-product k-NN search and the majority vote (faiss IndexFlatIP.search +
np.bincount(...).argmax()), and the literal double loop it is checked against.  The reference of every k-NN comparison."""
import numpy as np

U = 2.0 ** -24


def scores64(Q, S):
    """Float64 inner products of the fp32 inputs: [N, M]."""
    return np.asarray(Q, np.float32).astype(np.float64) @ np.asarray(S, np.float32).astype(np.float64).T


def search(Q, S, k):
    """(scores[N, k] float64, indices[N, k]) sorted by (-score, index), stable."""
    sc = scores64(Q, S)
    order = np.argsort(-sc, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(sc, order, axis=1), order


def search_loop(Q, S, k):
    """search() as a literal double loop with an explicit (-score, index) sort."""
    Q, S = np.asarray(Q, np.float32), np.asarray(S, np.float32)
    sc_out, idx_out = np.zeros((Q.shape[0], k)), np.zeros((Q.shape[0], k), np.int64)
    for g in range(Q.shape[0]):
        cand = []
        for j in range(S.shape[0]):
            s = 0.0
            for c in range(Q.shape[1]):
                s += float(Q[g, c]) * float(S[j, c])
            cand.append((-s, j))
        cand.sort()
        for o in range(k):
            sc_out[g, o], idx_out[g, o] = -cand[o][0], cand[o][1]
    return sc_out, idx_out


def vote(idx, labels, num_classes):
    """(label[N], counts[N, num_classes]): bincount().argmax() over the valid labels of each row's indices; -1 where none is valid."""
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    idx = np.asarray(idx).astype(np.int64)
    out = np.full(idx.shape[0], -1, np.int64)
    counts = np.zeros((idx.shape[0], num_classes), np.int64)
    for g in range(idx.shape[0]):
        lab = labels[idx[g]]
        lab = lab[(lab >= 0) & (lab < num_classes)]
        if lab.size:
            counts[g] = np.bincount(lab, minlength=num_classes)
            out[g] = counts[g].argmax()
    return out, counts


def eps(Q, S):
    """Per query row: 2 (D + 1) u |q| max_j |s_j|, norms in float64 -- twice the worst-case error of an fp32 dot product of length D
    in any order (gamma_D = D u / (1 - D u) <= (D + 1) u for D <= 4095)."""
    Q, S = np.asarray(Q, np.float32).astype(np.float64), np.asarray(S, np.float32).astype(np.float64)
    return 2.0 * (Q.shape[1] + 1) * U * np.linalg.norm(Q, axis=1) * np.linalg.norm(S, axis=1).max()


def make_case(D, M, N, rng):
    """The issue's recipe: unit-norm Gaussian sources, queries = unit-normalised S[random row] + 0.5 randn / sqrt(D)."""
    S = rng.standard_normal((M, D))
    S /= np.linalg.norm(S, axis=1, keepdims=True)
    Q = S[rng.integers(0, M, N)] + 0.5 * rng.standard_normal((N, D)) / np.sqrt(D)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return Q.astype(np.float32), S.astype(np.float32)


def check_rows(Q, S, k, idx, score, labels=None, num_classes=None, label_out=None, counts_out=None, sc=None):
    """Checks 1-4 of every row (assertions); returns the float64 score matrix.  idx / score: the code under test's output."""
    Q, S = np.asarray(Q, np.float32), np.asarray(S, np.float32)
    idx, score = np.asarray(idx).astype(np.int64), np.asarray(score, np.float32).astype(np.float64)
    N, M = Q.shape[0], S.shape[0]
    assert idx.shape == (N, k) and score.shape == (N, k)
    sc = scores64(Q, S) if sc is None else sc
    e = eps(Q, S)
    # 1. distinct, in range, ordered by (score desc, index asc)
    assert idx.min() >= 0 and idx.max() < M
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "repeated index in a row"
    ds, di = score[:, 1:] - score[:, :-1], idx[:, 1:] - idx[:, :-1]
    assert ((ds < 0) | ((ds == 0) & (di > 0))).all(), "row not ordered by (score desc, index asc)"
    # 2. each score within eps / 2 of the float64 score of its index
    own = np.take_along_axis(sc, idx, axis=1)
    err = np.abs(score - own).max(axis=1)
    print(f"knn check: max |score - f64| = {err.max():.3e}, min eps/2 = {e.min() / 2:.3e}, max ratio = {(err / (e / 2 + 1e-300)).max():.3e}")
    assert (err <= e / 2).all(), "returned score outside one dot product's bound"
    # 3. each returned index's float64 score >= the float64 k-th best - eps
    kth = -np.partition(-sc, k - 1, axis=1)[:, k - 1]
    assert (own >= (kth - e)[:, None]).all(), "returned index is not among the k best within eps"
    # 4. label / counts of the row's own indices
    if labels is not None:
        lab, cnt = vote(idx, labels, num_classes)
        assert np.array_equal(np.asarray(label_out).astype(np.int64), lab), "label differs from bincount().argmax() of the row's indices"
        if counts_out is not None:
            assert np.array_equal(np.asarray(counts_out).astype(np.int64), cnt), "counts differ from the row's histogram"
    return sc


def decided_rows(sc, k, e):
    """Rows whose float64 gap between the k-th and (k+1)-th best score exceeds eps (check 5 applies to them)."""
    if sc.shape[1] <= k:
        return np.ones(sc.shape[0], bool)
    top = -np.partition(-sc, (k - 1, k), axis=1)[:, :k + 1]
    return (top[:, k - 1] - top[:, k]) > e
