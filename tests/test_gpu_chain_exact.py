"""The MFMA kernels bit for bit against the fmaf chains their headers document (tests/chain_ref.py).

Every kernel family that computes on v_mfma_f32_16x16x4_f32 promises that a product sum is ONE chain of fp32 fused multiply-adds
from +0 in an order that depends on the reduction length alone.  The other GPU tests hold the kernels inside any-order rounding
bounds or against each other; here every score, label, index list and gradient of every row is compared with the documented chain
itself: equality of bits (view(uint32)) or of integers, no tolerance, no row left out.  Shapes are small enough to mirror on the
CPU (rows x columns x length of a product under about 2e7) and sit on the kernels' edges: lengths off the 16 / 32 / 64-column
blocks, row counts off the 128-row workgroup, one element, more than one tile of sources."""
import functools

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import cluster
from gsbp_amd.rasterization import get_engine

import chain_ref as cr
import decode_ref

pytestmark = pytest.mark.gpu
F = np.float32


def t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the cached cases are read-only)


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert a.dtype == F
    return a.view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    wrong = g != w
    if wrong.any():
        at = tuple(int(v) for v in np.argwhere(wrong)[0])
        raise AssertionError(f"{what}: {int(wrong.sum())} of {wrong.size} entries differ from the chain; first at {at}: "
                             f"kernel 0x{int(g[at]):08X}, mirror 0x{int(w[at]):08X}")


def odd_offset_view(a, dev, offset, extra):
    """a's rows inside a wider NaN-filled buffer at an odd column offset: 4-B aligned rows only, the element-load kernels."""
    wide = torch.full((a.shape[0], a.shape[1] + offset + extra), float("nan"), device=dev)
    wide[:, offset:offset + a.shape[1]] = t(a, dev)
    return wide[:, offset:offset + a.shape[1]]


# ---- k_knn_search and k_kmeans_assign: one score matrix per shape, shared ---------------------------------------------------------
KNN_SHAPES = [(130, 129, 1028, 5), (130, 129, 1024, 20), (257, 300, 36, 32), (127, 257, 30, 1), (1, 1, 1, 1), (129, 128, 33, 5)]


@functools.lru_cache(maxsize=None)
def knn_case(N, M, D, scale=1.0):
    """Seeded standard normal (Q [N, D], S [M, D]) times `scale` (a power of two) and the mirror's score matrix; never modified."""
    rng = np.random.default_rng(10000 * N + 100 * M + D)
    Q, S = (rng.standard_normal((N, D)) * scale).astype(F), (rng.standard_normal((M, D)) * scale).astype(F)
    sc = cr.chain(Q, S, cr.knn_order(D))
    for a in (Q, S, sc):
        a.setflags(write=False)
    return Q, S, sc


def check_search(dev, Q, S, sc, k, what):
    want_idx, want_score = cr.topk(sc, k)
    aligned = (t(Q, dev), t(S, dev))
    element = (odd_offset_view(Q, dev, 5, 2), odd_offset_view(S, dev, 3, 2))
    for name, (q, s) in (("16-B loads", aligned), ("element loads", element)):
        score, idx = gsbp_amd.knn_search(q, s, k)
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want_idx), (what, name)
        assert_bits(score, want_score, f"{what}, {name}: score")


@pytest.mark.parametrize("N, M, D, k", KNN_SHAPES)
def test_knn_search_equals_the_chain(dev, N, M, D, k):
    Q, S, sc = knn_case(N, M, D)
    check_search(dev, Q, S, sc, k, f"knn_search N={N} M={M} D={D} k={k}")


def test_knn_search_with_every_source_duplicated(dev):
    Q, A, sc = knn_case(127, 100, 30)
    S, sc2 = np.concatenate([A, A]), np.concatenate([sc, sc], axis=1)
    check_search(dev, Q, S, sc2, 6, "knn_search, duplicated sources")
    idx = gsbp_amd.knn_search(t(Q, dev), t(S, dev), 6)[1].cpu().numpy()
    assert np.array_equal(idx[:, 1::2], idx[:, 0::2] + 100)  # (the mirror's lists are pairs j, j + 100: so are the kernel's)


def test_knn_search_through_the_subnormal_range_and_into_infinity(dev):
    """Both operands times 2^-63: products of about 2^-126, partial sums in the fp32 subnormal range (the MFMA keeps them under the
    build's default denormal mode).  Times 2^63: sums beyond 2^128 become infinities, which order by index among themselves."""
    for scale, N, M, D, k in ((2.0 ** -63, 129, 128, 33, 5), (2.0 ** 63, 127, 257, 30, 20)):
        Q, S, sc = knn_case(N, M, D, scale)
        if scale < 1:
            tiny = (np.abs(sc) < 2.0 ** -126) & (sc != 0)
            assert tiny.mean() > 0.05 and len(np.unique(bits(sc))) > sc.size // 2  # subnormal scores among them, no flushed ones
        else:
            assert 0.1 < np.isinf(sc).mean() < 0.9 and not np.isnan(sc).any()
        check_search(dev, Q, S, sc, k, f"knn_search scaled by {scale:g}")


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("N, K, D, _k", KNN_SHAPES[:4])
def test_kmeans_assign_equals_the_chain(dev, N, K, D, _k, with_bias):
    X, C, sc = knn_case(N, K, D)
    b = (np.random.default_rng(K).standard_normal(K) * np.sqrt(D)).astype(F) if with_bias else None
    want_label, want_best = cr.assign(sc, b)
    for name, x, c in (("16-B loads", t(X, dev), t(C, dev)), ("element loads", odd_offset_view(X, dev, 5, 2), odd_offset_view(C, dev, 3, 2))):
        label, best = cluster._assign(x, c, None if b is None else t(b, dev))
        assert np.array_equal(label.cpu().numpy(), want_label), name
        assert_bits(best, want_best, f"kmeans_assign N={N} K={K} D={D} bias={with_bias}, {name}: best")
    if not with_bias:  # what the contract promises on top: the assignment without bias is knn_search(k = 1)
        score, idx = gsbp_amd.knn_search(t(X, dev), t(C, dev), 1)
        assert np.array_equal(idx.cpu().numpy()[:, 0], want_label) and np.array_equal(bits(score)[:, 0], bits(want_best))
    else:  # the public euclidean assignment: the mirror fed the bias the function computed on the device
        xd, cd = t(X, dev), t(C, dev)
        label, best = gsbp_amd.kmeans_assign(xd, cd, "euclidean")
        want_label, want_best = cr.assign(sc, cluster.centroid_bias(cd, "euclidean").cpu().numpy())
        assert np.array_equal(label.cpu().numpy(), want_label)
        assert_bits(best, want_best, f"kmeans_assign euclidean N={N} K={K} D={D}: best")


# ---- k_prompt_scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("N, D, P", [(130, 1028, 5), (257, 36, 32), (127, 30, 17), (1, 1, 1)])
def test_prompt_scores_and_mask_equal_the_chain(dev, N, D, P, normalize):
    rng = np.random.default_rng(1000 * N + D + P)
    X, prompts = rng.standard_normal((N, D)).astype(F), rng.standard_normal((P, D)).astype(F)
    want = cr.prompt_scores(X, prompts, normalize)
    for name, x in (("16-B loads", t(X, dev)), ("element loads", odd_offset_view(X, dev, 5, 2))):
        assert_bits(gsbp_amd.prompt_scores(x, t(prompts, dev), normalize), want, f"prompt_scores N={N} D={D} P={P}, {name}")
    thr = float(np.median(want[:, 0]))
    for n_pos, threshold in ((max(1, P // 2), None), (max(1, P // 2), thr), (P, thr), (1, None)):
        if n_pos == P and threshold is None:
            continue  # (a mask without negatives needs a threshold)
        got = gsbp_amd.prompt_mask(t(X, dev), t(prompts, dev), n_pos, threshold, normalize=normalize)
        assert np.array_equal(got.cpu().numpy(), cr.prompt_mask(want, n_pos, threshold)), (n_pos, threshold)


# ---- k_pca_project --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("D", [1028, 36])
@pytest.mark.parametrize("N", [130, 257])
def test_pca_transform_equals_the_chain(dev, N, D, k):
    rng = np.random.default_rng(100 * N + D)
    X = (rng.standard_normal((N, D)) * rng.uniform(0.5, 2.0, D) + rng.standard_normal(D)).astype(F)  # a mean and unequal spreads
    basis = gsbp_amd.fit_pca(t(X, dev), k)
    mean, V = basis.mean.cpu().numpy(), basis.components.cpu().numpy()
    assert mean.dtype == F and V.dtype == F and V.shape == (k, D)
    want = cr.pca_project(X, mean, V)
    assert_bits(gsbp_amd.pca_transform(t(X, dev), basis), want, f"pca_transform N={N} D={D} k={k}, 16-B loads")
    assert_bits(gsbp_amd.pca_transform(odd_offset_view(X, dev, 5, 2), basis), want, f"pca_transform N={N} D={D} k={k}, element loads")


# ---- k_encode_map ---------------------------------------------------------------------------------------------------------------------
def check_encode(dev, feats, enc, what):
    H, W, K = feats.shape
    want = cr.chain(feats.reshape(H * W, K), enc.T, cr.encode_order(K)).reshape(H, W, enc.shape[1])
    eng = gsbp_amd.Engine(16, W, H, device=dev)
    assert_bits(eng.encode_map(t(feats, dev), t(enc, dev)), want, f"{what}: dense map")
    big = torch.zeros(H, W + 3, 2 * K, device=dev)  # a view into a wider buffer: pixel stride 2 K, row stride with a gap
    big[:, :W, :K] = t(feats, dev)
    assert_bits(eng.encode_map(big[:, :W, :K], t(enc, dev)), want, f"{what}: pixel-strided map")
    return want


@pytest.mark.parametrize("H, W, K, n", [(37, 53, 512, 16), (16, 16, 64, 5), (9, 7, 32, 1), (40, 24, 128, 13)])
def test_encode_map_equals_the_chain(dev, H, W, K, n):
    g = torch.Generator().manual_seed(H * 1000 + W)
    feats = torch.randn(H, W, K, generator=g).numpy()
    enc = (torch.randn(K, n, generator=g) / K ** 0.5).numpy()
    check_encode(dev, feats, enc, f"encode_map {H}x{W} K={K} n={n}")


def test_encode_map_through_the_subnormal_range(dev):
    rng = np.random.default_rng(11)
    feats = (rng.standard_normal((16, 16, 64)) * 2.0 ** -63).astype(F)
    enc = (rng.standard_normal((64, 5)) * 2.0 ** -63).astype(F)
    want = check_encode(dev, feats, enc, "encode_map scaled by 2^-63")
    assert ((np.abs(want) < 2.0 ** -126) & (want != 0)).mean() > 0.05


# ---- k_decode_gr / k_decode_gc --------------------------------------------------------------------------------------------------------
DEC_SHAPES = {5: (1, 5), 64: (8, 8), 70 * 45: (45, 70)}  # P -> (H, W): less than a block, one block, 50 slices
DEC_SCALE = 0.125


def check_decode(dev, R, C, M, loss, what, weights=None):
    P, d = R.shape
    h, w = DEC_SHAPES[P]
    kw = {} if weights is None else dict(pixel_weights=t(weights, dev).reshape(h, w))
    _, GR, GC, table = get_engine(dev, decode_ref.N, decode_ref.W, decode_ref.H).decode_loss(
        t(R, dev).reshape(h, w, d), t(C, dev), t(M, dev).reshape(h, w, C.shape[1]), loss=loss, scale=DEC_SCALE, **kw)
    want_GR, want_GC = cr.decode_loss(R, C, M, loss, DEC_SCALE, weights)
    assert_bits(GR.reshape(P, d), want_GR, f"{what}: GR")
    assert_bits(GC, want_GC, f"{what}: GC")
    return GR.reshape(P, d), table


@pytest.mark.parametrize("loss", ["l1", "l2"])
@pytest.mark.parametrize("P, d, D", [(5, 16, 16), (64, 48, 80), (70 * 45, 48, 80), (64, 128, 528)])
def test_decode_loss_gradients_equal_the_chains(dev, P, d, D, loss):
    R, C, M = decode_ref.kernel_inputs(P, d, D, seed=5, loss=loss)
    check_decode(dev, R, C, M, loss, f"decode_loss P={P} d={d} D={D} {loss}")


@pytest.mark.parametrize("loss", ["l1", "l2"])
def test_decode_loss_with_a_weight_map_and_with_non_finite_rows(dev, loss):
    P, d, D = 70 * 45, 48, 80
    R, C, M = decode_ref.kernel_inputs(P, d, D, seed=6, loss=loss)
    weights = np.random.default_rng(12).uniform(0.0, 2.0, P).astype(F)
    weights[::17] = 0.0
    check_decode(dev, R, C, M, loss, f"decode_loss {loss}, weight map", weights)
    M = M.copy()
    rows = [7 * 70 + 33, 64, P - 1]  # inside a slice, first of a block, the last pixel (in the partial block)
    M[rows[0], 2], M[rows[0], D - 1], M[rows[1], 17], M[rows[2], 64] = np.nan, np.inf, -np.inf, np.nan
    GR, table = check_decode(dev, R, C, M, loss, f"decode_loss {loss}, non-finite rows")
    assert not bool(GR[rows].any()) and table.tolist()[1:4] == [P - 3, 3, P]
