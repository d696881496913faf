"""Point samples without a GPU: the float32 reference of the contract (sample_ref) against an independent float64 formulation within
a derived rounding bound; the contract's properties on the reference; the C ABI's validation; the symbols; the Python argument
checks; the command line's parser; score_point_labels against a literal loop."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib, sample
from gsbp_amd._lib import GwbpError

import sample_ref as ref

F = np.float32
EPS32 = float(np.finfo(F).eps)  # 2^-23; the unit roundoff of one correctly rounded operation is u = EPS32 / 2
C_BOUND = 16.0                  # derived in test_reference_agrees_with_float64_within_the_derived_bound's docstring


def scene(n=4096, q=4096, seed=0, ratio_lo=0.01, ratio_hi=0.1):
    """The issue's kind of inputs: means uniform in the unit cube, random quaternions, scales log-uniform in [0.01, 0.1], opacities
    in [0.05, 1], points = means + 0.03 x normal noise."""
    rng = np.random.default_rng(seed)
    means = rng.random((n, 3)).astype(F)
    quats = rng.standard_normal((n, 4)).astype(F)
    scales = np.exp(rng.uniform(np.log(ratio_lo), np.log(ratio_hi), (n, 3))).astype(F)
    opac = rng.uniform(0.05, 1.0, n).astype(F)
    pts = (means[rng.integers(0, n, q)] + 0.03 * rng.standard_normal((q, 3))).astype(F) if q != n else \
        (means + 0.03 * rng.standard_normal((n, 3))).astype(F)
    return pts, means, quats, scales, opac


def weights64(points, means, quats, scales, opac, qi, gi):
    """The independent formulation, float64 throughout: the rotation matrix of the normalised quaternion, u = S^-1 R^T d, np.exp.
    Returns (w, cond): cond = sum_a |u_a| sum_b |M_ab| |d_b|, the conditioning term of the bound."""
    q = np.asarray(quats, np.float64)
    q = q / np.sqrt((q * q).sum(axis=1))[:, None]
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)  # [N, 3, 3]
    M = R.transpose(0, 2, 1) / np.asarray(scales, np.float64)[:, :, None]
    d = np.asarray(points, np.float64)[qi] - np.asarray(means, np.float64)[gi]
    u = np.einsum("eab,eb->ea", M[gi], d)
    cond = (np.abs(u) * np.einsum("eab,eb->ea", np.abs(M[gi]), np.abs(d))).sum(axis=1)
    return np.asarray(opac, np.float64)[gi] * np.exp(-0.5 * (u * u).sum(axis=1)), cond


def test_reference_agrees_with_float64_within_the_derived_bound():
    """|w32 - w64| <= c eps32 w64 (1 + T), T = sum_a |u_a| sum_b |M_ab| |d_b|, with c = 16 for eps32 = 2^-23, i.e. 32 unit roundoffs
    u = 2^-24, from the operation count of the documented chain, to first order in u:
      quaternion: n2 is four roundings of non-negative terms (4 u), sqrtf halves that and adds one (3 u), the divide one (4 u), each
        q_c inv one more: every component carries 5 u.
      R: a product of two components 5 + 5 + 1 = 11 u; the sum of two products adds 1 u of the sum, the factor 2 is exact, and the
        diagonal's subtraction from 1 adds 1 u: with |xy| + |wz| <= 1/2 and y2 + z2 <= 1 every entry of R has an ABSOLUTE error of
        at most 25 u.  The count takes it as a RELATIVE error of 25 u of the entry, which is what it is for an entry of magnitude 1;
        an entry that cancels to far below 1 (a rotation close to an axis permutation) contributes to u_a through a product M_ab
        d_b that is small beside its row's other terms, which is where the form of the bound -- the row's sum of magnitudes, not
        the entry -- absorbs it for rotations in general position, the inputs below.
      M_ab = R_ba / s_a: one divide, 26 u.  d_b: one subtraction, 1 u.  The fmaf chain of u_a: three roundings, each of a partial sum
        bounded by the sum of magnitudes, 3 u.  So |du_a| <= 30 u sum_b |M_ab| |d_b|.
      sigma = 0.5 m2 (the factor is exact): dsigma = sum_a |u_a| |du_a| + 3 u sigma (m2's chain) <= 30 u T + 3 u sigma, and sigma =
        0.5 sum u_a^2 <= T / 2: dsigma <= 31.5 u T.
      w = o exp_neg(-sigma): exp turns dsigma into a relative error of its size; exp_neg's stated relative error is 2^-22 = 4 u
        (DESIGN 2); the product with o is one rounding: dw / w <= 31.5 u T + 5 u <= 32 u (1 + T).
    Kept-or-dropped must agree for every weight whose float64 value is not within a relative 1e-4 of alpha_min; at most 1 % of the
    weights may be left out for that reason."""
    pts, means, quats, scales, opac = scene()
    radius = sample.suggest_sample_radius(torch.from_numpy(scales), torch.from_numpy(opac))
    r2 = F(F(radius) * F(radius))
    M, o, live = ref.pack(means, quats, scales, opac)
    assert live.all()
    qi, gi = ref.candidate_pairs(pts, means, r2)
    sigma, w32 = ref.pair_weights(pts, means, M, o, qi, gi)
    keep32 = ref.kept(sigma, w32)
    w64, cond = weights64(pts, means, quats, scales, opac, qi, gi)
    keep64 = w64 >= float(ref.ALPHA_MIN)
    near = np.abs(w64 - float(ref.ALPHA_MIN)) <= 1e-4 * float(ref.ALPHA_MIN)
    assert near.mean() <= 0.01 and keep32.sum() > 8 * 4096
    assert np.array_equal(keep32[~near], keep64[~near])
    both = keep32 & keep64
    ratio = np.abs(w32[both].astype(np.float64) - w64[both]) / (EPS32 * w64[both] * (1.0 + cond[both]))
    print(f"pairs {qi.size}, kept {int(keep32.sum())}, left out {int(near.sum())}, max |w32 - w64| / (eps32 w64 (1 + T)) = {ratio.max():.3f}"
          f" (bound {C_BOUND})")
    assert ratio.max() <= C_BOUND
    # and the top-k of the reference are the float64 top-k wherever the float64 weights around rank k are not within the bound
    idx, w, nc = ref.point_gaussians(pts, means, quats, scales, opac, 8, r2, packed=(M, o, live))
    assert np.array_equal(nc, np.bincount(qi[keep32], minlength=pts.shape[0])) and (nc > 8).mean() > 0.5
    assert (np.diff(w.astype(np.float64), axis=1) <= 0).all() and ((idx >= 0) == (w > 0)).all()


# ---- properties of the contract, on the reference ------------------------------------------------------------------------------------

def test_quaternion_sign_and_scale_do_not_change_the_bits():
    _, means, quats, scales, opac = scene(256, 256, 1)
    M, o, _ = ref.pack(means, quats, scales, opac)
    for other in (-quats, (2 * quats).astype(F), (0.25 * quats).astype(F)):
        M2, o2, _ = ref.pack(means, other, scales, opac)
        assert ref.same_bits(M, M2) and ref.same_bits(o, o2)


def test_a_point_at_a_mean_has_the_opacity_exactly_and_alpha_min_is_kept():
    _, means, quats, scales, opac = scene(64, 64, 2)
    a = ref.ALPHA_MIN
    opac[:4] = [a, np.nextafter(a, F(0)), F(1.0), np.nextafter(a, F(1))]
    M, o, _ = ref.pack(means, quats, scales, opac)
    gi = np.arange(64)
    sigma, w = ref.pair_weights(means, means, M, o, gi, gi)
    assert (sigma == 0).all() and ref.same_bits(w, opac)
    assert ref.kept(sigma, w).tolist()[:4] == [True, False, True, True]
    idx, ws, nc = ref.point_gaussians(means[:4], means[:4], quats[:4], scales[:4] * F(1e-3), opac[:4], 2, F(0.0))
    assert idx[:, 0].tolist() == [0, -1, 2, 3] and nc.tolist() == [1, 0, 1, 1] and ws[0, 0] == a and ws[1, 0] == 0


def test_dead_gaussians_of_every_kind_and_non_finite_queries():
    pts, means, quats, scales, opac = scene(64, 16, 3)
    means[0, 1], quats[1, 2], quats[2], scales[3, 0], scales[4, 1], scales[5, 2] = np.nan, np.inf, 0.0, 0.0, -1.0, np.nan
    opac[6], opac[7], opac[8] = 0.0, np.nan, -0.5
    mask = np.ones(64, bool)
    mask[9] = False
    M, o, live = ref.pack(means, quats, scales, opac, mask)
    assert not live[:10].any() and live[10:].all() and not M[:10].any() and not o[:10].any()
    pts[3] = np.nan
    pts[5, 0] = np.inf
    idx, w, nc = ref.point_gaussians(pts, means, quats, scales, opac, 4, F(np.inf), live=mask)
    assert not np.isin(idx, np.arange(10)).any() and (idx[[3, 5]] == -1).all() and nc[3] == nc[5] == 0 and not w[[3, 5]].any()


def test_a_constant_power_of_two_field_comes_back_bit_for_bit():
    pts, means, quats, scales, opac = scene(512, 256, 4)
    idx, w, nc = ref.point_gaussians(pts, means, quats, scales, opac, 8, F(0.2 * 0.2))
    for value in (0.25, -8.0):
        out, wsum = ref.blend(idx, w, np.full((512, 5), value, F))
        valid = wsum > 0
        assert valid.sum() > 100 and (out[valid] == F(value)).all() and not out[~valid].any()
        assert np.array_equal(valid, nc > 0)


def test_a_nan_row_behind_a_zero_weight_does_not_leak():
    feats = np.arange(12, dtype=F).reshape(4, 3)
    feats[2], feats[3] = np.nan, np.inf
    idx = np.array([[0, 2, 1], [2, 3, -1], [4, 0, 3], [3, 2, 9]], np.int32)
    w = np.array([[0.5, 0.0, 0.25], [0.0, -0.0, 1.0], [1.0, 0.125, 0.0], [0.0, 0.0, 1.0]], F)
    out, wsum = ref.blend(idx, w, feats)
    assert wsum.tolist() == [0.75, 0.0, 0.125, 0.0] and np.isfinite(out).all()
    assert out[0].tolist() == [1.0, 2.0, 3.0] and not out[1].any() and out[2].tolist() == [0.0, 1.0, 2.0] and not out[3].any()


def test_vote_ties_go_to_the_smallest_class_and_outsiders_take_no_part():
    labels = np.array([3, 1, 1, 7, -2, 3], np.int64)
    idx = np.array([[0, 1, 2, -1], [5, 0, 1, 2], [3, 4, 6, 0], [3, 4, -1, 9], [1, 0, 3, 4]], np.int32)
    w = np.array([[0.5, 0.25, 0.25, 1.0], [0.25, 0.25, 0.5, 0.0], [1.0, 1.0, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0], [0.25, 0.5, 9.0, 9.0]], F)
    lab, share = ref.vote(idx, w, labels, 4)
    assert lab.tolist() == [1, 1, -1, -1, 3] and share.tolist() == [0.5, 0.5, 0.0, 0.0, F(0.5) / F(0.75)]
    assert ref.vote(idx, w, labels, 8)[0].tolist() == [1, 1, 7, 7, 7]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------

NAMES = {"gwbp_gaussian_pack", "gwbp_point_gaussians", "gwbp_neighbor_blend", "gwbp_weighted_vote"}


def test_new_symbols_are_in_the_map_the_header_and_the_binding():
    import fnmatch
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert NAMES <= set(_lib.EXPORTS)
    text = open(os.path.join(root, "include", "gwbp.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert NAMES <= set(re.findall(r"\b(gwbp_[a-z_]+)\s*\(", header))
    assert int(re.search(r"#define GWBP_SAMPLE_PACK (\d+)", text).group(1)) == sample.PACK and sample.PACK % 4 == 0
    vmap = re.sub(r"/\*.*?\*/", "", open(os.path.join(_lib.CSRC, "gwbp.map")).read(), flags=re.S)
    pattern = re.search(r"global:\s*([^;]+);", vmap).group(1).strip()
    assert all(fnmatch.fnmatchcase(n, pattern) for n in NAMES)
    gsbp_amd.build()
    for n in NAMES:
        assert getattr(_lib.lib(), n) is not None
    for fn in ("point_gaussians", "sample_field", "sample_labels", "transfer_field", "score_point_labels", "synthetic_points",
               "suggest_sample_radius", "neighbor_blend", "weighted_vote"):
        assert callable(getattr(gsbp_amd, fn))


P = [(1 << s) for s in range(12, 26)]  # fake, aligned, never dereferenced


def _pack(n=40, means=P[0], ldm=3, quats=P[1], ldq=4, scales=P[2], lds=3, opac=P[3], live=None, perm=P[4], pack=P[5]):
    return _lib.lib().gwbp_gaussian_pack(n, means, ldm, quats, ldq, scales, lds, opac, live, perm, pack, None)


def _walk(n=40, srt=P[0], cs=P[1], lo=(0.0, 0.0, 0.0), h=1.0, dims=(2, 2, 2), pack=P[5], r2=1.0, alpha=1.0 / 255, q=10, queries=P[6], ldq=3,
          order=P[7], k=8, idx=P[8], w=P[9], nc=P[10], visited=None):
    return _lib.lib().gwbp_point_gaussians(n, srt, cs, *lo, h, *dims, pack, r2, alpha, q, queries, ldq, order, k, idx, w, nc, visited, None)


def _blend(q=10, m=40, D=16, k=8, idx=P[8], w=P[9], feats=P[11], ldf=16, out=P[12], ldo=16, wsum=P[13]):
    return _lib.lib().gwbp_neighbor_blend(q, m, D, k, idx, w, feats, ldf, out, ldo, wsum, None)


def _vote(q=10, m=40, k=8, idx=P[8], w=P[9], labels=P[11], K=4, out=P[12], share=P[13]):
    return _lib.lib().gwbp_weighted_vote(q, m, k, idx, w, labels, K, out, share, None)


def _err():
    return _lib.lib().gwbp_last_error_string().decode()


def test_abi_argument_validation_needs_no_gpu():
    """Every entry point refuses each kind of bad argument with GWBP_EINVAL and a message before any HIP call (the pointers are fake
    and never dereferenced)."""
    gsbp_amd.build()
    nan, inf = float("nan"), float("inf")
    cases = {
        _pack: [(dict(n=0), "bad number"), (dict(n=1 << 31), "bad number"), (dict(ldm=2), "stride"), (dict(ldq=3), "stride"),
                (dict(lds=2), "stride"), (dict(means=None), "null"), (dict(quats=None), "null"), (dict(scales=None), "null"),
                (dict(opac=None), "null"), (dict(perm=None), "null"), (dict(pack=None), "null"), (dict(means=P[0] + 2), "aligned"),
                (dict(perm=P[4] + 4), "aligned"), (dict(pack=P[5] + 8), "aligned"), (dict(pack=P[0]), "must not be"),
                (dict(live=P[5]), "must not be")],
        _walk: [(dict(n=0), "bad number"), (dict(r2=-1.0), "r2"), (dict(r2=nan), "r2"), (dict(k=0), "k must"), (dict(k=33), "k must"),
                (dict(alpha=0.0), "alpha_min"), (dict(alpha=1e-31), "alpha_min"), (dict(alpha=1.5), "alpha_min"), (dict(alpha=nan), "alpha_min"),
                (dict(q=-1), "bad number"), (dict(ldq=2), "stride"), (dict(h=0.0), "cell size"), (dict(dims=(0, 1, 1)), "grid dimensions"),
                (dict(lo=(inf, 0.0, 0.0)), "origin"), (dict(srt=None), "null"), (dict(cs=None), "null"), (dict(pack=None), "null"),
                (dict(queries=None), "null"), (dict(order=None), "null"), (dict(idx=None), "null"), (dict(w=None), "null"),
                (dict(nc=None), "null"), (dict(srt=P[0] + 8), "aligned"), (dict(pack=P[5] + 4), "aligned"), (dict(order=P[7] + 4), "aligned"),
                (dict(idx=P[8] + 2), "aligned"), (dict(visited=P[11] + 1), "aligned"), (dict(idx=P[9]), "same array"),
                (dict(visited=P[10]), "same array"), (dict(w=P[5]), "must not be"), (dict(nc=P[6]), "must not be"), (dict(idx=P[0]), "must not be")],
        _blend: [(dict(q=-1), "bad sizes"), (dict(m=0), "bad sizes"), (dict(k=0), "k must"), (dict(k=33), "k must"), (dict(D=0), "D must"),
                 (dict(ldf=15), "stride"), (dict(ldo=15), "stride"), (dict(idx=None), "null"), (dict(w=None), "null"), (dict(feats=None), "null"),
                 (dict(out=None), "null"), (dict(wsum=None), "null"), (dict(feats=P[11] + 2), "aligned"), (dict(w=P[9] + 1), "aligned"),
                 (dict(out=P[11]), "must not be"), (dict(wsum=P[9]), "must not be"), (dict(wsum=P[12]), "same array")],
        _vote: [(dict(q=1 << 31), "bad sizes"), (dict(m=0), "bad sizes"), (dict(k=33), "k must"), (dict(K=0), "num_classes"),
                (dict(labels=None), "null"), (dict(out=None), "null"), (dict(share=None), "null"), (dict(labels=P[11] + 2), "aligned"),
                (dict(share=P[13] + 2), "aligned"), (dict(out=P[8]), "must not be"), (dict(share=P[12]), "same array")],
    }
    for fn, rows in cases.items():
        for kw, word in rows:
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert word in _err(), (fn.__name__, kw, _err())
    assert _walk(r2=inf, q=0, queries=None, order=None, idx=None, w=None, nc=None) == 0  # nothing to do is not an error, +inf is a radius
    assert _blend(q=0, idx=None, w=None, out=None, wsum=None) == 0 and _vote(q=0, idx=None, w=None, out=None, share=None) == 0


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------

def test_python_argument_checks():
    m, q, s, o = torch.zeros(8, 3), torch.ones(8, 4), torch.ones(8, 3), torch.ones(8)
    with pytest.raises(GwbpError, match="HIP tensors"):
        gsbp_amd.point_gaussians(m, m, q, s, o)
    with pytest.raises(GwbpError, match="HIP tensors"):
        gsbp_amd.transfer_field(m, q, s, o, torch.zeros(8, 4), m)
    with pytest.raises(GwbpError, match="HIP tensor"):
        gsbp_amd.neighbor_blend(torch.zeros(8, 4), torch.zeros(8, 2, dtype=torch.int32), torch.zeros(8, 2))
    with pytest.raises(GwbpError, match="HIP tensor"):
        gsbp_amd.weighted_vote(torch.zeros(8, dtype=torch.int64), 3, torch.zeros(8, 2, dtype=torch.int32), torch.zeros(8, 2))
    with pytest.raises(GwbpError, match="integer"):
        gsbp_amd.weighted_vote(torch.zeros(8), 3, torch.zeros(8, 2, dtype=torch.int32), torch.zeros(8, 2))
    for bad in (0.0, 1e-31, 1.5, float("nan")):
        with pytest.raises(GwbpError, match="alpha_min"):
            sample._alpha_min(bad)
    with pytest.raises(GwbpError, match="quantile"):
        gsbp_amd.suggest_sample_radius(s, o, quantile=1.5)
    with pytest.raises(GwbpError, match="point_gaussians"):
        gsbp_amd.sample_field(torch.zeros(8, 4), None)
    with pytest.raises(GwbpError, match="fallback"):
        gsbp_amd.sample_field(torch.zeros(8, 4), None, fallback="mean")
    with pytest.raises(GwbpError, match="point_gaussians"):
        gsbp_amd.sample_labels(torch.zeros(8, dtype=torch.int64), 3, None)


def test_suggested_radius_is_a_quantile_of_the_reach():
    scales = torch.tensor([[0.1, 0.2, 0.05], [1.0, 1.0, 1.0], [0.3, 0.1, 0.1], [5.0, 5.0, 5.0], [1.0, -1.0, 1.0]])
    opac = torch.tensor([1.0, 0.5, 0.25, 0.001, 1.0])
    r = sample.reach(scales, opac)
    a = sample.ALPHA_MIN
    s02, s03 = float(F(0.2)), float(F(0.3))  # (the scales are float32 tensors)
    want = [s02 * np.sqrt(2 * np.log(1.0 / a)), np.sqrt(2 * np.log(0.5 / a)), s03 * np.sqrt(2 * np.log(0.25 / a)), 0.0, 0.0]
    assert np.allclose(r.numpy(), want, rtol=1e-12)
    assert gsbp_amd.suggest_sample_radius(scales, opac, quantile=1.0) == pytest.approx(max(want) * (1 + 1e-4), rel=1e-12)
    assert gsbp_amd.suggest_sample_radius(scales, opac, quantile=0.0) == pytest.approx(min(w for w in want if w > 0) * (1 + 1e-4), rel=1e-12)
    assert gsbp_amd.suggest_sample_radius(scales, torch.zeros(5)) == 0.0
    # at quantile 1.0 no kept weight is lost to the radius: the reference with that radius equals the reference with r2 = +inf
    pts, means, quats, sc, op = scene(300, 200, 6)
    full = sample.suggest_sample_radius(torch.from_numpy(sc), torch.from_numpy(op), quantile=1.0)
    got = ref.point_gaussians(pts, means, quats, sc, op, 4, F(F(full) * F(full)))
    want = ref.point_gaussians(pts, means, quats, sc, op, 4, F(np.inf))
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and want[2].max() > 4


def test_score_point_labels_against_a_literal_loop():
    rng = np.random.default_rng(0)
    k = 5
    pred = rng.integers(-1, k + 1, 500)
    gt = rng.integers(-1, k + 1, 500)
    want = np.zeros((k, 3), np.int64)
    for p, t in zip(pred, gt):
        if t == -1 or not 0 <= t < k:
            continue
        want[t, 2] += 1
        if 0 <= p < k:
            want[p, 1] += 1
        if p == t:
            want[t, 0] += 1
    got = gsbp_amd.score_point_labels(torch.from_numpy(pred), torch.from_numpy(gt), k)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    res = gsbp_amd.miou_recall(got)
    iou = [want[c, 0] / (want[c, 1] + want[c, 2] - want[c, 0]) for c in range(1, k)]
    assert res["miou"] == pytest.approx(float(np.mean(iou)))
    ign = gsbp_amd.score_point_labels(torch.from_numpy(pred), torch.from_numpy(gt), k, ignore=2).numpy()
    assert ign[2, 0] == 0 and ign[2, 2] == 0 and np.array_equal(ign[[0, 1, 3, 4]][:, [0, 2]], want[[0, 1, 3, 4]][:, [0, 2]])
    with pytest.raises(GwbpError, match="one shape"):
        gsbp_amd.score_point_labels(torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 2)


def test_synthetic_points_are_seeded_jittered_means_plus_far_points():
    means = torch.rand(400, 3, generator=torch.Generator().manual_seed(1))
    a, b = gsbp_amd.synthetic_points(means), gsbp_amd.synthetic_points(means)
    assert torch.equal(a, b) and a.shape == (416, 3) and a.dtype == torch.float32
    d = torch.cdist(a, means).min(dim=1).values
    assert float(d[:400].max()) < 0.2 and float(d[400:].min()) > 9.0
    assert gsbp_amd.synthetic_points(means, count=10, far=2).shape == (12, 3)


# ---- the command line ------------------------------------------------------------------------------------------------------------------

def test_cli_help_parser_and_argument_checks(capsys):
    import run_sample
    ap = run_sample.build_parser()
    with pytest.raises(SystemExit) as e:
        ap.parse_args(["--help"])
    assert e.value.code == 0 and "--colmap-points" in capsys.readouterr().out
    a = ap.parse_args(["--synthetic", "C1", "--num-classes", "6", "--k", "16", "--radius-quantile", "1.0", "--fallback", "nearest",
                       "--out", "x"])
    assert a.k == 16 and a.radius is None and a.radius_quantile == 1.0 and a.fallback == "nearest" and a.num_classes == 6
    assert a.alpha_min is None and a.points is None and not a.colmap_points and a.scene_points is None
    run_sample.check_args(ap, a)
    for extra in (["--radius", "0.1", "--radius-quantile", "0.9"], ["--points", "p.pt", "--colmap-points"], ["--fallback", "mean"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["--synthetic", "C1", "--out", "x"] + extra)
    for extra in (["--k", "0"], ["--k", "33"], ["--radius", "-1"], ["--radius", "nan"], ["--radius-quantile", "1.5"], ["--alpha-min", "0"],
                  ["--alpha-min", "2"], ["--labels", "l.pt"], ["--num-classes", "0"]):
        with pytest.raises(SystemExit):
            run_sample.check_args(ap, ap.parse_args(["--synthetic", "C1", "--out", "x"] + extra))
    with pytest.raises(SystemExit):  # a scene needs points and something to sample
        run_sample.check_args(ap, ap.parse_args(["--checkpoint", __file__, "--features", "f.pt", "--out", "x"]))
    with pytest.raises(SystemExit):
        run_sample.check_args(ap, ap.parse_args(["--checkpoint", __file__, "--points", "p.pt", "--out", "x"]))
    with pytest.raises(SystemExit):
        run_sample.check_args(ap, ap.parse_args(["--checkpoint", "/nonexistent/ckpt.pt", "--points", "p.pt", "--features", "f.pt", "--out", "x"]))
