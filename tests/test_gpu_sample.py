"""Point samples on the GPU (csrc/sample.hip) against the brute-force reference in the contract's own fp32 arithmetic (sample_ref):
the walk's lists, weights and counts, the blend, the vote and the Python layer, EXACTLY (equal bits), whatever the grid; every case
runs twice and the two runs give identical tensors."""
import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import regions, sample, spatial, synthetic as syn

import sample_ref as ref

pytestmark = pytest.mark.gpu
F = np.float32
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:  # a reference is computed once, shared, and left unchanged
        _CACHE[key] = make()
    return _CACHE[key]


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert x.dtype == y.dtype and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    return a


def dev_t(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


# ---- the walk ------------------------------------------------------------------------------------------------------------------------------

RADIUS = 0.375  # dyadic: 0.5 + RADIUS and its square are exact in fp32
N_WALK, Q_JITTER = 2048, 1000


def walk_scene():
    """2048 Gaussians in the unit cube with scales in [0.02, 0.2] (so that n_contrib > k on many rows, at k = 32 too): Gaussians 64 ..
    127 are bit-identical copies of 0 .. 63 (ties by index), 128 .. 137 are dead, each in its own way, 138 is masked out, 139 sits
    at exactly RADIUS from query 0.  Queries: 1000 jittered means, 16 far points, 8 non-finite ones: Q = 1024."""
    rng = np.random.default_rng(11)
    means = rng.random((N_WALK, 3)).astype(F)
    quats = rng.standard_normal((N_WALK, 4)).astype(F)
    scales = np.exp(rng.uniform(np.log(0.02), np.log(0.2), (N_WALK, 3))).astype(F)
    opac = rng.uniform(0.05, 1.0, N_WALK).astype(F)
    for a in (means, quats, scales, opac):
        a[64:128] = a[0:64]
    means[128, 2], quats[129, 0], quats[130], scales[131, 1], scales[132, 0], scales[133, 2] = np.nan, np.nan, 0.0, 0.0, -0.1, np.inf
    opac[134], opac[135], opac[136], means[137, 0] = 0.0, np.nan, -1.0, np.inf
    mask = np.ones(N_WALK, bool)
    mask[138] = False
    pts = (means[rng.integers(0, N_WALK, Q_JITTER)] + 0.03 * rng.standard_normal((Q_JITTER, 3))).astype(F)
    pts[np.isnan(pts).any(axis=1) | np.isinf(pts).any(axis=1)] = 0.5
    pts[0] = (0.5, 0.5, 0.5)
    means[139], scales[139], opac[139] = (0.5 + RADIUS, 0.5, 0.5), 1.0, 1.0  # dx = RADIUS exactly in fp32: d2 == r2
    far = (100.0 * np.sign(rng.standard_normal((16, 3))) + rng.random((16, 3))).astype(F)
    bad = np.full((8, 3), 0.5, F)
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3], bad[4, 0], bad[5, 1], bad[6, 2], bad[7] = np.nan, np.nan, np.nan, np.nan, np.inf, -np.inf, np.inf, np.inf
    return np.concatenate([pts, far, bad]), means, quats, scales, opac, mask


def walk_ref(radius):
    def make():
        pts, means, quats, scales, opac, mask = walk_scene()
        r2 = F(np.inf) if radius == np.inf else F(F(radius) * F(radius))
        rows = pts[:256] if radius == np.inf else pts
        return ref.point_gaussians(rows, means, quats, scales, opac, 32, r2, live=mask)
    return cached(("walk", radius), make)


def run_walk(dev, pts, k, radius, **kw):
    _, means, quats, scales, opac, mask = walk_scene()
    t = dev_t(dev, pts, means, quats, scales, opac, mask)
    pg = gsbp_amd.point_gaussians(t[0], t[1], t[2], t[3], t[4], k, radius, mask=t[5], return_visited=True, **kw)
    return pg.idx, pg.weights, pg.n_contrib, pg.visited


def check_walk(got, want, k):
    idx, w, nc = (g.cpu().numpy() for g in got[:3])
    assert idx.dtype == np.int32 and w.dtype == F and nc.dtype == np.int32
    assert np.array_equal(nc, want[2])
    assert np.array_equal(idx, want[0][:, :k])  # (the top k of a longer list is its prefix)
    assert ref.same_bits(w, want[1][:, :k])


@pytest.mark.parametrize("k", [1, 8, 32])
def test_walk_equals_the_reference_on_three_grids(dev, k):
    pts = walk_scene()[0]
    want = walk_ref(RADIUS)
    nc = want[2]
    assert (nc > k).mean() > 0.3 and (nc[:Q_JITTER] == 0).sum() < 50 and not nc[Q_JITTER:].any()  # truncated rows; far and bad rows empty
    assert pts.shape[0] == 1024 and np.isin(139, want[0][0])  # the centre at exactly d2 == r2 counts
    dup = (want[0][:, :-1] + 64 == want[0][:, 1:]) & (want[0][:, :-1] < 64) & (want[1][:, :-1] == want[1][:, 1:])
    assert dup.sum() > 100  # bit-identical duplicates sit side by side, the smaller index first
    assert not np.isin(want[0], np.arange(128, 139)).any()
    for cell in (1e6, None, RADIUS / 8.0):  # one cell, the planned grid, cells far smaller than the radius
        got = twice(lambda: run_walk(dev, pts, k, RADIUS, cell_size=cell))
        check_walk(got, want, k)
        visited = got[3].cpu().numpy()
        assert (visited[:Q_JITTER] >= nc[:Q_JITTER]).all() and not visited[-8:].any()
        if cell == 1e6:
            assert (visited[:Q_JITTER + 16] == np.isfinite(walk_scene()[1]).all(axis=1).sum()).all()


def test_walk_radius_edge_infinite_radius_and_odd_query_counts(dev):
    pts = walk_scene()[0]
    below = float(np.nextafter(F(RADIUS), F(0)))
    got = run_walk(dev, pts[:1], 32, below)  # Q = 1; the next radius below drops the centre at RADIUS
    want = cached("below", lambda: ref.point_gaussians(pts[:1], *walk_scene()[1:5], 32, F(F(below) * F(below)), live=walk_scene()[5]))
    check_walk(got, want, 32)
    assert not np.isin(139, want[0][0]) and want[2][0] == walk_ref(RADIUS)[2][0] - 1
    winf = walk_ref(np.inf)
    for cell in (None, 0.05):
        check_walk(twice(lambda: run_walk(dev, pts[:256], 8, float("inf"), cell_size=cell)), winf, 8)
    assert (winf[2] >= walk_ref(RADIUS)[2][:256]).all() and (winf[2] > walk_ref(RADIUS)[2][:256]).any()
    sub = (walk_ref(RADIUS)[0][:131], walk_ref(RADIUS)[1][:131], walk_ref(RADIUS)[2][:131])
    check_walk(run_walk(dev, pts[:131], 8, RADIUS), sub, 8)  # Q not a multiple of the workgroup
    empty = run_walk(dev, pts[:0], 8, RADIUS)
    assert empty[0].shape == (0, 8) and empty[1].shape == (0, 8) and empty[2].shape == (0,)


# ---- the blend -----------------------------------------------------------------------------------------------------------------------------

Q_BLEND, M_BLEND = 512, 2048


def blend_lists(k):
    """idx / w [512, k]: random rows of 2048 with -1 and >= m entries, zero (and -0) weights in front of the rows 0 .. 7, which hold NaN
    and infinities, and all-skipped rows (row 5: every weight 0; row 6: every index outside)."""
    rng = np.random.default_rng(100 + k)
    idx = rng.integers(8, M_BLEND, (Q_BLEND, k)).astype(np.int32)
    w = rng.uniform(0.01, 1.0, (Q_BLEND, k)).astype(F)
    hit = rng.random((Q_BLEND, k))
    idx[hit < 0.05] = -1
    idx[(hit >= 0.05) & (hit < 0.10)] = M_BLEND + 3
    idx[(hit >= 0.10) & (hit < 0.11)] = np.iinfo(np.int32).max
    poison = (hit >= 0.11) & (hit < 0.2)
    idx[poison] = rng.integers(0, 8, int(poison.sum()))
    w[poison] = np.where(rng.random(int(poison.sum())) < 0.5, F(0.0), F(-0.0))
    w[5] = 0.0
    idx[6] = -1
    return idx, w


def blend_feats(d):
    feats = np.random.default_rng(d).standard_normal((M_BLEND, d)).astype(F)
    feats[0:4], feats[4:6], feats[6:8] = np.nan, np.inf, -np.inf
    return feats


@pytest.mark.parametrize("d", [1, 3, 64, 255, 256, 257, 516, 2048])
def test_blend_equals_the_reference_at_every_alignment(dev, d):
    feats = blend_feats(d)
    f_al = torch.from_numpy(feats).to(dev)
    buf = torch.full((M_BLEND * (d + 1) + 1,), float("nan"), device=dev)
    f_off = torch.as_strided(buf, (M_BLEND, d), (d + 1, 1), 1)  # rows at stride D + 1, the base 4 B off a 16-B boundary
    f_off.copy_(f_al)
    assert f_off.data_ptr() % 16 == 4 and f_al.data_ptr() % 16 == 0
    for k in (1, 8, 32):
        idx, w = blend_lists(k)
        want_out, want_w = ref.blend(idx, w, feats)
        ti, tw = dev_t(dev, idx, w)
        out, wsum = twice(lambda: gsbp_amd.neighbor_blend(f_al, ti, tw))
        assert ref.same_bits(wsum.cpu().numpy(), want_w) and ref.same_bits(out.cpu().numpy(), want_out)
        out2, wsum2 = gsbp_amd.neighbor_blend(f_off, ti, tw)
        assert torch.equal(out2, out) and torch.equal(wsum2, wsum)
        o = out.cpu().numpy()
        assert np.isfinite(o).all() and not o[5].any() and not o[6].any() and want_w[5] == 0 and want_w[6] == 0


# ---- the vote ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("classes", [2, 150])
def test_vote_equals_the_reference(dev, classes):
    rng = np.random.default_rng(classes)
    labels = rng.integers(-2, classes + 3, M_BLEND).astype(np.int64)  # some outside [0, K) on both sides
    for k in (1, 8, 32):
        idx, _ = blend_lists(k)
        idx = np.where(idx >= 0, idx % (M_BLEND + 5), idx).astype(np.int32)
        w = (rng.integers(0, 5, idx.shape) * 0.25).astype(F)  # small dyadic weights: exact sums, many ties, some zeros
        idx[7], w[8] = -1, 0.0                                # all-invalid rows
        idx[9] = np.nonzero((labels < 0) | (labels >= classes))[0][:1]
        want = ref.vote(idx, w, labels, classes)
        tl, ti, tw = dev_t(dev, labels, idx, w)
        lab, share = twice(lambda: gsbp_amd.weighted_vote(tl, classes, ti, tw))
        assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), want[0]) and ref.same_bits(share.cpu().numpy(), want[1])
        assert (want[0][[7, 8, 9]] == -1).all() and (want[0] >= 0).sum() > 50
        if k > 1:
            ties = 0
            for g in range(64):  # the reference's ties went to the smallest class
                sums = {}
                for j in range(k):
                    c = int(labels[idx[g, j]]) if 0 <= idx[g, j] < M_BLEND and w[g, j] != 0 else -1
                    if 0 <= c < classes:
                        sums[c] = sums.get(c, 0.0) + float(w[g, j])
                top = [c for c in sums if sums[c] == max(sums.values())]
                ties += len(top) > 1
                assert not top or want[0][g] == min(top)
            assert ties > 0


# ---- the Python layer on the synthetic scene ---------------------------------------------------------------------------------------------

def c1(dev):
    def make():
        splats = syn.make_scene(syn.CONFIGS["C1"])
        gauss = tuple(t.float().to(dev) for t in syn.activate(splats))
        pts = sample.synthetic_points(gauss[0], count=1024)
        feats = regions.synthetic_regions(gauss[0])[0].to(dev)
        return gauss, pts, feats
    return cached("c1", make)


def test_sample_field_and_labels_equal_the_reference_on_the_synthetic_scene(dev):
    gauss, pts, feats = c1(dev)
    pg = gsbp_amd.point_gaussians(pts, *gauss, k=8)
    npg = [g.cpu().numpy() for g in gauss]
    want = cached("c1ref", lambda: ref.point_gaussians(pts.cpu().numpy(), *npg, 8, F(F(pg.radius) * F(pg.radius))))
    check_walk((pg.idx, pg.weights, pg.n_contrib), want, 8)
    assert 0.0 <= pg.beyond_radius <= 0.011 and pg.grid_stats["points_in_cells"] == gauss[0].shape[0]
    out, valid = gsbp_amd.sample_field(feats, pg)
    want_out, want_w = ref.blend(want[0], want[1], feats.cpu().numpy())
    assert ref.same_bits(out.cpu().numpy(), want_out) and np.array_equal(valid.cpu().numpy(), want_w > 0)
    assert int(valid[:1024].sum()) > 900 and not bool(valid[1024:].any())
    # fallback "nearest": the far points take the row of the Gaussian with the nearest centre, valid stays False
    filled, valid2 = gsbp_amd.sample_field(feats, pg, fallback="nearest")
    assert torch.equal(valid2, valid) and torch.equal(filled[valid], out[valid])
    near = torch.cdist(pts[~valid].double(), gauss[0].double()).argmin(dim=1)
    assert torch.equal(filled[~valid], feats[near]) and sample.fallback_rows(pg, valid) == int((~valid).sum()) >= 16
    cut, _ = gsbp_amd.sample_field(feats, pg, fallback="nearest", fallback_radius=1.0)
    assert not bool(cut[1024:].any())
    # labels: the vote, and its counts through miou_recall
    labels = spatial.synthetic_labels(gauss[0], 6)[1]
    lab, share = gsbp_amd.sample_labels(labels, 6, pg)
    want_lab, want_share = ref.vote(want[0], want[1], labels.cpu().numpy(), 6)
    assert np.array_equal(lab.cpu().numpy(), want_lab) and ref.same_bits(share.cpu().numpy(), want_share)
    gt = torch.from_numpy(np.random.default_rng(0).integers(-1, 6, lab.shape[0])).to(dev)
    counts = gsbp_amd.score_point_labels(lab, gt, 6)
    p, t = lab.cpu().numpy(), gt.cpu().numpy()
    ok = t >= 0
    table = np.stack([np.bincount(t[ok & (p == t)], minlength=6), np.bincount(p[ok & (p >= 0)], minlength=6), np.bincount(t[ok], minlength=6)], 1)
    assert np.array_equal(counts.cpu().numpy(), table)
    res = gsbp_amd.miou_recall(counts)
    iou = [table[c, 0] / (table[c, 1] + table[c, 2] - table[c, 0]) for c in range(1, 6)]
    assert res["miou"] == pytest.approx(float(np.mean(iou)))


def test_transfer_field_onto_the_scenes_own_means(dev):
    gauss, _, feats = c1(dev)
    means, quats, scales, opac = gauss
    out, valid, pg = gsbp_amd.transfer_field(means, quats, scales, opac, feats, means, k=32)
    n = means.shape[0]
    me = torch.arange(n, device=dev, dtype=torch.int32)[:, None]
    mine = pg.idx == me
    live = opac >= sample.ALPHA_MIN
    listed = mine.any(dim=1)
    assert not bool(listed[~live].any()) and int(listed.sum()) > 0.9 * n
    assert torch.equal(pg.weights[mine], opac[listed])  # w == o exactly at the Gaussian's own mean
    # a live Gaussian that does not list itself was pushed out by 32 entries that order before (o, its index)
    out_of = live & ~listed
    last_w, last_i = pg.weights[out_of, -1], pg.idx[out_of, -1]
    assert bool(((last_w > opac[out_of]) | ((last_w == opac[out_of]) & (last_i < me[out_of, 0]))).all())
    assert bool((pg.n_contrib[live] >= 1).all()) and bool(valid[live].all()) and out.shape == feats.shape
    # the list's order: weight descending, then index ascending
    w, i = pg.weights.double(), pg.idx.long()
    full = i[:, 1:] >= 0
    assert bool(((w[:, :-1] > w[:, 1:]) | ((w[:, :-1] == w[:, 1:]) & (i[:, :-1] < i[:, 1:])) | ~full).all())
