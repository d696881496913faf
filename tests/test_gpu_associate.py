"""The mask association on the GPU (gwbp_label_overlap, gwbp_label_votes, Engine.label_overlap / label_votes, associate_masks):
both kernels sum fixed-point integers, so every table must equal the numpy form over the view's own weight store (Engine.dump_pairs)
EXACTLY -- whatever the label type, the number of distinct keys per record and per tile, the store layout or the group table -- and
the whole association must equal the numpy reference run on the CPU oracle's blend, bit for bit and from run to run."""
import numpy as np
import pytest
import torch

import associate_ref as ref
from util import scene_np, to_dev

import gsbp_amd
from gsbp_amd import synthetic as syn
from gsbp_amd.associate import WEIGHT_SCALE, associate_masks, quantize_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t1(dev):
    cfg, sc = scene_np("T1")
    return cfg, sc, to_dev(sc, dev)


@pytest.fixture(scope="module")
def eng(t1, dev):
    return gsbp_amd.Engine(t1[0].n_gaussians, t1[0].width, t1[0].height, device=dev)


_PAIRS = {}


def _blended(eng, t1, wide=False, weights=None):
    """View 0 of T1 blended into the weight store (narrow or wide layout, weighted or not) and its (gid, pix, w) triples as numpy,
    read once per kind of blend."""
    cfg, _, g = t1
    eng.set_narrow_scatter(not wide)
    view = eng.view(g["vms"][0], g["K"], cfg.width, cfg.height)
    eng.project(view, g["means"], g["quats"], g["scales"], g["opac"])
    eng.bin_sort(view)
    if weights is not None:
        eng.blend_weighted(view, weights)
    else:
        eng.blend_weights(view)
    key = (wide, weights is not None)
    if key not in _PAIRS:
        _PAIRS[key] = tuple(t.cpu().numpy() for t in eng.dump_pairs(view))
        assert eng.stats()["overflow"] == 0 and len(_PAIRS[key][0]) > 1000
    return view, _PAIRS[key]


def _full(cfg, L, upsample):
    """The map at the view's resolution, as numpy int64."""
    L = L.cpu().to(torch.int64)
    if upsample is None:
        return L.numpy()
    ym, xm = gsbp_amd.nearest_index(L.shape[0], cfg.height), gsbp_amd.nearest_index(L.shape[1], cfg.width)
    return L[ym.long()][:, xm.long()].numpy()


def _groups(n, kind, seed=5):
    g = torch.Generator().manual_seed(seed)
    if kind == "none":
        return torch.full((n,), -1, dtype=torch.int32)
    grp = torch.randint(-1, 63, (n,), generator=g, dtype=torch.int32)  # [-1, 62]: columns 0 .. 63
    if kind == "wild":  # values outside [-1, n_cols - 2] count as -1
        grp[::7], grp[1::7], grp[2::7] = 63, -5, 2 ** 31 - 1
    return grp


def _check_overlap(eng, t1, dev, view, pairs, L, K, group, n_cols, upsample=None, ldo=None):
    cfg = t1[0]
    ldo = n_cols if ldo is None else ldo
    store = torch.full((K + 1, ldo), 7, dtype=torch.int64, device=dev)
    O = store[:, :n_cols]
    O.zero_()
    eng.label_overlap(view, L.to(dev), group.to(dev), O, K, upsample=upsample)
    assert eng.stats()["overflow"] == 0
    want = ref.overlap_table(*pairs, _full(cfg, L, upsample), K, group.numpy(), n_cols)
    assert int(want.sum()) == int(quantize_weights(pairs[2]).sum()) > 0  # every entry lands somewhere: the column sums are complete
    assert torch.equal(O.cpu(), torch.from_numpy(want))
    assert bool((store[:, n_cols:] == 7).all())
    return want


def _check_votes(eng, t1, dev, view, pairs, L, K, remap, n_cols, upsample=None, ldv=None):
    cfg = t1[0]
    ldv = n_cols if ldv is None else ldv
    store = torch.full((cfg.n_gaussians, ldv), 7, dtype=torch.int64, device=dev)
    V = store[:, :n_cols]
    V.zero_()
    eng.label_votes(view, L.to(dev), remap.to(dev), V, K, upsample=upsample)
    assert eng.stats()["overflow"] == 0
    want = ref.add_votes(np.zeros((cfg.n_gaussians, n_cols), np.int64), *pairs, _full(cfg, L, upsample), remap.numpy())
    assert torch.equal(V.cpu(), torch.from_numpy(want))
    assert bool((store[:, n_cols:] == 7).all())
    return want


def _map(cfg, K, dtype, per_pixel=False):
    """Ids in [-1, K + 1]: some are ignored (uint8 wraps them: -1 is 255, outside [0, K) for K <= 255; every byte is a label of 300)."""
    L = syn.make_label_map(cfg, 0, K + 3, per_pixel=per_pixel) - 1
    return (L % 256).to(torch.uint8) if dtype == torch.uint8 else L.to(dtype)


def _remap(K, n_cols, seed=9):
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(-1, n_cols, (K,), generator=g, dtype=torch.int32)
    r[::5] = -1
    return r


DTYPES = [torch.uint8, torch.int16, torch.int32, torch.int64]
CASES = [(K, dt, pp) for K in (1, 5, 300) for dt in DTYPES for pp in (False, True)]
IDS = [f"K{K}-{str(dt).split('.')[1]}-{'pixel' if pp else 'voronoi'}" for K, dt, pp in CASES]


@pytest.mark.parametrize("K, dtype, per_pixel", CASES, ids=IDS)
def test_label_overlap_equals_numpy_exactly(t1, eng, dev, K, dtype, per_pixel):
    """Voronoi maps (a few keys per record) and per-pixel-random maps (more than four distinct labels per record: the left-over path;
    with K = 300 and 64 columns more keys per tile than the 512-slot LDS table holds: the direct path), random groups in 64 columns,
    both store layouts, an O whose rows are wider than n_cols."""
    cfg = t1[0]
    L, group = _map(cfg, K, dtype, per_pixel), _groups(cfg.n_gaussians, "some")
    for wide in (False, True):
        view, pairs = _blended(eng, t1, wide)
        want = _check_overlap(eng, t1, dev, view, pairs, L, K, group, 64, ldo=64 if wide else 67)
    assert want[:K].sum() > 0 and np.count_nonzero(want.sum(axis=0)) == 64
    assert want[K].sum() > 0 or (dtype == torch.uint8 and K > 255)  # the ignored pixels' row


@pytest.mark.parametrize("kind, n_cols", [("none", 64), ("none", 1), ("some", 1), ("wild", 64), ("wild", 3)])
def test_label_overlap_group_conventions(t1, eng, dev, kind, n_cols):
    """group all -1 (everything in column 0), n_cols = 1 (one column whatever group says), and values outside [-1, n_cols - 2],
    which count as -1."""
    cfg = t1[0]
    view, pairs = _blended(eng, t1)
    want = _check_overlap(eng, t1, dev, view, pairs, _map(cfg, 5, torch.int32), 5, _groups(cfg.n_gaussians, kind), n_cols)
    if kind == "none" or n_cols == 1:
        assert want[:, 1:].sum() == 0


def test_low_resolution_map_and_clamped_pixel_weights(t1, eng, dev):
    """upsample="nearest" reads a [17, 23] map through F.interpolate's index maps; an fp32 pixel-weight map with the values 0, 0.5
    and 6 stores weights up to 6 w, which saturate at 4."""
    cfg = t1[0]
    K, group, remap = 7, _groups(cfg.n_gaussians, "some"), _remap(7, 9)
    view, pairs = _blended(eng, t1)
    low = syn.make_label_map(cfg, 1, K + 2, size=(17, 23), n_seeds=40) - 1
    _check_overlap(eng, t1, dev, view, pairs, low, K, group, 64, upsample="nearest")
    _check_votes(eng, t1, dev, view, pairs, low.to(torch.int16), K, remap, 9, upsample="nearest")
    c = torch.tensor([0.0, 0.5, 6.0])[torch.randint(0, 3, (cfg.height, cfg.width), generator=torch.Generator().manual_seed(3))]
    view, pairs = _blended(eng, t1, weights=c.to(dev))
    assert pairs[2].max() > 4.0 and np.isfinite(pairs[2]).all()
    L = _map(cfg, K, torch.int32)
    want = _check_overlap(eng, t1, dev, view, pairs, L, K, group, 64)
    assert int(want.sum()) < int(np.rint(pairs[2].astype(np.float64) * WEIGHT_SCALE).sum())  # the clamp took something away
    _check_votes(eng, t1, dev, view, pairs, L, K, remap, 9)


@pytest.mark.parametrize("K, dtype, per_pixel", CASES, ids=IDS)
def test_label_votes_equals_numpy_exactly(t1, eng, dev, K, dtype, per_pixel):
    """The same grid; remap sends labels to [-1, n_cols), a fifth of them to -1, several to the same column."""
    cfg = t1[0]
    n_cols = 40
    L, remap = _map(cfg, K, dtype, per_pixel), _remap(K, n_cols)
    for wide in (False, True):
        view, pairs = _blended(eng, t1, wide)
        want = _check_votes(eng, t1, dev, view, pairs, L, K, remap, n_cols, ldv=n_cols if wide else n_cols + 3)
    assert want.sum() > 0 or int((remap >= 0).sum()) == 0
    # entries beyond the columns add nothing either (the kernel's own guard; the Engine hands the table over as it is)
    bad = remap.clone()
    bad[bad >= 0] += 1
    view, pairs = _blended(eng, t1)
    _check_votes(eng, t1, dev, view, pairs, L, K, bad, n_cols)


@pytest.mark.parametrize("per_pixel", [False, True])
def test_votes_agree_with_the_float_label_kernel(t1, eng, dev, per_pixel):
    """votes / 2^20 against scatter_labels' F on the same map and store, row by row: every entry rounds by at most 2^-21 (the first
    term, n_entries of the row's Gaussian), and F carries the float kernel's own tolerance of 1e-5 of the row's norm."""
    cfg = t1[0]
    K = 12
    view, pairs = _blended(eng, t1)
    L = syn.make_label_map(cfg, 0, K + 2, per_pixel=per_pixel).to(dev) - 1
    F = torch.zeros(cfg.n_gaussians, K, device=dev)
    eng.scatter_labels(view, L, F, None, K)
    V = torch.zeros(cfg.n_gaussians, K, dtype=torch.int64, device=dev)
    eng.label_votes(view, L, torch.arange(K, dtype=torch.int32, device=dev), V, K)
    Ff = F.cpu().double()
    diff = (V.cpu().double() / WEIGHT_SCALE - Ff).norm(dim=1)
    n_entries = torch.from_numpy(np.bincount(pairs[0], minlength=cfg.n_gaussians)).double()
    bound = n_entries * 2.0 ** -21 + 1e-5 * Ff.norm(dim=1)
    print(f"max diff {float(diff.max()):.3e}, max diff / bound {float((diff / bound.clamp(min=1e-30)).max()):.3f}")
    assert float(Ff.max()) > 0 and bool((diff <= bound).all())


def test_store_without_weights_is_flagged_and_outputs_left_untouched(t1, dev):
    """After the fused blend + scatter kernel the workspace holds no weight store: both calls set overflow bit 2 and add nothing."""
    cfg, _, g = t1
    e = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = e.view(g["vms"][0], g["K"], cfg.width, cfg.height)
    L = syn.make_label_map(cfg, 0, 3).to(dev)
    O = torch.full((4, 5), 3, dtype=torch.int64, device=dev)
    V = torch.full((cfg.n_gaussians, 2), 3, dtype=torch.int64, device=dev)
    for call in (lambda: e.label_overlap(view, L, _groups(cfg.n_gaussians, "some").to(dev), O, 3),
                 lambda: e.label_votes(view, L, torch.tensor([0, 1, -1], dtype=torch.int32, device=dev), V, 3)):
        e.project(view, g["means"], g["quats"], g["scales"], g["opac"])
        e.bin_sort(view)
        e.blend_scatter(view, syn.make_feature_map(cfg, 0, device=dev, dim=4), torch.zeros(cfg.n_gaussians, 4, device=dev), None)
        assert not e.stats()["overflow"] & 4
        call()
        assert e.stats()["overflow"] & 4
    assert bool((O == 3).all()) and bool((V == 3).all())


def test_engine_rejects_what_the_kernels_cannot_read(t1, eng, dev):
    cfg = t1[0]
    view, _ = _blended(eng, t1)
    L = syn.make_label_map(cfg, 0, 3).to(dev)
    grp = torch.zeros(cfg.n_gaussians, dtype=torch.int32, device=dev)
    for O in (torch.zeros(4, 5, device=dev), torch.zeros(3, 5, dtype=torch.int64, device=dev), torch.zeros(4, 5, dtype=torch.int64)):
        with pytest.raises(gsbp_amd.GwbpError):
            eng.label_overlap(view, L, grp, O, 3)
    with pytest.raises(gsbp_amd.GwbpError):
        eng.label_overlap(view, L, grp.long(), torch.zeros(4, 5, dtype=torch.int64, device=dev), 3)
    with pytest.raises(gsbp_amd.GwbpError):
        eng.label_votes(view, L, torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(cfg.n_gaussians, 5, dtype=torch.int64,
                                                                                            device=dev), 3)


@pytest.fixture(scope="module")
def orbit(t1, orc, dev):
    """T1, an 8-view orbit, 4 instances with ids permuted per view in [0, 6): the maps and the CPU oracle's pairs, the numpy
    reference's result and the product's."""
    cfg, _, g = t1
    vms = syn.make_orbit(cfg, 8)
    instance, maps, pairs = ref.oracle_instance_views(orc, cfg, vms, 4, n_ids=6)
    want = ref.associate_ref(pairs, maps, cfg.n_gaussians, 6, max_groups=16)
    dev_maps = [torch.from_numpy(m).to(dev) for m in maps]

    def run():
        return associate_masks(g["means"], g["quats"], g["scales"], g["opac"], vms.to(dev), g["K"], cfg.width, cfg.height,
                               lambda v: dev_maps[v], 6, max_groups=16)
    return dict(cfg=cfg, vms=vms, maps=maps, pairs=pairs, want=want, run=run, got=run(), instance=instance, g=g)


def test_associate_masks_equals_the_reference_on_the_oracle(orbit, dev):
    """maps, groups, votes and n_groups, exactly.  A difference in a single (Gaussian, pixel) weight between the GPU blend and the
    oracle's would show here; it is looked for first and reported as such."""
    cfg, got, want = orbit["cfg"], orbit["got"], orbit["want"]
    e = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, tight_binning=True)
    g = orbit["g"]
    view = e.view(orbit["vms"][0], g["K"], cfg.width, cfg.height)
    e.project(view, g["means"], g["quats"], g["scales"], g["opac"])
    e.bin_sort(view)
    e.blend_weights(view)
    gid, pix, w = (t.cpu().numpy() for t in e.dump_pairs(view))
    rg, rp, rw = orbit["pairs"][0]
    k1, k2 = gid.astype(np.int64) << 32 | pix, rg.astype(np.int64) << 32 | rp
    o1, o2 = np.argsort(k1, kind="stable"), np.argsort(k2, kind="stable")
    assert np.array_equal(k1[o1], k2[o2]), "the set of (Gaussian, pixel) pairs of view 0 differs from the oracle's"
    differ = np.nonzero(w[o1].view(np.uint32) != rw[o2].view(np.uint32))[0]
    assert differ.size == 0, f"{differ.size} pair weights of view 0 differ from the oracle's, first at key {k1[o1][differ[0]]}"
    assert got.n_groups == want["n_groups"] and got.n_groups >= 4
    for v in range(8):
        assert np.array_equal(got.maps[v].cpu().numpy(), want["maps"][v]), v
    assert torch.equal(got.votes.cpu(), torch.from_numpy(want["votes"]))
    assert np.array_equal(got.groups.cpu().numpy(), want["groups"])
    assert [r["view"] for r in got.views] == list(range(8)) and got.views[0]["unassigned_share"] == 1.0
    assert [r["dropped"] for r in got.views] == want["dropped"]
    assert sum(r["matched"] for r in got.views) > 0 and got.views[0]["matched"] == 0
    share, worst, _ = ref.purity(want["groups"], orbit["instance"])
    print(f"8-view orbit: share {share:.4f}, worst majority {worst:.4f}, groups {want['n_groups']}")


def test_two_runs_give_identical_bits(orbit):
    a, b = orbit["got"], orbit["run"]()
    assert a.n_groups == b.n_groups and torch.equal(a.votes, b.votes) and torch.equal(a.groups, b.groups)
    assert all(torch.equal(x, y) for x, y in zip(a.maps, b.maps)) and a.views == b.views


def test_renamed_maps_lift_with_the_existing_label_tools(orbit, dev):
    """associated_label_fn feeds create_label_field; remap_masks keeps ignored pixels ignored."""
    cfg, got, g = orbit["cfg"], orbit["got"], orbit["g"]
    dev_maps = [torch.from_numpy(m).to(dev) for m in orbit["maps"]]
    fn = gsbp_amd.associated_label_fn(got, lambda v: dev_maps[v])
    m0 = fn(0)
    assert m0.dtype == torch.int32 and bool(((m0 >= 0) <= (dev_maps[0] >= 0)).all()) and int(m0.max()) < got.n_groups
    P = gsbp_amd.create_label_field(g["means"], g["quats"], g["scales"], g["opac"], orbit["vms"].to(dev), g["K"], cfg.width, cfg.height,
                                    fn, got.n_groups, pipeline=False)
    n_entries = sum(np.bincount(p[0], minlength=cfg.n_gaussians) for p in orbit["pairs"])
    clear = torch.from_numpy(ref.clear_maximum(got.votes.cpu().numpy(), n_entries)).to(dev)
    assert int(clear.sum()) > 0.8 * int((got.groups >= 0).sum())
    assert torch.equal(P.argmax(dim=1)[clear].int(), got.groups[clear])
