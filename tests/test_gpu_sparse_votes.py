"""The votes into per-Gaussian slot lists on the GPU (gwbp_label_votes_sparse, Engine.label_votes_sparse, associate_masks(votes=
"sparse"), create_sparse_label_field).  The sums are integers and a slot's key never changes once set, so on every row that fits
its slots the canonical lists must equal the numpy reference over the view's own weight store (Engine.dump_pairs) EXACTLY, and on
the rows that do not fit the five invariants of include/gwbp.h must hold -- whatever the order in which the lanes ran."""
import warnings

import numpy as np
import pytest
import torch

import associate_ref as ref
import sparse_votes_ref as sref
from test_gpu_associate import DTYPES, _full, _map
from util import scene_np, to_dev

import gsbp_amd
from gsbp_amd import synthetic as syn
from gsbp_amd.associate import WEIGHT_SCALE, associate_masks, associated_label_fn, create_sparse_label_field
from gsbp_amd.sparse_votes import (SparseVotes, new_sparse_votes, sparse_label_argmax, sparse_label_dense, sparse_votes_canonical,
                                   sparse_votes_dense, sparse_votes_groups, sparse_votes_stats)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t1(dev):
    cfg, sc = scene_np("T1")
    return cfg, sc, to_dev(sc, dev)


@pytest.fixture(scope="module")
def eng(t1, dev):
    return gsbp_amd.Engine(t1[0].n_gaussians, t1[0].width, t1[0].height, device=dev)


_PAIRS = {}


def _blended(eng, t1, wide=False, v=0):
    """View v of T1 blended into the weight store (narrow or wide layout) and its (gid, pix, w) triples as numpy, read once."""
    cfg, _, g = t1
    eng.set_narrow_scatter(not wide)
    view = eng.view(g["vms"][v], g["K"], cfg.width, cfg.height)
    eng.project(view, g["means"], g["quats"], g["scales"], g["opac"])
    eng.bin_sort(view)
    eng.blend_weights(view)
    if (wide, v) not in _PAIRS:
        _PAIRS[wide, v] = tuple(t.cpu().numpy() for t in eng.dump_pairs(view))
        assert eng.stats()["overflow"] == 0 and len(_PAIRS[wide, v][0]) > 1000
    return view, _PAIRS[wide, v]


def _padded(n, S, dev, total=False, pad=(3, 2)):
    """(SparseVotes whose keys and vals are the first S columns of wider stores, the stores): the padding holds 7."""
    k_store = torch.full((n, S + pad[0]), 7, dtype=torch.int32, device=dev)
    v_store = torch.full((n, S + pad[1]), 7, dtype=torch.int64, device=dev)
    keys, vals = k_store[:, :S], v_store[:, :S]
    keys.fill_(-1)
    vals.zero_()
    z = lambda: torch.zeros(n, dtype=torch.int64, device=dev)  # noqa: E731
    return SparseVotes(keys, vals, z(), z() if total else None), (k_store, v_store)


def _np(sv):
    return sv.keys.cpu().numpy(), sv.vals.cpu().numpy(), sv.spill.cpu().numpy()


def _assert_exact(sv, V):
    """Every row fits: no spill, and the canonical lists are the reference's, bit for bit."""
    S = sv.keys.shape[1]
    assert int(sv.spill.abs().sum()) == 0
    sref.check_invariants(*_np(sv), V, S)
    k_ref, v_ref, exact = sref.canonical_lists(V, S)
    assert exact.all()
    c = sparse_votes_canonical(sv)
    assert np.array_equal(c.keys.cpu().numpy(), k_ref) and np.array_equal(c.vals.cpu().numpy(), v_ref)


# remap of the K labels into keys below 40: "distinct" keeps K keys apart (a row can hold all K: the exactly-full boundary at S = K),
# "shared" sends several labels to one key and some to -1
REMAPS = {"distinct": [7, 0, 39, 2, 11], "shared": [3, -1, 17, 3, 17]}
EXACT = [(K, dt, pp, S, kind) for K in (1, 5) for dt in DTYPES for pp in (False, True) for S in (8, 5) for kind in REMAPS]


@pytest.mark.parametrize("K, dtype, per_pixel, S, kind", EXACT,
                         ids=[f"K{K}-{str(dt).split('.')[1]}-{'pixel' if pp else 'voronoi'}-S{S}-{kind}" for K, dt, pp, S, kind in EXACT])
def test_lists_equal_the_reference_exactly_where_nothing_can_overflow(t1, eng, dev, K, dtype, per_pixel, S, kind):
    """At most 5 distinct keys per row, so 8 slots and 5 slots (where the rows with all five keys are exactly full) hold everything:
    spill 0, the canonical lists are the reference's, the dense form is what Engine.label_votes writes, in both store layouts and
    with row strides wider than S, whose padding stays as it was."""
    cfg = t1[0]
    n, n_cols = cfg.n_gaussians, 40
    L, remap = _map(cfg, K, dtype, per_pixel), torch.tensor(REMAPS[kind][:K], dtype=torch.int32)
    for wide in (False, True):
        view, pairs = _blended(eng, t1, wide)
        V = sref.dense_votes(pairs, _full(cfg, L, None), remap.numpy(), n, n_cols)
        sv, (k_store, v_store) = _padded(n, S, dev)
        eng.label_votes_sparse(view, L.to(dev), remap.to(dev), sv, K)
        assert eng.stats()["overflow"] == 0
        _assert_exact(sv, V)
        dense = torch.zeros(n, n_cols, dtype=torch.int64, device=dev)
        eng.label_votes(view, L.to(dev), remap.to(dev), dense, K)
        assert torch.equal(sparse_votes_dense(sv, n_cols), dense) and torch.equal(dense.cpu(), torch.from_numpy(V))
        assert bool((k_store[:, S:] == 7).all()) and bool((v_store[:, S:] == 7).all())
    full = int((sref.distinct_keys(V) == 5).sum())
    print(f"rows with exactly five keys: {full}")
    if K == 5 and per_pixel and kind == "distinct":
        assert full == 3431  # the exactly-full rows at S = 5 (the count on the CPU oracle's view-0 store)
    assert V.sum() > 0


def test_views_accumulate_and_a_second_vote_changes_no_key(t1, eng, dev):
    """View 0, then view 1 with another remap into the same lists: the reference's sum of both.  View 0 voted a second time
    doubles every value and moves no key."""
    cfg = t1[0]
    n, K = cfg.n_gaussians, 5
    L0, L1 = _map(cfg, K, torch.int32, True), (syn.make_label_map(cfg, 1, K + 3) - 1).to(torch.int16)
    r0, r1 = torch.tensor([7, 0, 39, 2, 11], dtype=torch.int32), torch.tensor([0, 5, 7, -1, 21], dtype=torch.int32)  # 7 keys in all
    sv = new_sparse_votes(n, 8, device=dev)
    view, p0 = _blended(eng, t1, v=0)
    eng.label_votes_sparse(view, L0.to(dev), r0.to(dev), sv, K)
    V = sref.dense_votes(p0, _full(cfg, L0, None), r0.numpy(), n, 40)
    _assert_exact(sv, V)
    view, p1 = _blended(eng, t1, v=1)
    eng.label_votes_sparse(view, L1.to(dev), r1.to(dev), sv, K)
    sref.dense_votes(p1, _full(cfg, L1, None), r1.numpy(), n, 40, into=V)
    _assert_exact(sv, V)
    assert int((sref.distinct_keys(V) > 5).sum()) > 0  # rows that hold keys of both views
    before = SparseVotes(sv.keys.clone(), sv.vals.clone(), sv.spill.clone(), None)
    view, _ = _blended(eng, t1, v=0)
    eng.label_votes_sparse(view, L0.to(dev), r0.to(dev), sv, K)
    sref.dense_votes(p0, _full(cfg, L0, None), r0.numpy(), n, 40, into=V)
    _assert_exact(sv, V)
    once = new_sparse_votes(n, 8, device=dev)
    eng.label_votes_sparse(view, L0.to(dev), r0.to(dev), once, K)
    keys1, vals1 = once.keys.clone(), once.vals.clone()
    eng.label_votes_sparse(view, L0.to(dev), r0.to(dev), once, K)
    assert torch.equal(once.keys, keys1) and torch.equal(once.vals, 2 * vals1) and int(vals1.sum()) > 0
    _assert_exact(once, 2 * sref.dense_votes(p0, _full(cfg, L0, None), r0.numpy(), n, 40))
    # keys that were set stay where they are (raw slot order, not the canonical one)
    had = before.keys >= 0
    assert torch.equal(sv.keys[had], before.keys[had]) and bool((sv.vals >= before.vals).all())


OVERFLOW = [(pp, S) for pp in (False, True) for S in (4, 8, 16)]
# the rows that overflow on the CPU oracle's view-0 store, which the GPU's equals pair for pair (test_gpu_associate.py): of 3523
# voting rows with the Voronoi map, and of the per-pixel map at 8 slots
OVERFLOW_ROWS = {(False, 4): 1929, (False, 8): 572, (False, 16): 51, (True, 8): 3489}


@pytest.mark.parametrize("per_pixel, S", OVERFLOW, ids=[f"{'pixel' if pp else 'voronoi'}-S{S}" for pp, S in OVERFLOW])
def test_overflowed_rows_keep_the_invariants(t1, eng, dev, per_pixel, S):
    """300 ids, identity remap: rows with more than S distinct keys spill.  Invariants 1 to 4 against the dense reference: the
    overflowed set is {rows with > S distinct keys}, every slot's value is the dense entry of its key, keys are distinct,
    vals + spill is the row sum, rows without spill are exact (bit for bit in the canonical order)."""
    cfg = t1[0]
    n, K = cfg.n_gaussians, 300
    L, remap = _map(cfg, K, torch.int32, per_pixel), torch.arange(K, dtype=torch.int32)
    view, pairs = _blended(eng, t1)
    V = sref.dense_votes(pairs, _full(cfg, L, None), remap.numpy(), n, K)
    sv = new_sparse_votes(n, S, device=dev)
    eng.label_votes_sparse(view, L.to(dev), remap.to(dev), sv, K)
    assert eng.stats()["overflow"] == 0
    over = sref.check_invariants(*_np(sv), V, S)
    voting = int((V.sum(axis=1) > 0).sum())
    print(f"{int(over.sum())} of {voting} voting rows overflow at S = {S}; stats {sparse_votes_stats(sv)}")
    if not per_pixel:
        assert int(over.sum()) >= 20 and int((~over).sum()) >= 1000, "the fixture no longer exercises both kinds of row"
    if (per_pixel, S) in OVERFLOW_ROWS:
        assert int(over.sum()) == OVERFLOW_ROWS[per_pixel, S] and (per_pixel or voting == 3523)
    k_ref, v_ref, exact = sref.canonical_lists(V, S)
    c = sparse_votes_canonical(sv)
    assert np.array_equal(c.keys.cpu().numpy()[exact], k_ref[exact]) and np.array_equal(c.vals.cpu().numpy()[exact], v_ref[exact])
    groups, certain = sparse_votes_groups(sv)
    ok = certain.cpu().numpy()
    assert np.array_equal(groups.cpu().numpy()[ok], ref.groups_of(V)[ok]) and ok[exact].all()
    assert sparse_votes_stats(sv)["overflow_rows"] == int(over.sum())


@pytest.mark.parametrize("K", [5, 300])
def test_total_is_the_sum_of_every_entry(t1, eng, dev, K):
    """total[g] = sum of q over all of g's entries, the ignored labels' and the -1 remaps' included; without total nothing else
    changes."""
    cfg = t1[0]
    n = cfg.n_gaussians
    L = _map(cfg, K, torch.int16, True)
    remap = torch.arange(K, dtype=torch.int32)
    remap[::3] = -1
    for wide in (False, True):
        view, pairs = _blended(eng, t1, wide)
        with_total, _ = _padded(n, 8, dev, total=True)
        eng.label_votes_sparse(view, L.to(dev), remap.to(dev), with_total, K)
        without = new_sparse_votes(n, 8, device=dev)
        eng.label_votes_sparse(view, L.to(dev), remap.to(dev), without, K)
        want = sref.totals(pairs, n)
        assert np.array_equal(with_total.total.cpu().numpy(), want) and want.sum() > 0
        V = sref.dense_votes(pairs, _full(cfg, L, None), remap.numpy(), n, K)
        assert (want > V.sum(axis=1)).any()  # something was ignored
        for sv in (with_total, without):
            sref.check_invariants(*_np(sv), V, 8)
        a, b = sparse_votes_canonical(with_total), sparse_votes_canonical(without)
        exact = torch.from_numpy(~sref.overflow_rows(V, 8)).to(dev)
        assert torch.equal(a.keys[exact], b.keys[exact]) and torch.equal(a.vals[exact], b.vals[exact])
        # (an overflowed row's spill depends on which keys took its slots, invariant 5; WHICH rows spill does not, and an exact
        # row's spill is zero in both)
        assert torch.equal(with_total.spill > 0, without.spill > 0) and not bool(with_total.spill[exact].any())


def test_store_without_weights_is_flagged_and_the_lists_left_untouched(t1, dev):
    cfg, _, g = t1
    e = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = e.view(g["vms"][0], g["K"], cfg.width, cfg.height)
    L = syn.make_label_map(cfg, 0, 3).to(dev)
    sv = new_sparse_votes(cfg.n_gaussians, 4, device=dev, total=True)
    e.project(view, g["means"], g["quats"], g["scales"], g["opac"])
    e.bin_sort(view)
    e.blend_scatter(view, syn.make_feature_map(cfg, 0, device=dev, dim=4), torch.zeros(cfg.n_gaussians, 4, device=dev), None)
    assert not e.stats()["overflow"] & 4
    e.label_votes_sparse(view, L, torch.tensor([0, 1, -1], dtype=torch.int32, device=dev), sv, 3)
    assert e.stats()["overflow"] & 4
    assert bool((sv.keys == -1).all()) and not bool(sv.vals.any()) and not bool(sv.spill.any()) and not bool(sv.total.any())


def test_engine_rejects_what_the_kernel_cannot_read(t1, eng, dev):
    cfg = t1[0]
    n = cfg.n_gaussians
    view, _ = _blended(eng, t1)
    L = syn.make_label_map(cfg, 0, 3).to(dev)
    remap = torch.zeros(3, dtype=torch.int32, device=dev)
    good = new_sparse_votes(n, 4, device=dev, total=True)
    k0, v0 = torch.empty(n, 0, dtype=torch.int32, device=dev), torch.empty(n, 0, dtype=torch.int64, device=dev)
    k33, v33 = torch.full((n, 33), -1, dtype=torch.int32, device=dev), torch.zeros(n, 33, dtype=torch.int64, device=dev)
    bad = [good._replace(vals=good.vals.double()), good._replace(keys=good.keys.long()), SparseVotes(k0, v0, good.spill, None),
           SparseVotes(k33, v33, good.spill, None), good._replace(keys=good.keys[:, :3]), good._replace(keys=good.keys[:-1]),
           good._replace(spill=good.spill[:-1]), good._replace(total=good.total.int()), good._replace(spill=good.spill.cpu()),
           SparseVotes(*(t.cpu() for t in good)), good._replace(keys=good.keys.t().contiguous().t())]
    for sv in bad:
        with pytest.raises(gsbp_amd.GwbpError):
            eng.label_votes_sparse(view, L, remap, sv, 3)
    for r in (remap[:2], remap.long(), remap.cpu()):  # a short remap, a wrong type, a CPU tensor
        with pytest.raises(gsbp_amd.GwbpError):
            eng.label_votes_sparse(view, L, r, good, 3)
    with pytest.raises(gsbp_amd.GwbpError):  # the library's own check: the same memory for two of the lists
        eng.label_votes_sparse(view, L, remap, good._replace(total=good.spill), 3)
    assert bool((good.keys == -1).all()) and not bool(good.spill.any())
    eng.label_votes_sparse(view, L, remap, good, 3)
    assert int(good.vals.sum()) > 0


# ---- the association and the label field on the slot lists ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orbit(t1, orc, dev):
    """The fixture of test_gpu_associate.py: T1, an 8-view orbit, 4 instances with ids permuted per view in [0, 6), max_groups =
    16; the numpy reference's result on the CPU oracle's pairs, computed once."""
    cfg, _, g = t1
    vms = syn.make_orbit(cfg, 8)
    instance, maps, pairs = ref.oracle_instance_views(orc, cfg, vms, 4, n_ids=6)
    want = ref.associate_ref(pairs, maps, cfg.n_gaussians, 6, max_groups=16)
    dev_maps = [torch.from_numpy(m).to(dev) for m in maps]

    def run(**kw):
        kw.setdefault("max_groups", 16)
        return associate_masks(g["means"], g["quats"], g["scales"], g["opac"], vms.to(dev), g["K"], cfg.width, cfg.height,
                               lambda v: dev_maps[v], 6, votes="sparse", **kw)
    return dict(cfg=cfg, vms=vms, maps=maps, dev_maps=dev_maps, pairs=pairs, want=want, run=run, g=g)


def test_sparse_association_equals_the_reference_at_eight_slots(orbit):
    """No Gaussian of the orbit votes for more than 6 groups: maps, groups and n_groups are the dense reference's, the lists hold
    its votes, nothing spills, two runs give the same canonical lists, and max_groups = 65536 changes nothing."""
    want = orbit["want"]
    got = orbit["run"](slots=8)
    assert got.n_groups == want["n_groups"] and got.n_groups >= 4
    for v in range(8):
        assert np.array_equal(got.maps[v].cpu().numpy(), want["maps"][v]), v
    assert np.array_equal(got.groups.cpu().numpy(), want["groups"])
    assert isinstance(got.votes, SparseVotes) and got.votes.keys.shape == (orbit["cfg"].n_gaussians, 8)
    assert torch.equal(sparse_votes_dense(got.votes, 16).cpu(), torch.from_numpy(want["votes"]))
    assert int(got.votes.spill.abs().sum()) == 0 and [r["overflow_rows"] for r in got.views] == [0] * 8
    assert [r["dropped"] for r in got.views] == want["dropped"] and [r["view"] for r in got.views] == list(range(8))
    k_ref, v_ref, _ = sref.canonical_lists(want["votes"], 8)
    assert np.array_equal(got.votes.keys.cpu().numpy(), k_ref) and np.array_equal(got.votes.vals.cpu().numpy(), v_ref)
    for other in (orbit["run"](slots=8), orbit["run"](slots=8, max_groups=65536)):
        assert other.n_groups == got.n_groups and torch.equal(other.groups, got.groups) and other.views == got.views
        assert all(torch.equal(x, y) for x, y in zip(other.maps, got.maps))
        assert torch.equal(other.votes.keys, got.votes.keys) and torch.equal(other.votes.vals, got.votes.vals)
        assert torch.equal(other.votes.spill, got.votes.spill)


def test_sparse_association_reports_overflow_at_four_slots(orbit):
    """288 Gaussians of the orbit end with 5 or 6 groups: "raise" raises at the first view that leaves a row with spill, "warn"
    warns once and counts the rows per view."""
    with pytest.raises(gsbp_amd.GwbpError, match="more than 4 distinct groups"):
        orbit["run"](slots=4, on_overflow="raise")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = orbit["run"](slots=4, on_overflow="warn")
    said = [w for w in caught if issubclass(w.category, RuntimeWarning) and "distinct groups" in str(w.message)]
    assert len(said) == 1 and "same on every run" in str(said[0].message)
    rows = [r["overflow_rows"] for r in got.views]
    print(f"overflow rows per view at 4 slots: {rows}")
    assert rows[-1] > 0 and rows == sorted(rows) and rows[-1] == int((got.votes.spill > 0).sum())
    with pytest.raises(ValueError):
        orbit["run"](slots=4, on_overflow="ignore")


def test_sparse_label_field_agrees_with_the_dense_one(orbit, dev):
    """create_sparse_label_field on the orbit's renamed maps against create_label_field: the same argmax on the rows
    associate_ref.clear_maximum calls clear, and the same fractions to the bound of
    test_gpu_associate.py::test_votes_agree_with_the_float_label_kernel -- in units of blend weight a row of integer sums lies
    within n_entries * 2^-21 (every entry rounds by at most half a step of 2^-20) + 1e-5 * |F| (the float kernel's tolerance) of F,
    the numerator create_label_field returns beside P = F / d.  That bound, unchanged, is asserted twice: for the integer sums
    behind the fractions (the association's lists: the same keys, no narrowing anywhere), and for the fractions themselves taken
    back to blend weight with their own exact denominator, fractions * total / 2^20.  total is d in fixed point under the same
    bound."""
    cfg, g, want = orbit["cfg"], orbit["g"], orbit["want"]
    assoc = orbit["run"](slots=8)
    fn = associated_label_fn(assoc, lambda v: orbit["dev_maps"][v])
    args = (g["means"], g["quats"], g["scales"], g["opac"], orbit["vms"].to(dev), g["K"], cfg.width, cfg.height, fn, assoc.n_groups)
    field = create_sparse_label_field(*args, slots=8)
    P, F, d, _ = gsbp_amd.create_label_field(*args, pipeline=False, return_partials=True)
    assert field.ids.shape == (cfg.n_gaussians, 8) and field.ids.dtype == torch.int32 and field.fractions.dtype == torch.float32
    assert field.total.dtype == torch.int64 and not bool(field.spill_fraction.any())
    n_entries = torch.from_numpy(sum(np.bincount(p[0], minlength=cfg.n_gaussians) for p in orbit["pairs"])).double()
    clear = torch.from_numpy(ref.clear_maximum(want["votes"], n_entries.numpy())).to(dev)
    assert int(clear.sum()) > 0.8 * int((assoc.groups >= 0).sum())
    assert torch.equal(sparse_label_argmax(field)[clear], P.argmax(dim=1)[clear])
    assert torch.equal(sparse_label_argmax(field)[clear].int(), assoc.groups[clear])
    # the field IS the association's lists over the total: the same canonical keys, exact integers behind the fractions
    assert torch.equal(field.ids, assoc.votes.keys)
    Ff = F.cpu().double()
    assert Ff.shape == (cfg.n_gaussians, assoc.n_groups)
    bound = n_entries * 2.0 ** -21 + 1e-5 * Ff.norm(dim=1)
    integers = sparse_votes_dense(assoc.votes, assoc.n_groups).cpu().double() / WEIGHT_SCALE
    mine = sparse_label_dense(field, assoc.n_groups).cpu().double() * (field.total.cpu().double() / WEIGHT_SCALE)[:, None]
    for name, x in (("integer sums", integers), ("fractions * total", mine)):
        diff = (x - Ff).norm(dim=1)
        print(f"{name}: max diff {float(diff.max()):.3e}, max diff / bound {float((diff / bound.clamp(min=1e-30)).max()):.3f}")
        assert float(Ff.max()) > 0 and bool((diff <= bound).all()), name
    dd = d.cpu().double().reshape(-1)
    assert bool(((field.total.cpu().double() / WEIGHT_SCALE - dd).abs() <= n_entries * 2.0 ** -21 + 1e-5 * dd).all())
    rows = field.fractions.sum(dim=1) + field.spill_fraction
    assert float(rows.max()) <= 1.0 + 1e-6
