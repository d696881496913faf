"""No-GPU checks of the per-Gaussian slot lists (gsbp_amd.sparse_votes): the host functions on random tables, the argument checks
of gwbp_label_votes_sparse (no HIP call), the header's contract, and what compressing the reference association's dense votes
loses on the CPU oracle's orbit (nothing at 8 slots; 288 rows at 4)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import associate_ref as ref
import sparse_votes_ref as sref
import gsbp_amd
from gsbp_amd import _lib, synthetic as syn
from gsbp_amd.associate import group_of_votes
from gsbp_amd.sparse_votes import (SparseVotes, new_sparse_votes, sparse_label_argmax, sparse_label_dense, sparse_label_field_of,
                                   sparse_votes_bytes, sparse_votes_canonical, sparse_votes_dense, sparse_votes_groups,
                                   sparse_votes_stats)


def _lists_of(V, S, rng):
    """A SparseVotes a run could have left for the dense table V (numpy int64 [n, K]): every row's non-zero entries in a random
    arrival order, the first S of them in the slots 0, 1, ... (a lane takes the first empty slot), the rest in the spill."""
    n = V.shape[0]
    keys, vals, spill = np.full((n, S), -1, np.int32), np.zeros((n, S), np.int64), np.zeros(n, np.int64)
    for g in range(n):
        cols = rng.permutation(np.nonzero(V[g])[0])
        keys[g, :min(S, len(cols))] = cols[:S]
        vals[g, :min(S, len(cols))] = V[g, cols[:S]]
        spill[g] = V[g, cols[S:]].sum()
    return SparseVotes(torch.from_numpy(keys), torch.from_numpy(vals), torch.from_numpy(spill), None)


def _random_table(rng, n=400, K=23):
    V = rng.integers(1, 5, size=(n, K)).astype(np.int64) * (1 << 18)  # few distinct values: many ties
    V[rng.random(V.shape) < 0.75] = 0
    V[::17] = 0  # empty rows
    return V


@pytest.mark.parametrize("S", [1, 4, 8, 32])
def test_host_functions_on_random_tables(S):
    rng = np.random.default_rng(S)
    V = _random_table(rng)
    sv = _lists_of(V, S, rng)
    over = sref.check_invariants(sv.keys.numpy(), sv.vals.numpy(), sv.spill.numpy(), V, S)  # (the generator obeys the contract)
    assert over.any() == (S < 32) and (~over).sum() > 20  # (24 rows are empty)
    exact = torch.from_numpy(~over)
    # groups: group_of_votes of the dense table on every row without spill, ties (the smallest key) and empty rows included
    groups, certain = sparse_votes_groups(sv)
    want = group_of_votes(torch.from_numpy(V))
    assert groups.dtype == torch.int32 and torch.equal(groups[exact], want[exact])
    assert int((want[exact] == -1).sum()) > 0
    best2 = np.sort(V, axis=1)[:, -2:]
    assert int((best2[~over, 0] == best2[~over, 1]).sum()) > 0, "the tables must hold ties for the argmax"
    assert bool(certain[exact].all())
    # certain rows with spill: the best kept value beats the whole spill, so it beats every left-out key
    sure = certain & ~exact
    assert torch.equal(groups[sure], want[sure])
    # canonical: value descending, key ascending, empties last; idempotent; the reference's lists on exact rows
    c = sparse_votes_canonical(sv)
    cc = sparse_votes_canonical(c)
    assert torch.equal(c.keys, cc.keys) and torch.equal(c.vals, cc.vals) and c.spill is sv.spill
    k_ref, v_ref, ex = sref.canonical_lists(V, S)
    assert np.array_equal(ex, ~over)
    assert np.array_equal(c.keys.numpy()[ex], k_ref[ex]) and np.array_equal(c.vals.numpy()[ex], v_ref[ex])
    sref.check_invariants(c.keys.numpy(), c.vals.numpy(), c.spill.numpy(), V, S)
    # dense o canonical round-trips (every row: a slot's value lands in its key's column)
    D = sparse_votes_dense(c, V.shape[1])
    assert torch.equal(D, sparse_votes_dense(sv, V.shape[1])) and torch.equal(D[exact], torch.from_numpy(V)[exact])
    assert torch.equal(D.sum(dim=1) + sv.spill, torch.from_numpy(V.sum(axis=1)))
    with pytest.raises(gsbp_amd.GwbpError):
        sparse_votes_dense(sv, int(sv.keys.max()))
    st = sparse_votes_stats(sv)
    assert st["overflow_rows"] == int(over.sum()) and st["rows"] == V.shape[0] and st["slots"] == S
    assert st["slots_in_use"] == np.bincount(np.minimum((V != 0).sum(axis=1), S), minlength=S + 1).tolist()
    assert st["spilled_share"] == pytest.approx(float(sv.spill.sum()) / float(V.sum())) and st["uncertain_rows"] == int((~certain).sum())


def test_new_sparse_votes_and_the_label_field_form():
    sv = new_sparse_votes(7, 3, total=True)
    assert sv.keys.dtype == torch.int32 and bool((sv.keys == -1).all()) and sv.vals.dtype == torch.int64 and sv.total.shape == (7,)
    assert new_sparse_votes(7).keys.shape == (7, 8) and new_sparse_votes(7).total is None
    assert sparse_votes_bytes(10 ** 6, 8) == 104 * 10 ** 6 and sparse_votes_bytes(10, 4, total=True) == 10 * 64
    for bad in (0, 33, -1):
        with pytest.raises(gsbp_amd.GwbpError):
            new_sparse_votes(7, bad)
    with pytest.raises(gsbp_amd.GwbpError):
        sparse_label_field_of(new_sparse_votes(7, 3))
    # row 0: classes 5 (1/4) and 2 (1/2), a quarter ignored; row 1: a tie, the smaller id first; row 2: untouched; row 3: spill
    sv.keys[0, :2], sv.vals[0, :2], sv.total[0] = torch.tensor([5, 2]), torch.tensor([1 << 20, 2 << 20]), 4 << 20
    sv.keys[1, :2], sv.vals[1, :2], sv.total[1] = torch.tensor([9, 3]), torch.tensor([3, 3]), 6
    sv.keys[3], sv.vals[3], sv.spill[3], sv.total[3] = torch.tensor([1, 0, 4]), torch.tensor([1, 1, 1]), 5, 8
    f = sparse_label_field_of(sv)
    assert f.ids.tolist()[:2] == [[2, 5, -1], [3, 9, -1]] and f.fractions.dtype == torch.float32
    assert f.fractions[0].tolist() == [0.5, 0.25, 0.0] and f.spill_fraction.tolist()[3] == 0.625 and f.total is sv.total
    assert sparse_label_argmax(f).tolist() == [2, 3, -1, 0, -1, -1, -1]
    P = sparse_label_dense(f, 10)
    assert P.shape == (7, 10) and P[0, 2] == 0.5 and P[0, 5] == 0.25 and float(P[2].sum()) == 0.0
    with pytest.raises(gsbp_amd.GwbpError):
        sparse_label_dense(f, 9)


# ---- the C ABI: every rejected argument, before any HIP call (the pattern of test_associate_cpu.py) ---------------------------------
# argument indices behind (caps, workspace, workspace_bytes, view): labels 4, label_type 5, ls_y 6, ls_x 7, num_labels 8, ymap 9,
# xmap 10, remap 11, slots 12, keys 13, ld_keys 14, vals 15, ld_vals 16, spill 17, total 18, stream 19.  The caps say N = 10 rows:
# keys span 160 B, vals 320 B, spill and total 80 B each at slots = ld = 4
REJECTED = [({5: 3}, b"unknown label type"), ({5: -1}, b"unknown label type"), ({8: 0}, b"num_labels must be positive"),
            ({8: -2}, b"num_labels must be positive"), ({11: None}, b"null remap"), ({12: 0}, b"slots must lie in [1, 32]"),
            ({12: 33}, b"slots must lie in [1, 32]"), ({12: -4}, b"slots must lie in [1, 32]"), ({14: 3}, b"ld_keys 3 < slots 4"),
            ({16: 3}, b"ld_vals 3 < slots 4"), ({12: 5}, b"ld_keys 4 < slots 5"), ({13: None}, b"keys must be a non-null"),
            ({15: None}, b"vals must be a non-null"), ({17: None}, b"spill must be a non-null"), ({13: "+2"}, b"keys must be"),
            ({15: "+4"}, b"vals must be"), ({17: "+4"}, b"spill must be"), ({18: "+4"}, b"total must be"),
            ({15: "keys"}, b"keys and vals overlap"), ({15: "keys+152"}, b"keys and vals overlap"),
            ({17: "keys+8"}, b"keys and spill overlap"), ({18: "keys"}, b"keys and total overlap"),
            ({17: "vals+312"}, b"vals and spill overlap"), ({18: "vals+160"}, b"vals and total overlap"),
            ({18: "spill+72"}, b"spill and total overlap"), ({18: "spill"}, b"spill and total overlap"),
            ({14: 40, 15: "keys+16"}, b"keys and vals overlap"),  # wide rows: the lists interleave, and so they overlap
            ({4: None}, b"bad label map"), ({6: -1}, b"bad label map"), ({7: -1}, b"bad label map"),
            ({9: None}, b"both index maps or neither"), ({10: None}, b"both index maps or neither")]


def test_sparse_entry_point_rejects_bad_arguments_before_any_device_call():
    L = _lib.lib()
    small = _lib.Caps(10, 1 << 16, 1 << 20, 64, 64)
    nbytes = C.c_size_t(0)
    assert L.gwbp_workspace_size(C.byref(small), C.byref(nbytes)) == 0
    view = _lib.View()
    view.width, view.height = 64, 64
    view.K[0] = view.K[4] = 50.0
    buf = (C.c_char * 8192)()
    addr = (C.addressof(buf) + 255) & ~255
    fake = C.c_void_p(addr)
    at = dict(keys=addr + 1024, vals=addr + 2048, spill=addr + 3072, total=addr + 4096)  # disjoint, never dereferenced
    f = L.gwbp_label_votes_sparse
    assert _lib.ARGTYPES["gwbp_label_votes_sparse"][:4] == _lib._WSV and len(_lib.ARGTYPES["gwbp_label_votes_sparse"]) == 20

    def args_of(own):
        args = [C.byref(small), fake, nbytes, C.byref(view), fake, _lib.LABEL_I16, 4, 1, 4, fake, fake, fake, 4,
                C.c_void_p(at["keys"]), 4, C.c_void_p(at["vals"]), 4, C.c_void_p(at["spill"]), C.c_void_p(at["total"]), None]
        names = {13: "keys", 15: "vals", 17: "spill", 18: "total"}
        for i, val in own.items():
            if isinstance(val, str):
                base, _, off = val.partition("+")
                val = C.c_void_p(at[base or names[i]] + int(off or 0))
            args[i] = val
        return args

    for own, msg in REJECTED:
        assert f(*args_of(own)) == -1, (own, L.gwbp_last_error_string())
        assert msg in L.gwbp_last_error_string(), (own, L.gwbp_last_error_string())
    # the caps, the workspace and the view come first, as for every call on a view
    args = args_of({5: 99, 12: 0})
    args[0] = None
    assert f(*args) == -1 and b"null caps" in L.gwbp_last_error_string()
    args = args_of({5: 99})
    args[3] = None
    assert f(*args) == -1 and b"null view" in L.gwbp_last_error_string()


def test_header_documents_the_contract():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gwbp.h")).read()
    for s in ("GWBP_API int gwbp_label_votes_sparse(", "#define GWBP_SPARSE_MAX_SLOTS 32", "-1 = empty", "never evicted",
              "never appears twice in a row", "first empty slot in index order", "spill[g] > 0 exactly when",
              "value descending, then key ascending, empties last", "there is no column count"):
        assert s in hdr, s
    assert "gwbp_label_votes_sparse" in _lib.EXPORTS and _lib.SPARSE_MAX_SLOTS == 32
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "4.0b" in design and "gwbp_label_votes_sparse" in design
    for name in ("SparseVotes", "new_sparse_votes", "sparse_votes_canonical", "sparse_votes_groups", "sparse_votes_dense",
                 "sparse_votes_stats", "SparseLabelField", "create_sparse_label_field", "sparse_label_argmax", "sparse_label_dense"):
        assert hasattr(gsbp_amd, name), name


# ---- the reference association's votes, compressed ---------------------------------------------------------------------------------
def test_orbit_votes_fit_eight_slots_and_overflow_288_rows_at_four(orc):
    """T1, the 8-view orbit of the GPU tests (4 instances, ids permuted per view in [0, 6), max_groups = 16): the reference opens 8
    groups and no Gaussian votes for more than 6 of them -- 16, 5, 101, 1608, 1982, 286 and 2 Gaussians have 0 .. 6 distinct
    groups.  So 8 slots lose nothing and the argmax is unchanged; 4 slots overflow exactly the 288 rows with 5 or 6."""
    cfg = syn.CONFIGS["T1"]
    vms = syn.make_orbit(cfg, 8)
    _, maps, pairs = ref.oracle_instance_views(orc, cfg, vms, 4, n_ids=6)
    want = ref.associate_ref(pairs, maps, cfg.n_gaussians, 6, max_groups=16)
    V = want["votes"]
    assert want["n_groups"] == 8
    assert np.bincount(sref.distinct_keys(V)).tolist() == [16, 5, 101, 1608, 1982, 286, 2]
    rng = np.random.default_rng(0)
    sv = _lists_of(V, 8, rng)
    assert not sref.check_invariants(sv.keys.numpy(), sv.vals.numpy(), sv.spill.numpy(), V, 8).any()
    assert torch.equal(sparse_votes_dense(sv, 16), torch.from_numpy(V))
    assert np.array_equal(sparse_votes_groups(sv)[0].numpy(), want["groups"])
    assert sparse_votes_stats(sv)["overflow_rows"] == 0 and sparse_votes_stats(sv)["slots_in_use"][:7] == [16, 5, 101, 1608, 1982, 286, 2]
    assert int(sref.overflow_rows(V, 4).sum()) == 288
    sv4 = _lists_of(V, 4, rng)
    assert int(sref.check_invariants(sv4.keys.numpy(), sv4.vals.numpy(), sv4.spill.numpy(), V, 4).sum()) == 288
    groups4, certain4 = sparse_votes_groups(sv4)
    assert np.array_equal(groups4.numpy()[certain4.numpy()], want["groups"][certain4.numpy()]) and int((~certain4).sum()) <= 288
