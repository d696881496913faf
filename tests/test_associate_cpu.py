"""No-GPU checks of the mask association (gsbp_amd.associate): match_masks on hand-made tables and against the numpy reference,
the quantisation contract, the argument checks of gwbp_label_overlap / gwbp_label_votes (no HIP call), and the whole algorithm
end to end on the CPU oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import associate_ref as ref
from gsbp_amd import _lib, synthetic as syn
from gsbp_amd.associate import WEIGHT_CLAMP, WEIGHT_SCALE, match_masks, quantize_weights, remap_masks

S = WEIGHT_SCALE


def _table(rows, n_cols):
    """int64 [len(rows) + 1, n_cols] from {(m, col): units of blend weight}; the last row (ignored pixels) may be addressed too."""
    O = np.zeros((len(rows) + 1, n_cols), np.int64)
    for m, row in enumerate(rows):
        for col, x in row.items():
            O[m, col] = int(x * S)
    return O


def test_iou_tie_goes_to_the_smaller_mask_then_the_smaller_group():
    # masks 0 and 1 overlap group 0 alike (iou 4 / (4 + 8 - 4) = 0.5 each); mask 1 overlaps group 1 with the same iou
    O = _table([{1: 4}, {1: 4, 2: 4}], 3)
    O[1, 2] = 4 * S
    A1 = int(O[1].sum())
    assert A1 == 8 * S
    # iou(0,0) = 4/(4+8-4) = .5; iou(1,0) = 4/(8+8-4) = 1/3; iou(1,1) = 4/(8+4-4) = .5  -> (0,0) before (1,1) by m; both taken
    remap, n, c = match_masks(O, 2, return_counts=True)
    assert remap.tolist() == [0, 1] and n == 2 and c == dict(matched=2, opened=0, dropped=0, dead=0)
    # two masks, one group, the same iou: the smaller mask takes it, the other opens a group
    O = _table([{1: 3, 0: 1}, {1: 3, 0: 1}], 2)
    remap, n = match_masks(O, 1)
    assert remap.tolist() == [0, 1] and n == 2
    # one mask, two groups, the same iou: the smaller group
    O = _table([{1: 3, 2: 3}], 3)
    assert match_masks(O, 2)[0].tolist() == [0]


def test_two_masks_want_one_group_the_higher_iou_wins():
    O = _table([{1: 2, 0: 6}, {1: 6, 0: 1}], 2)  # iou 2/(8+8-2) = 1/7 < 0.2 ... use a lower bar to make both candidates
    remap, n, c = match_masks(O, 1, iou_min=0.1, return_counts=True)
    assert remap.tolist() == [1, 0] and n == 2 and c["matched"] == 1 and c["opened"] == 1
    assert match_masks(O, 1, iou_min=0.2)[0].tolist() == [1, 0]  # (mask 0 is no candidate at all now: the same outcome)


def test_max_groups_exhausted_counts_the_dropped_masks():
    O = _table([{0: 2}, {0: 2}, {0: 2}, {0: 0.5}], 3)
    remap, n, c = match_masks(O, 0, max_groups=2, return_counts=True)
    assert remap.tolist() == [0, 1, -1, -1] and n == 2
    assert c == dict(matched=0, opened=2, dropped=1, dead=1)
    remap, n, c = match_masks(O, 2, max_groups=2, return_counts=True)  # already full: nothing opens
    assert remap.tolist() == [-1, -1, -1, -1] and n == 2 and c["dropped"] == 3


def test_min_mass_no_groups_and_an_empty_table():
    O = _table([{0: 1}, {0: 1 - 2.0 ** -20}, {0: 0.5, 1: 0.5}], 2)
    remap, n, c = match_masks(O, 0, return_counts=True)  # exactly min_mass is live, one step below is dead
    assert remap.tolist() == [0, -1, 1] and n == 2 and c["dead"] == 1
    assert match_masks(O, 0, min_mass=0.25)[0].tolist() == [0, 1, 2]
    remap, n, c = match_masks(np.zeros((4, 5), np.int64), 3, return_counts=True)
    assert remap.tolist() == [-1, -1, -1] and n == 3 and c == dict(matched=0, opened=0, dropped=0, dead=3)
    remap, n = match_masks(np.zeros((3, 1), np.int64), 0)
    assert remap.tolist() == [-1, -1] and n == 0
    # the ignored row counts in a group's mass: iou 4 / (4 + (4 + 20) - 4) = 1/6 with it, 1 without
    O = _table([{1: 4}], 2)
    O[1, 1] = 20 * S
    assert match_masks(O, 1)[0].tolist() == [1]
    assert match_masks(torch.from_numpy(O), 1, iou_min=0.1)[0].tolist() == [0]


def test_match_masks_equals_the_reference_on_random_tables():
    rng = np.random.default_rng(7)
    for case in range(200):
        K, G = int(rng.integers(1, 9)), int(rng.integers(0, 7))
        O = rng.integers(0, 6, size=(K + 1, G + 1 + int(rng.integers(0, 3)))).astype(np.int64) * (S // 2)  # many ties
        O[rng.random(O.shape) < 0.4] = 0
        O[:, G + 1:] = 0
        if case % 3 == 0:
            O += rng.integers(0, 1000, size=O.shape)
        max_groups = G + int(rng.integers(0, 4))
        iou_min = float(rng.choice([0.0, 0.1, 0.2, 0.5]))
        min_mass = float(rng.choice([0.0, 0.5, 1.0, 2.0]))
        remap, n, c = match_masks(O, G, iou_min, min_mass, max_groups, return_counts=True)
        r_remap, r_n, r_drop = ref.match_ref(O, G, iou_min, min_mass, max_groups)
        assert remap.dtype == np.int32 and np.array_equal(remap, r_remap) and n == r_n and c["dropped"] == r_drop, case


def test_quantize_weights_contract():
    w = np.array([0.0, -1.0, -0.0, np.nan, 4.0, 5.0, np.inf, -np.inf, 2.0 ** -21, 1.5 * 2.0 ** -20, 2.5 * 2.0 ** -20, 1.0,
                  0.75 * 2.0 ** -20], np.float32)
    want = [0, 0, 0, 0, 4 * S, 4 * S, 4 * S, 0, 0, 2, 2, S, 1]
    q = quantize_weights(w)
    assert q.dtype == np.int64 and q.tolist() == want
    qt = quantize_weights(torch.from_numpy(w))
    assert qt.dtype == torch.int64 and qt.tolist() == want
    assert WEIGHT_CLAMP == 4.0 and S == 2 ** 20
    rng = np.random.default_rng(1)
    x = (rng.random(10000) * 1.2 - 0.1).astype(np.float32)
    assert np.array_equal(quantize_weights(x), quantize_weights(torch.from_numpy(x)).numpy())


def test_remap_masks_ignores_ids_outside_the_table():
    L = torch.tensor([[0, 1, 2], [-1, 3, 200]], dtype=torch.int16)
    out = remap_masks(L, np.array([5, -1, 7], np.int32))
    assert out.dtype == torch.int32 and out.tolist() == [[5, -1, 7], [-1, -1, -1]]
    assert remap_masks(torch.tensor([[200, 1]], dtype=torch.uint8), torch.tensor([4, 9], dtype=torch.int32)).tolist() == [[-1, 9]]


# ---- the C ABI: every rejected argument, before any HIP call (the pattern of test_capi_cpu.py) -----------------------------------
# argument indices behind (caps, workspace, workspace_bytes, view): labels 4, label_type 5, ls_y 6, ls_x 7, num_labels 8, ymap 9,
# xmap 10, group / remap 11, n_cols 12, O / V 13, ldo / ldv 14, stream 15
REJECTED = [({5: 3}, b"unknown label type"), ({5: -1}, b"unknown label type"), ({8: 0}, b"num_labels must be positive"),
            ({8: -2}, b"num_labels must be positive"), ({12: 0}, b"n_cols must be positive"), ({14: 3}, b"< n_cols 4"),
            ({4: None}, b"bad label map"), ({11: None}, b"null "), ({13: None}, b"8-B aligned"), ({13: "odd"}, b"8-B aligned"),
            ({6: -1}, b"bad label map"), ({7: -1}, b"bad label map"), ({9: None}, b"both index maps or neither"),
            ({10: None}, b"both index maps or neither")]


@pytest.mark.parametrize("name", ["gwbp_label_overlap", "gwbp_label_votes"])
def test_association_entry_points_reject_bad_arguments_before_any_device_call(name):
    L = _lib.lib()
    small = _lib.Caps(10, 1 << 16, 1 << 20, 64, 64)
    nbytes = C.c_size_t(0)
    assert L.gwbp_workspace_size(C.byref(small), C.byref(nbytes)) == 0
    view = _lib.View()
    view.width, view.height = 64, 64
    view.K[0] = view.K[4] = 50.0
    buf = (C.c_char * 512)()
    addr = (C.addressof(buf) + 255) & ~255
    fake = C.c_void_p(addr)
    f = getattr(L, name)
    assert _lib.ARGTYPES[name][:4] == _lib._WSV and len(_lib.ARGTYPES[name]) == 16
    for own, msg in REJECTED:
        args = [C.byref(small), fake, nbytes, C.byref(view), fake, _lib.LABEL_I16, 4, 1, 4, fake, fake, fake, 4, fake, 4, None]
        for i, val in own.items():
            args[i] = C.c_void_p(addr + 4) if val == "odd" else val
        assert f(*args) == -1, (own, L.gwbp_last_error_string())
        assert msg in L.gwbp_last_error_string(), (own, L.gwbp_last_error_string())
    # the caps, the workspace and the view come first, as for every call on a view
    args = [None, fake, nbytes, C.byref(view), fake, 99, 4, 1, 4, fake, fake, fake, 4, fake, 4, None]
    assert f(*args) == -1 and b"null caps" in L.gwbp_last_error_string()


def test_header_documents_the_contract():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gwbp.h")).read()
    for s in ("GWBP_API int gwbp_label_overlap(", "GWBP_API int gwbp_label_votes(", "rintf(fminf(fmaxf(w, 0), 4) * 1048576)"):
        assert s in hdr
    assert "gwbp_label_overlap" in _lib.EXPORTS and "gwbp_label_votes" in _lib.EXPORTS


# ---- the whole algorithm on the CPU oracle -----------------------------------------------------------------------------------------
def test_orbit_association_recovers_the_instances(orc):
    """T1, a 16-view orbit (synthetic.make_orbit), the 4-site 3-D Voronoi partition of synthetic.make_instances (seed 60000), per
    view the argmax map of the oracle's render with ids permuted per view, iou_min = 0.2, min_mass = 1.  The reference groups
    3984 Gaussians; 0.8986 of them lie in a group whose majority instance is their own (3580), the least pure non-empty group
    has a majority share of 0.830, and four large groups (1404, 1199, 1010, 363) form for the four instances beside two of 2 and
    6 Gaussians.  This pins the algorithm (and the fixture), not the kernels."""
    cfg = syn.CONFIGS["T1"]
    vms = syn.make_orbit(cfg, 16)
    instance, maps, pairs = ref.oracle_instance_views(orc, cfg, vms, 4)
    for v in (0, 5):  # ids are unrelated between the views: a permutation of [0, 4) each, -1 where alpha < 0.5
        assert set(np.unique(maps[v])) <= {-1, 0, 1, 2, 3} and (maps[v] >= 0).any()
    r = ref.associate_ref(pairs, maps, cfg.n_gaussians, 4)
    share, worst, n_nonempty = ref.purity(r["groups"], instance)
    print(f"grouped {(r['groups'] >= 0).sum()} share {share:.4f} worst majority {worst:.4f} groups {r['n_groups']} "
          f"non-empty {n_nonempty}")
    assert (r["groups"] >= 0).sum() > 0.9 * cfg.n_gaussians
    assert share >= 0.8
    assert worst > 0.5
    # the product's host half on the same tables: match_masks view by view reproduces the reference's maps
    V = np.zeros((cfg.n_gaussians, 256), np.int64)
    group, n_groups = np.full(cfg.n_gaussians, -1, np.int32), 0
    for v in range(len(maps)):
        O = ref.overlap_table(*pairs[v], maps[v], 4, group, 257)
        remap, n_groups = match_masks(O, n_groups)
        assert np.array_equal(remap, r["maps"][v]), v
        ref.add_votes(V, *pairs[v], maps[v], remap)
        group = ref.groups_of(V)
    assert n_groups == r["n_groups"] and np.array_equal(group, r["groups"])


def test_make_orbit_is_evenly_spaced_and_looks_at_the_origin():
    cfg = syn.CONFIGS["T1"]
    vms = syn.make_orbit(cfg, 8, elevation_deg=30.0, radius=2.0)
    assert vms.shape == (8, 4, 4)
    R, t = vms[:, :3, :3], vms[:, :3, 3]
    c = -(R.transpose(1, 2) @ t[:, :, None])[:, :, 0]
    assert torch.allclose(c.norm(dim=1), torch.full((8,), 2.0), atol=1e-5)
    assert torch.allclose(c[:, 2], torch.full((8,), 2.0 * float(np.sin(np.deg2rad(30.0)))), atol=1e-5)
    assert torch.allclose((R @ c[:, :, None])[:, :2, 0], torch.zeros(8, 2), atol=1e-5)  # the origin projects to the centre
    az = torch.atan2(c[:, 1], c[:, 0]) % (2 * np.pi)
    assert torch.allclose(az, 2 * np.pi * torch.arange(8) / 8, atol=1e-5)
    assert torch.equal(syn.make_cameras(cfg), syn.make_cameras(cfg))
