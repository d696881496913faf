"""No-GPU checks of the per-pixel Gaussian lists: the numpy reference against the float64 matrix form, the entry point's own invalid
cases, the Python layer's argument errors, and its plain-torch helpers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib, pixels

import pixel_gaussians_ref as ref
import ref_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W0, H0 = 33, 20


def _small_scene(n=7, seed=5):
    rng = np.random.default_rng(seed)
    means = np.concatenate([rng.uniform(-0.45, 0.45, (n, 1)), rng.uniform(-0.25, 0.25, (n, 1)), rng.uniform(2.0, 4.0, (n, 1))], 1)
    quats = rng.normal(size=(n, 4))
    scales = rng.uniform(0.08, 0.35, (n, 3))
    opac = rng.uniform(0.3, 0.95, n)
    K = np.array([[30.0, 0, W0 / 2], [0, 30.0, H0 / 2], [0, 0, 1]])
    return means, quats, scales, opac, np.eye(4), K


def test_reference_lists_and_median_equal_the_float64_matrix_form():
    means, quats, scales, opac, vm, K = _small_scene()
    proj = ref_np.project(means, quats, scales, vm, K, W0, H0)
    Wm, amap = ref_np.weights(proj, opac, W0, H0)  # [P, n] float64, alpha [H, W]
    Wm = Wm.astype(np.float32)  # the triples a kernel would give are fp32
    pix, gid = np.nonzero(Wm)
    w = Wm[pix, gid]
    n, P = Wm.shape[1], W0 * H0
    assert (np.count_nonzero(Wm, axis=1) > 3).any() and (np.count_nonzero(Wm, axis=1) == 0).any()
    for k in (1, 3, 16):
        ids, weights, nc = ref.lists(gid, pix, w, P, k)
        for p in range(P):
            row = sorted(((-float(Wm[p, g]), g) for g in range(n) if Wm[p, g] > 0))
            assert nc[p] == len(row)
            want_ids = [g for _, g in row[:k]] + [-1] * (k - min(k, len(row)))
            want_w = [-x for x, _ in row[:k]] + [0.0] * (k - min(k, len(row)))
            assert ids[p].tolist() == want_ids and weights[p].tolist() == want_w
    # the median: the tile lists as a front stage would sort them (depth, then index), the chain walked pixel by pixel
    order = sorted(np.nonzero(proj["ok"])[0], key=lambda i: (np.float32(proj["z"][i]), i))
    tw, th = -(-W0 // 16), -(-H0 // 16)
    flat, offs = [], [0]
    for t in range(tw * th):
        tx, ty = t % tw, t // tw
        flat += [i for i in order if proj["rect"][i][0] <= tx < proj["rect"][i][2] and proj["rect"][i][1] <= ty < proj["rect"][i][3]]
        offs.append(len(flat))
    bins = dict(tile_offsets=np.array(offs, np.int32), flatten_ids=np.array(flat, np.int32), tile_w=tw, tile_h=th)
    med, decided, T_last = ref.median(gid, pix, w, bins, n, W0, H0)
    assert (med >= 0).any() and (med < 0).any()
    for p in range(P):
        T, want = 1.0, -1
        for g in order:
            if Wm[p, g] > 0:
                T -= float(Wm[p, g])
                if want < 0 and T <= 0.5:
                    want = g
        assert med[p] == want
        assert abs(T_last[p] - T) < 1e-12 and abs((1.0 - T) - amap.reshape(-1)[p]) < 1e-6


def test_reference_orders_equal_weights_by_id_and_flags_the_band():
    gid = np.array([5, 2, 9, 2], np.int32)
    pix = np.array([0, 0, 0, 1], np.int32)
    w = np.array([0.25, 0.25, 0.5, 0.5 - 1e-6], np.float32)
    ids, weights, nc = ref.lists(gid, pix, w, 3, 2)
    assert ids.tolist() == [[9, 2], [2, -1], [-1, -1]] and nc.tolist() == [3, 1, 0]
    assert weights.tolist() == [[0.5, 0.25], [w[3], 0.0], [0.0, 0.0]]
    bins = dict(tile_offsets=np.array([0, 3], np.int32), flatten_ids=np.array([5, 2, 9], np.int32), tile_w=1, tile_h=1)
    med, decided, _ = ref.median(gid, pix, w, bins, 10, 3, 1)
    # pixel 0: T = 0.75, 0.5 (on the band), 0.0; pixel 1: T = 0.5 + 1e-6 (inside the band); pixel 2: nothing
    assert med.tolist() == [2, -1, -1] and decided.tolist() == [False, False, True]


def _call(**over):
    """gwbp_pixel_gaussians with null caps and valid own arguments but `over`; the pointers are never dereferenced."""
    L = _lib.lib()
    buf = (C.c_char * 512)()
    fake = (C.addressof(buf) + 255) & ~255
    view = _lib.View()
    a = dict(k=4, M=4, xy=fake, ids=fake, weights=fake, n_contrib=fake, alpha=fake, median_id=fake, median_depth=fake)
    a.update(over)
    rc = L.gwbp_pixel_gaussians(None, C.c_void_p(fake), C.c_size_t(1 << 20), C.byref(view), a["k"], a["M"],
                                *(C.c_void_p(a[n]) if a[n] else None
                                  for n in ("xy", "ids", "weights", "n_contrib", "alpha", "median_id", "median_depth")), None)
    return rc, L.gwbp_last_error_string()


def test_entry_point_refuses_its_own_invalid_arguments_before_the_caps():
    gsbp_amd.build()
    assert "gwbp_pixel_gaussians" in _lib.ARGTYPES
    rc, msg = _call()
    assert rc == -1 and b"null caps" in msg  # its own arguments pass: the caps are looked at next
    assert _call(xy=None, M=0)[1].find(b"null caps") >= 0  # the image form ignores M
    assert _call(xy=None, M=1 << 20)[1].find(b"null caps") >= 0
    for optional in ("n_contrib", "alpha", "median_id", "median_depth"):
        assert b"null caps" in _call(**{optional: None})[1]
    for over, text in ((dict(k=0), b"k must be in [1, 16]"), (dict(k=17), b"k must be in [1, 16]"), (dict(k=-1), b"k must be"),
                       (dict(M=0), b"M must be in [1, 4096]"), (dict(M=4097), b"M must be in [1, 4096]"),
                       (dict(ids=None), b"ids and weights"), (dict(weights=None), b"ids and weights")):
        rc, msg = _call(**over)
        assert rc == -1 and b"pixel_gaussians" in msg and text in msg, (over, msg)
    buf = (C.c_char * 512)()
    odd = ((C.addressof(buf) + 255) & ~255) + 2
    for name, text in (("xy", b"xy must be 4-B aligned"), ("ids", b"ids and weights"), ("weights", b"ids and weights"),
                       ("n_contrib", b"must be 4-B aligned"), ("alpha", b"must be 4-B aligned"), ("median_id", b"must be 4-B aligned"),
                       ("median_depth", b"must be 4-B aligned")):
        rc, msg = _call(**{name: odd})
        assert rc == -1 and b"pixel_gaussians" in msg and text in msg, (name, msg)


def test_python_functions_refuse_cpu_tensors_and_bad_arguments():
    z3, z4, z1 = torch.zeros(4, 3), torch.zeros(4, 4), torch.zeros(4)
    scene = (z3, z4, z3, z1, torch.eye(4), torch.eye(3), 64, 64)
    for fn in (gsbp_amd.pixel_gaussians, gsbp_amd.render_id_map, gsbp_amd.median_depth):
        with pytest.raises(gsbp_amd.GwbpError, match="HIP tensors"):
            fn(*scene)
    with pytest.raises(gsbp_amd.GwbpError, match="HIP tensors"):
        gsbp_amd.pick_gaussians(*scene, xy=[[1, 2]])
    for k in (0, 17, 2.0, True, None):
        with pytest.raises(gsbp_amd.GwbpError, match="k must be"):
            gsbp_amd.pixel_gaussians(*scene, k=k)
    for xy in ([[0.5, 1.0]], [[1, 2, 3]], [], torch.zeros(4097, 2, dtype=torch.int32), [1, 2, 3]):
        with pytest.raises(gsbp_amd.GwbpError, match="xy must be|number of pixels"):
            gsbp_amd.pixel_gaussians(*scene, xy=xy)
    with pytest.raises(gsbp_amd.GwbpError, match="needs xy"):
        gsbp_amd.pick_gaussians(*scene, xy=None)


def test_lookup_keeps_the_table_type_and_fills_the_empty_pixels():
    id_map = torch.tensor([[0, 2, -1], [1, -1, 2]], dtype=torch.int32)
    labels = torch.tensor([7, 8, 9], dtype=torch.int64)
    assert pixels.lookup(id_map, labels, fill=-1).tolist() == [[7, 9, -1], [8, -1, 9]]
    colours = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], dtype=torch.float16)
    out = pixels.lookup(id_map, colours, fill=0.5)
    assert out.dtype == torch.float16 and out.shape == (2, 3, 3)
    assert out[0, 1].tolist() == [0, 0, 1.0] and out[0, 2].tolist() == [0.5, 0.5, 0.5]
    assert pixels.lookup(id_map, colours.bfloat16()).dtype == torch.bfloat16
    with pytest.raises(gsbp_amd.GwbpError):
        pixels.lookup(id_map.float(), labels)


def test_dominance_counts_and_the_order_of_picked_ids():
    ids = torch.tensor([[[3, 1], [3, -1]], [[-1, -1], [0, 3]]], dtype=torch.int32)
    weights = torch.tensor([[[0.5, 0.2], [0.9, 0.0]], [[0.0, 0.0], [0.2, 0.1]]])
    z = torch.zeros(2, 2)
    pg = pixels.PixelGaussians(ids, weights, z.int(), z, None, None)
    assert pixels.dominance_counts(pg, 5).tolist() == [1, 0, 0, 2, 0]
    assert pixels.dominance_counts(ids[..., 0], 4).tolist() == [1, 0, 0, 2]
    with pytest.raises(gsbp_amd.GwbpError):
        pixels.dominance_counts(pg, 3)
    # distinct ids by their largest weight; 0 and 1 tie at 0.2 and go by id; the weight 0 of an empty slot never counts
    assert pixels.ranked_ids(ids, weights).tolist() == [3, 0, 1]
    assert pixels.ranked_ids(ids, weights, min_weight=0.2).tolist() == [3]
    assert pixels.ranked_ids(ids[1, :1], weights[1, :1]).tolist() == []


def test_run_pick_parses_its_documented_options():
    sys.path.insert(0, ROOT)
    import run_pick
    ap = run_pick.build_parser()
    a = ap.parse_args(["--synthetic", "C1", "--click", "0:200,150", "--click", "2:7,9", "--k", "8", "--components", "--radius-factor",
                       "1.5", "--id-maps", "--median-depth", "--out", "x"])
    assert a.click == [(0, 200, 150), (2, 7, 9)] and a.k == 8 and a.components and a.radius_factor == 1.5 and a.radius is None
    assert a.id_maps and a.median_depth and a.out == "x" and a.synthetic == "C1"
    a = ap.parse_args(["--click", "1:-1,0", "--radius", "0.05", "--out", "y"])
    assert a.click == [(1, -1, 0)] and a.radius == 0.05 and a.k == 4 and not a.components
    for bad in (["--click", "0:1"], ["--click", "a:1,2"], ["--radius", "1", "--radius-factor", "2", "--out", "z"], ["--click", "0:1,2"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
