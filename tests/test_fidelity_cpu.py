"""No-GPU checks of gsbp_amd.fidelity: field_fidelity and agreement_weights on hand-made tables and planes, the argument errors of
the Python layer, the numpy reference on a hand-made pixel, and the C ABI's declaration of the entry point."""
import math
import os
import re

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib, fidelity

import fidelity_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def test_field_fidelity_per_view_and_overall():
    #                 sum cos  l1   l2    mm   valid bad pixels D
    t = torch.tensor([[3.0, 4.0, 8.0, 16.0, 4.0, 1.0, 10.0, 2.0],
                      [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 10.0, 2.0],     # a view that sees nothing
                      [1.0, 6.0, 2.0, 4.0, 2.0, 0.0, 10.0, 2.0]], dtype=torch.float64)
    rep = gsbp_amd.field_fidelity(t)
    pv = rep["per_view"]
    assert pv["cosine"].dtype == torch.float64 and pv["cosine"].shape == (3,)
    assert pv["cosine"].tolist()[::2] == [0.75, 0.5] and math.isnan(pv["cosine"][1])
    assert pv["mae"].tolist()[::2] == [0.5, 1.5] and pv["mse"].tolist()[::2] == [1.0, 0.5] and pv["relative"].tolist()[::2] == [0.5, 0.5]
    assert all(math.isnan(pv[k][1]) for k in pv)
    assert rep["overall"] == dict(cosine=4.0 / 6.0, mae=10.0 / 12.0, mse=10.0 / 12.0, relative=0.5)
    assert rep["n_valid"].tolist() == [4, 0, 2] and rep["n_bad"].tolist() == [1, 0, 0] and rep["views_scored"] == 2
    # the empty view alone, and one view's row
    only = gsbp_amd.field_fidelity(t[1])
    assert only["views_scored"] == 0 and all(math.isnan(x) for x in only["overall"].values())
    assert gsbp_amd.field_fidelity(t[0])["overall"]["cosine"] == 0.75
    with pytest.raises(gsbp_amd.GwbpError, match=r"\[V, 8\]"):
        gsbp_amd.field_fidelity(torch.zeros(3, 7))


def test_agreement_weights_criteria_nan_dtype_and_shape():
    cos = torch.tensor([[0.9, NAN, 0.5], [0.2, 0.6, -0.3]])
    w = gsbp_amd.agreement_weights(dict(cosine=cos), cosine_min=0.5)
    assert w.dtype == torch.bool and w.shape == (2, 3) and w.tolist() == [[True, False, True], [False, True, False]]
    assert gsbp_amd.agreement_weights(cos, cosine_min=0.5).tolist() == w.tolist()       # the bare plane
    # the lowest 40 % of the five finite cosines go: -0.3 and 0.2
    q = gsbp_amd.agreement_weights(cos, quantile=0.4)
    assert q.dtype == torch.bool and q.tolist() == [[True, False, True], [False, True, False]]
    assert gsbp_amd.agreement_weights(cos, quantile=0.0).tolist() == [[True, False, True], [True, True, True]]
    assert not bool(gsbp_amd.agreement_weights(torch.full((2, 2), NAN), quantile=0.5).any())
    for kw in (dict(), dict(cosine_min=0.5, quantile=0.5)):
        with pytest.raises(gsbp_amd.GwbpError, match="exactly one"):
            gsbp_amd.agreement_weights(cos, **kw)
    with pytest.raises(gsbp_amd.GwbpError, match="quantile"):
        gsbp_amd.agreement_weights(cos, quantile=1.0)
    with pytest.raises(gsbp_amd.GwbpError, match="cosine plane"):
        gsbp_amd.agreement_weights(torch.zeros(3), cosine_min=0.1)
    # what create_feature_field's pixel_weight_fn may return
    from gsbp_amd.engine import PIXEL_WEIGHT_TYPES
    assert w.dtype in PIXEL_WEIGHT_TYPES


def test_argument_errors_of_the_python_layer():
    z3, z4, z1 = torch.zeros(5, 3), torch.zeros(5, 4), torch.zeros(5)
    feats, fmap = torch.zeros(5, 8), torch.zeros(4, 6, 8)
    vm, K = torch.eye(4), torch.eye(3)
    for fn, args in ((gsbp_amd.render_field_agreement, (feats, fmap, vm, K, 6, 4)),
                     (gsbp_amd.score_field_views, (feats, vm[None], K, 6, 4, lambda v: fmap))):
        with pytest.raises(gsbp_amd.GwbpError, match="Pass the upsampled"):   # bilinear maps: the error says what to do
            fn(z3, z4, z3, z1, *args, upsample="bilinear")
        with pytest.raises(gsbp_amd.GwbpError, match="None or 'nearest'"):
            fn(z3, z4, z3, z1, *args, upsample="bicubic")
        with pytest.raises(gsbp_amd.GwbpError, match="HIP tensors"):        # no CPU path
            fn(z3, z4, z3, z1, *args)
    assert fidelity.PLANES == ("dot", "rr", "mm", "l1", "l2", "cosine") and len(fidelity.TABLE_COLUMNS) == 8


def test_the_numpy_reference_on_hand_made_pixels():
    r = np.zeros((ref.H * ref.W, 2))
    m = np.zeros((ref.H, ref.W, 2))
    r[0], m[0, 0] = (3.0, 4.0), (4.0, 3.0)
    r[1], m[0, 1] = (1.0, 0.0), (NAN, 0.0)
    r[2], m[0, 2] = (0.0, 0.0), (0.0, 2.0)
    p, scale = ref.planes_of(r, m)
    assert [p[k][0, 0] for k in ref.NAMES] == [24.0, 25.0, 25.0, 2.0, 2.0] and p["cosine"][0, 0] == 24.0 / 25.0
    assert all(np.isnan(p[k][0, 1]) for k in ref.NAMES + ("cosine",)) and p["bad"][0, 1] and not p["valid"][0, 1]
    assert p["rr"][0, 2] == 0 and p["l2"][0, 2] == p["mm"][0, 2] == 4.0 and np.isnan(p["cosine"][0, 2]) and not p["valid"][0, 2]
    assert scale["dot"][0, 0] == 24.0
    assert ref.table_of(p, 2).tolist() == [0.96, 2.0, 2.0, 25.0, 1.0, 1.0, float(ref.H * ref.W), 2.0]


def test_header_map_and_binding_name_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "gwbp.h")).read()
    assert re.search(r"GWBP_API int gwbp_field_compare\(", hdr) and "GWBP_FIELD_COMPARE_MAX_TILES" in hdr
    assert "gwbp_field_compare" in open(os.path.join(_lib.CSRC, "gwbp.map")).read()
    assert "gwbp_field_compare" in _lib.ARGTYPES and "field_compare.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    gsbp_amd.build()
    assert getattr(_lib.lib(), "gwbp_field_compare") is not None


def test_own_arguments_are_refused_before_any_device_call():
    """Behind valid caps, workspace and view: each kind of argument of gwbp_field_compare, GWBP_EINVAL with its own message."""
    import ctypes as C
    L = _lib.lib()
    caps = _lib.Caps(10, 1 << 16, 1 << 20, 64, 64)
    nbytes = C.c_size_t(0)
    assert L.gwbp_workspace_size(C.byref(caps), C.byref(nbytes)) == 0
    view = _lib.View()
    view.width, view.height = 64, 64
    view.K[0] = view.K[4] = 50.0
    buf = (C.c_char * 1024)()
    fake = (C.addressof(buf) + 255) & ~255
    good = dict(features=fake, ldf=8, D=8, map=fake, map_type=_lib.MAP_F32, ms_y=512, ms_x=8, lr_h=0, lr_w=0, ymap=None, xmap=None,
                planes=fake, table=fake)
    for kw, msg in ((dict(map_type=7), b"unknown map type"), (dict(D=0), b"D must be in"), (dict(D=2049, ldf=4096), b"D must be in"),
                    (dict(ldf=4), b"row stride"), (dict(features=None), b"features"), (dict(features=fake + 2), b"features"),
                    (dict(map=None), b"map must be"), (dict(map=fake + 2), b"map must be"),
                    (dict(map=fake + 1, map_type=_lib.MAP_F16), b"map must be"), (dict(ms_y=-1), b"negative map strides"),
                    (dict(ymap=fake), b"both index maps or neither"), (dict(ymap=fake, xmap=fake), b"low-resolution map's shape"),
                    (dict(ymap=fake + 2, xmap=fake, lr_h=4, lr_w=4), b"4-B aligned"), (dict(planes=fake + 2), b"planes"),
                    (dict(table=None), b"table"), (dict(table=fake + 4), b"table")):
        a = dict(good, **kw)
        rc = L.gwbp_field_compare(C.byref(caps), C.c_void_p(fake), nbytes, C.byref(view), a["features"], a["ldf"], a["D"], a["map"],
                                  a["map_type"], a["ms_y"], a["ms_x"], a["lr_h"], a["lr_w"], a["ymap"], a["xmap"], a["planes"],
                                  a["table"], None)
        assert rc == -1 and msg in L.gwbp_last_error_string(), (kw, rc, L.gwbp_last_error_string())
