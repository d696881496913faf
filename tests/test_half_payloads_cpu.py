"""fp16 / bf16 fields as render payloads, and half outputs, without a GPU: the six new entry points exist in every layer and refuse
bad arguments before any HIP call (fake pointers, never dereferenced: every call below returns from the C ABI layer's checks)."""
import ctypes as C
import os
import re

import pytest

import gsbp_amd
from gsbp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 2
NEW = ("gwbp_render_typed", "gwbp_render_pixels_typed", "gwbp_probe_pixels_typed", "gwbp_field_compare_typed",
       "gwbp_neighbor_mean_out_typed", "gwbp_neighbor_blend_out_typed")


def test_the_six_entry_points_exist_in_every_layer():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gwbp.h")).read(), flags=re.S)
    declared = set(re.findall(r"GWBP_API int (gwbp_[a-z0-9_]+)\(", header))
    capi = open(os.path.join(_lib.CSRC, "capi.hip")).read()
    gsbp_amd.build()
    for name in NEW:
        assert name in declared, name
        assert re.search(r"^int %s\(" % name, capi, flags=re.M), name
        assert name in _lib.EXPORTS and name in _lib.FIELD_ARGTYPES, name
        fn = getattr(_lib.lib(), name)  # resolves in the built library, with its argument types set
        assert fn is not None and list(fn.argtypes) == _lib.FIELD_ARGTYPES[name]
    # the untyped functions and the fp32-output typed ones are calls of the new ones: their bodies hold no check of their own
    for old, new in (("gwbp_render", "gwbp_render_typed"), ("gwbp_render_pixels", "gwbp_render_pixels_typed"),
                     ("gwbp_probe_pixels", "gwbp_probe_pixels_typed"), ("gwbp_field_compare", "gwbp_field_compare_typed"),
                     ("gwbp_neighbor_mean_typed", "gwbp_neighbor_mean_out_typed"),
                     ("gwbp_neighbor_blend_typed", "gwbp_neighbor_blend_out_typed")):
        body = re.search(r"^int %s\(.*?^\{(.*?)^\}" % old, capi, flags=re.M | re.S).group(1)
        assert body.strip().startswith("return %s(" % new) and "GWBP_MAP_F32" in body and body.count(";") == 1, old


# ---- argument validation ---------------------------------------------------------------------------------------------------------------
P = [1 << s for s in range(12, 24)]  # fake, 4-KiB aligned, never dereferenced
CAPS = _lib.Caps(40, 1 << 16, 1 << 20, 64, 64)
VIEW = _lib.View()
VIEW.width, VIEW.height = 64, 64
VIEW.K[0] = VIEW.K[4] = 50.0


def _err():
    return _lib.lib().gwbp_last_error_string().decode()


def _ws():
    n = C.c_size_t(0)
    assert _lib.lib().gwbp_workspace_size(C.byref(CAPS), C.byref(n)) == 0
    return C.byref(CAPS), P[11], n, C.byref(VIEW)  # (P[11]: 256-B aligned, as a workspace must be)


# every call below: (X = the payload pointer, t = its type code, ld = its row stride) first, then the function's other arguments
def _render(X=P[0], t=F16, ld=16, D=16, out=P[1], ot=F32):
    return _lib.lib().gwbp_render_typed(*_ws(), X, t, ld, D, out, ot, None)


def _pixels(X=P[0], t=F16, ld=16, D=16, out=P[1], alphas=P[2]):
    return _lib.lib().gwbp_render_pixels_typed(*_ws(), X, t, ld, D, out, alphas, None)


def _probe(X=P[0], t=F16, ld=16, M=3, xy=P[1], D=16, out=P[2], depth=P[3], alpha=P[4]):
    return _lib.lib().gwbp_probe_pixels_typed(*_ws(), M, xy, X, t, ld, D, out, depth, alpha, None)


def _compare(X=P[0], t=F16, ld=16, D=16, fmap=P[1], mt=F32, ms_y=64 * 16, ms_x=16, lr_h=0, lr_w=0, ymap=None, xmap=None, planes=P[2],
             table=P[3]):
    return _lib.lib().gwbp_field_compare_typed(*_ws(), X, t, ld, D, fmap, mt, ms_y, ms_x, lr_h, lr_w, ymap, xmap, planes, table, None)


def _mean(X=P[0], t=F16, ld=16, n=40, m=40, D=16, k=4, idx=P[1], out=P[2], ot=F16, ldo=16):
    return _lib.lib().gwbp_neighbor_mean_out_typed(n, m, D, k, idx, X, t, ld, out, ot, ldo, None)


def _blend(X=P[0], t=F16, ld=16, q=40, m=40, D=16, k=4, idx=P[1], w=P[2], out=P[3], ot=F16, ldo=16, wsum=P[4]):
    return _lib.lib().gwbp_neighbor_blend_out_typed(q, m, D, k, idx, w, X, t, ld, out, ot, ldo, wsum, None)


# the untyped functions' own invalid cases, through the typed entry point
OWN = {
    _render: [dict(X=None), dict(out=None), dict(D=0)],
    _pixels: [dict(X=None), dict(out=None), dict(D=0), dict(D=33, ld=64)],
    _probe: [dict(M=0), dict(M=4097), dict(D=0), dict(D=2049, ld=4096), dict(X=None), dict(xy=None), dict(xy=P[1] + 2), dict(out=None),
             dict(out=P[2] + 2), dict(depth=P[3] + 2), dict(alpha=P[4] + 1)],
    _compare: [dict(mt=5), dict(D=0), dict(D=2049, ld=4096), dict(X=None), dict(fmap=None), dict(fmap=P[1] + 2), dict(mt=F16, fmap=P[1] + 1),
               dict(ms_y=-1), dict(ms_x=-1), dict(ymap=P[4]), dict(xmap=P[5]), dict(ymap=P[4], xmap=P[5]),
               dict(ymap=P[4] + 2, xmap=P[5], lr_h=4, lr_w=4), dict(planes=P[2] + 2), dict(table=None), dict(table=P[3] + 4)],
    _mean: [dict(n=-1), dict(m=0), dict(D=0), dict(k=0), dict(k=33), dict(ldo=15), dict(X=None), dict(idx=None), dict(out=None)],
    _blend: [dict(q=-1), dict(m=0), dict(k=0), dict(k=33), dict(idx=None), dict(w=P[2] + 1), dict(D=0), dict(ldo=15), dict(X=None),
             dict(out=None), dict(wsum=P[4] + 2), dict(wsum=P[3])],
}
HAS_OUT_TYPE = (_render, _mean, _blend)


@pytest.mark.parametrize("call", list(OWN), ids=lambda f: f.__name__.strip("_"))
def test_entry_points_refuse_bad_arguments_before_any_hip_call(call):
    gsbp_amd.build()
    # an unknown type code, checked before anything else: even with every other argument bad
    for t in (-1, 3, 7):
        assert call(t=t) == -1 and "type" in _err(), (t, _err())
    assert call(t=9, X=None, ld=-1, D=-3) == -1 and "unknown" in _err(), _err()
    if call in HAS_OUT_TYPE:
        for ot in (-1, 3):
            assert call(ot=ot) == -1 and "type" in _err(), (ot, _err())
        assert call(ot=9, X=None, ld=-1, out=None) == -1 and "unknown" in _err(), _err()
    # a half element at an odd address; an fp32 element at a 2-B aligned one
    for t in (F16, BF16):
        assert call(t=t, X=P[0] + 1) == -1 and "aligned" in _err(), (t, _err())
    assert call(t=F32, X=P[0] + 2) == -1 and "aligned" in _err(), _err()
    if call in HAS_OUT_TYPE:
        out = P[3] if call is _blend else P[2] if call is _mean else P[1]
        for ot in (F16, BF16):
            assert call(ot=ot, out=out + 1) == -1 and "aligned" in _err(), (ot, _err())
        assert call(ot=F32, out=out + 2) == -1 and "aligned" in _err(), _err()
    for t in (F32, F16, BF16):  # a row stride, in elements, below D
        assert call(t=t, ld=15) == -1 and "stride" in _err(), (t, _err())
    for t in (F32, F16, BF16):
        for kw in OWN[call]:
            assert call(t=t, **kw) == -1, (t, kw)
            assert _err(), kw


@pytest.mark.parametrize("call", HAS_OUT_TYPE, ids=lambda f: f.__name__.strip("_"))
def test_a_half_out_that_aliases_the_payload_is_refused(call):
    gsbp_amd.build()
    for t in (F16, BF16):
        for ot in (F16, BF16):
            assert call(t=t, ot=ot, out=P[0]) == -1 and ("alias" in _err() or "must not be one of the input" in _err()), _err()


def test_the_caps_the_workspace_and_the_view_are_still_checked():
    """The four entry points that work on a view keep the untyped functions' order behind the type code: caps, workspace, view."""
    gsbp_amd.build()
    L = _lib.lib()
    caps, ws, n, view = _ws()
    assert L.gwbp_render_typed(None, ws, n, view, P[0], F16, 16, 16, P[1], F32, None) == -1 and "null caps" in _err()
    assert L.gwbp_render_pixels_typed(caps, None, n, view, P[0], F16, 16, 16, P[1], None, None) == -1 and "null workspace" in _err()
    assert L.gwbp_probe_pixels_typed(caps, ws, C.c_size_t(1024), view, 3, P[1], P[0], F16, 16, 16, P[2], None, None, None) == -2
    assert L.gwbp_field_compare_typed(caps, ws, n, None, P[0], F16, 16, 16, P[1], F32, 1024, 16, 0, 0, None, None, None, P[3],
                                      None) == -1 and "null view" in _err()
