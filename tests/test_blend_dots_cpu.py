"""No-GPU checks of the dots form of the blend backward (csrc/render_grad_wide.hip, gwbp_render_dots_backward).

    (a) the identity the kernel rests on: with m_j = <c_j, vo_p> and ONE scalar B per pixel, v_g2d equals the differentiated blend of
        tests/blend_grad_ref.py in float64 to 1e-12 relative, at D = 1, 33 and 128, on the CPU oracle's lists and cut
    (b) the comparison has teeth: B dropped, alpha_k in place of fac_k, the v_alpha term dropped -- each is off by orders of magnitude
    (c) the entry point is declared, bound and exported, and every argument check answers before any HIP call
"""
import ctypes as C
import functools
import os
import re

import pytest
import torch

import blend_dots_ref as bd
import blend_grad_ref as bg
import raster_grad_ref as rg
from gsbp_amd import _lib
from test_gpu_raster_grad import _stack, _t0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (1, 33, 128)


@functools.lru_cache(maxsize=None)
def _case(name, D, orc):
    """The oracle's front and cut of the scene, a seeded table, v_out and v_alpha, and the float64 truth; computed once, never modified."""
    sc = _t0() if name == "t0" else _stack(0.1, n=80)
    f = bg.oracle_front(orc, *sc["inputs"][:4], sc["vm"], sc["K"], sc["W"], sc["H"])
    g = torch.Generator().manual_seed(53 + D)
    colors = torch.rand(sc["inputs"][0].shape[0], D, generator=g)
    v_out = torch.randn(sc["H"], sc["W"], D, generator=g)
    v_alpha = torch.randn(sc["H"], sc["W"], generator=g)
    args = (f["means2d"], f["conics"], f["opacities"], colors, v_out, v_alpha)
    return dict(front=f, args=args, truth=bg.blend(torch.float64, f["plan"], *args)["v_g2d"])


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", ["t0", "stack80"])
def test_dots_form_equals_the_differentiated_blend_in_float64(orc, name, D):
    c = _case(name, D, orc)
    got = bd.v_g2d_dots(torch.float64, c["front"]["plan"], *c["args"])
    assert float(c["truth"].abs().max()) > 0
    for k, col in enumerate(bg.COLUMNS):
        fro, top = rg.errors(got[:, k], c["truth"][:, k])
        print(f"{name} D={D} {col}: dots form against autograd: {fro:.2e} (Frobenius), {top:.2e} (max)")
        assert fro <= 1e-12 and top <= 1e-12, (name, D, col)


@pytest.mark.parametrize("D", DIMS)
def test_without_v_alpha_it_is_v_alpha_zero(orc, D):
    c = _case("t0", D, orc)
    truth = bg.blend(torch.float64, c["front"]["plan"], *c["args"][:5], None)["v_g2d"]
    got = bd.v_g2d_dots(torch.float64, c["front"]["plan"], *c["args"][:5], None)
    assert max(rg.errors(got, truth)) <= 1e-12


@pytest.mark.parametrize("mutant", ["no-B", "alpha-for-fac", "no-va"])
@pytest.mark.parametrize("D", DIMS)
def test_mutants_of_the_dots_form_are_off_by_orders_of_magnitude(orc, mutant, D):
    """Against a bound of 1e-12 the mutants miss every column by more than 1e-3: nine orders of magnitude."""
    c = _case("t0", D, orc)
    got = bd.v_g2d_dots(torch.float64, c["front"]["plan"], *c["args"], mutant=mutant)
    for k, col in enumerate(bg.COLUMNS):
        fro, _ = rg.errors(got[:, k], c["truth"][:, k])
        print(f"{mutant} D={D} {col}: {fro:.2e}")
        assert fro > 1e-3, (mutant, D, col)


def test_the_entry_point_is_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gwbp.h")).read(), flags=re.S)
    assert re.search(r"GWBP_API int gwbp_render_dots_backward\(", hdr)
    assert "gwbp_render_dots_backward" in _lib.ARGTYPES and "gwbp_render_dots_backward" in _lib.EXPORTS
    mp = open(os.path.join(_lib.CSRC, "gwbp.map")).read()
    assert re.search(r"global:\s*gwbp_\*;", mp) and "gwbp_render_dots_backward" in mp
    assert _lib.lib().gwbp_render_dots_backward.argtypes == _lib.ARGTYPES["gwbp_render_dots_backward"]
    import gsbp_amd
    assert callable(gsbp_amd.render_latents) and callable(gsbp_amd.Engine.render_dots_backward)


def test_render_dots_backward_refuses_bad_arguments_before_any_device_call():
    """D = 0, D = 129, ldc < D, a null v_out, v_g2d or table and misaligned pointers: GWBP_EINVAL with a message.  Every pointer is a fake
    aligned host address and the workspace is never touched: these calls return before any HIP call (this test runs without a GPU)."""
    L = _lib.lib()
    caps = _lib.Caps(10, 1 << 16, 1 << 20, 64, 64)
    nbytes = C.c_size_t(0)
    assert L.gwbp_workspace_size(C.byref(caps), C.byref(nbytes)) == 0
    view = _lib.View()
    view.width, view.height = 64, 64
    view.K[0] = view.K[4] = 50.0
    buf = (C.c_char * 512)()
    fake = C.c_void_p((C.addressof(buf) + 255) & ~255)
    odd = C.c_void_p(fake.value + 2)

    def call(colors=fake, ldc=128, D=128, v_out=fake, v_alpha=fake, v_g2d=fake, w=64):
        view.width = w
        rc_ = L.gwbp_render_dots_backward(C.byref(caps), fake, nbytes, C.byref(view), colors, C.c_int64(ldc), D, v_out, v_alpha, v_g2d, None)
        return rc_, L.gwbp_last_error_string()

    for kw, msg in ((dict(D=0, ldc=0), b"1 <= D <= 128 (got D=0)"), (dict(D=129, ldc=129), b"1 <= D <= 128 (got D=129)"),
                    (dict(D=65, ldc=64), b"row stride 64 below D = 65"), (dict(v_out=None), b"null v_out"),
                    (dict(v_g2d=None), b"null v_g2d"), (dict(colors=None), b"null colors"), (dict(v_alpha=odd), b"4-B aligned"),
                    (dict(v_g2d=odd), b"4-B aligned"), (dict(colors=odd), b"4-B aligned")):
        rc_, err = call(**kw)
        assert rc_ == -1 and msg in err and b"render_dots_backward" in err, (kw, rc_, err)
    rc_, err = call(w=65)  # the view against the caps
    assert rc_ != 0 and err, (rc_, err)
