"""No-GPU checks behind the geometry gradients of rasterization(): the torch restatements of the projection and SH kernels against
the CPU checker and the float64 camera reference, the gradient yardstick against finite differences of its own loss, and the argument
checks of gwbp_render_pixels_backward."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import raster_grad_ref as rg
import ref_camera_np as rc
from gsbp_amd import _lib
from gsbp_amd.projection import project_torch, sh_colors_torch
from util import scene_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23


def _t0(view=0):
    cfg, sc = scene_np("T0")
    return cfg, sc, sc["vms"][view], sc["K"]


def _ulps(got, ref):
    """Largest |got - ref| of a [n, k] table in float32 ulps of each ROW's largest reference magnitude (a conic's three numbers, a
    mean's two, share one scale: the off-diagonal of a nearly axis-aligned conic is as exact as its diagonal, not as itself)."""
    got, ref = np.asarray(got, np.float64).reshape(len(ref), -1), np.asarray(ref, np.float64).reshape(len(ref), -1)
    scale = np.abs(ref).max(axis=1, keepdims=True)
    return float((np.abs(got - ref) / (scale * ULP)).max())


# Bounds in float32 ulps of the row's scale: what the float32 restatement showed on T0, view 0, against the checker's float32
# projection (pinhole) and the float64 reference (ortho, fisheye) -- the observed figure beside each bound -- times about 2.5.
# project_torch orders its float32 operations differently from the kernel (matrix products instead of fma chains), so a few ulps per
# stage, amplified by the 2 x 2 inverse (1 / det cancels for a thin 2-D covariance), is what "agrees to float32 rounding" means here;
# a wrong term is off by 1e5 ulps or more, and the float64 run of the same code has to meet a thousandth of each bound.
MEANS2D_ULPS = 8.0    # observed: pinhole 1.7, ortho 2.5, fisheye 3.4
CONICS_ULPS = 64.0    # observed: pinhole 24.4, ortho 10.9, fisheye 14.3
OPACITY_ULPS = 24.0   # observed (antialiased: the ratio of two determinants): pinhole 9.5, ortho 3.1, fisheye 5.4; classic: exact


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_project_torch_pinhole_against_the_checker(orc, mode):
    """means2d and conics of the visible rows against the CPU checker's float32 projection (the kernel's bits), the effective opacity
    against the float64 camera reference (the checker knows no antialiasing)."""
    cfg, sc, vm, K = _t0()
    want = orc.project(sc["means"].numpy(), sc["quats"].numpy(), sc["scales"].numpy(), vm.numpy(), K.numpy(), cfg.width, cfg.height)
    vis = want["radii"] > 0
    assert vis.sum() > 300
    ref = rc.project(sc["means"].numpy(), sc["quats"].numpy(), sc["scales"].numpy(), sc["opac"].numpy(), vm.numpy(), K.numpy(),
                     cfg.width, cfg.height, "pinhole", antialiased=mode == "antialiased")
    assert np.array_equal(ref["ok"], vis)
    m2d, con, oe = project_torch(sc["means"], sc["quats"], sc["scales"], sc["opac"], vm, K, cfg.width, cfg.height, 0.3, "pinhole",
                                 mode, torch.from_numpy(vis))
    figures = (_ulps(m2d.numpy()[vis], want["means2d"][vis]), _ulps(con.numpy()[vis], want["conics"][vis]),
               _ulps(oe.numpy()[vis, None], ref["opacities"][vis, None]))
    print(f"pinhole {mode}: means2d {figures[0]:.1f} conics {figures[1]:.1f} opacity {figures[2]:.1f} ulps")
    assert figures[0] <= MEANS2D_ULPS and figures[1] <= CONICS_ULPS and figures[2] <= OPACITY_ULPS
    if mode == "classic":
        assert torch.equal(oe[torch.from_numpy(vis)], sc["opac"][torch.from_numpy(vis)])
    # rows outside `visible` are zero
    hidden = torch.from_numpy(~vis)
    assert not m2d[hidden].any() and not con[hidden].any() and not oe[hidden].any()


@pytest.mark.parametrize("model", ["ortho", "fisheye"])
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_project_torch_ortho_and_fisheye_against_the_float64_reference(model, mode):
    """In float64 the restatement IS the reference's function (1e-9 relative); in float32 it agrees with it to float32 rounding."""
    cfg, sc, vm, K = _t0()
    K = K.clone()
    if model == "ortho":
        K[0, 0] = K[1, 1] = 0.4 * cfg.width
    ref = rc.project(sc["means"].numpy(), sc["quats"].numpy(), sc["scales"].numpy(), sc["opac"].numpy(), vm.numpy(), K.numpy(),
                     cfg.width, cfg.height, model, antialiased=mode == "antialiased")
    vis = ref["ok"]
    assert vis.sum() > 200
    for dtype, scale in ((torch.float64, 1e-3), (torch.float32, 1.0)):
        g = [sc[k].to(dtype) for k in ("means", "quats", "scales", "opac")]
        m2d, con, oe = project_torch(*g, vm, K, cfg.width, cfg.height, 0.3, model, mode, torch.from_numpy(vis))
        figures = (_ulps(m2d.numpy()[vis], ref["means2d"][vis]), _ulps(con.numpy()[vis], ref["conics"][vis]),
                   _ulps(oe.numpy()[vis, None], ref["opacities"][vis, None]))
        print(f"{model} {mode} {dtype}: means2d {figures[0]:.3g} conics {figures[1]:.3g} opacity {figures[2]:.3g} ulps")
        assert figures[0] <= scale * MEANS2D_ULPS and figures[1] <= scale * CONICS_ULPS and figures[2] <= scale * OPACITY_ULPS


def test_project_torch_clamped_rows_get_no_jacobian_gradient_from_the_ratio():
    """The pinhole clamp of x/z inside the Jacobian is torch.clamp: where it binds, the covariance no longer depends on x/z through
    that term -- d(conic) / d(mean_x) of a Gaussian far outside the frustum equals the value with the clamp's limit held fixed."""
    K = torch.tensor([[50.0, 0, 32], [0, 50.0, 32], [0, 0, 1]])
    vm = torch.eye(4)
    means = torch.tensor([[3.0, 0.1, 2.0]], dtype=torch.float64, requires_grad=True)  # x/z = 1.5, the limit is 0.64 + 0.3 * 0.64
    quats = torch.tensor([[1.0, 0.2, -0.1, 0.3]], dtype=torch.float64)
    scales = torch.tensor([[0.2, 0.1, 0.15]], dtype=torch.float64)
    _, con, _ = project_torch(means, quats, scales, torch.ones(1, dtype=torch.float64), vm, K, 64, 64)
    (g,) = torch.autograd.grad(con.sum(), means)
    h = 1e-6
    with torch.no_grad():
        plus = project_torch(means + torch.tensor([[h, 0, 0]]), quats, scales, torch.ones(1, dtype=torch.float64), vm, K, 64, 64)[1]
        minus = project_torch(means - torch.tensor([[h, 0, 0]]), quats, scales, torch.ones(1, dtype=torch.float64), vm, K, 64, 64)[1]
    assert float(g[0, 0]) == 0.0  # J02 = -fx lim / z: no x in it once the clamp binds, and J00 = fx / z has none either
    assert abs(float((plus - minus).sum()) / (2 * h)) < 1e-6


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_colors_torch_against_the_checker(orc, degree):
    cfg, sc, vm, _ = _t0()
    g = torch.Generator().manual_seed(5 + degree)
    coeffs = 0.5 * torch.randn(cfg.n_gaussians, 16, 3, generator=g)
    campos = (-(vm[:3, :3].T @ vm[:3, 3])).tolist()
    want = orc.sh_colors(degree, sc["means"].numpy(), coeffs.numpy(), np.asarray(campos, np.float32))
    got = sh_colors_torch(degree, sc["means"], coeffs, campos).numpy()
    assert (want == 0).any() or degree == 0  # (the clamp at 0 is exercised)
    # float32 sums of up to 16 terms of size <= 1 in another order: a few ulps of 1
    assert np.abs(got - want).max() <= 16 * ULP, np.abs(got - want).max()


def _tiny_scene():
    """6 Gaussians in front of an identity pinhole camera, 8 x 8 pixels, D = 3; opacities below 0.9 (nothing near the clamp)."""
    g = torch.Generator().manual_seed(11)
    n, W, H = 6, 8, 8
    means = torch.cat([0.5 * (torch.rand(n, 2, generator=g) - 0.5), 2.0 + torch.rand(n, 1, generator=g)], dim=1)
    quats = torch.randn(n, 4, generator=g)
    scales = 0.08 + 0.1 * torch.rand(n, 3, generator=g)
    opac = 0.3 + 0.55 * torch.rand(n, generator=g)
    colors = torch.rand(n, 3, generator=g)
    K = torch.tensor([[12.0, 0, 4], [0, 12.0, 4], [0, 0, 1]])
    G, A = torch.randn(H, W, 3, generator=g), torch.randn(H, W, generator=g)
    return (means, quats, scales, opac, colors), torch.eye(4), K, W, H, G, A


def _fixed_cut(inputs, vm, K, W, H, **kw):
    """A mask decided once, in float64, by the blend's own rule without termination (alpha >= 1/255), then held fixed."""
    n = inputs[0].shape[0]
    everything = dict(mask=torch.ones(W * H, n, dtype=torch.bool), visible=torch.ones(n, dtype=torch.bool),
                      order=torch.arange(n))
    ins = [t.double() for t in inputs]
    depths = (ins[0] @ vm.double()[:3, :3].T + vm.double()[:3, 3])[:, 2].float()
    everything["order"] = rg.depth_order(depths, everything["visible"])
    raw = rg.render(*ins, vm, K, W, H, everything, **kw)[2]
    inv = torch.argsort(everything["order"])
    return dict(everything, mask=(raw >= 1.0 / 255.0)[:, inv])


@pytest.mark.parametrize("kw", [dict(), dict(rasterize_mode="antialiased", render_mode="RGB+ED"),
                                dict(camera_model="fisheye", render_mode="RGB+D", background=torch.tensor([0.3, 0.1, 0.7, 0.2]))],
                         ids=["plain", "antialiased-ED", "fisheye-D-background"])
def test_the_yardstick_equals_finite_differences_of_its_own_loss(kw):
    """With the mask held fixed the loss is smooth: the autograd gradients of the float64 restatement equal central differences.  This
    keeps the thing every kernel gradient is measured against from being wrong."""
    inputs, vm, K, W, H, G, A = _tiny_scene()
    cut = _fixed_cut(inputs, vm, K, W, H, **{k: v for k, v in kw.items() if k in ("camera_model", "rasterize_mode")})
    assert 40 < int(cut["mask"].sum()) < W * H * 6  # (a real cut: some pairs in, some out)
    if "D" in kw.get("render_mode", "RGB"):
        G = torch.cat([G, G[..., :1]], dim=-1)
    grads, _, raw = rg.gradients(torch.float64, inputs, G, A, vm, K, W, H, cut, **kw)
    assert float(raw.max()) < 0.95

    def loss_at(k, delta):
        ins = [t.double().clone() for t in inputs]
        ins[k] = ins[k] + delta
        out, alpha, _ = rg.rasterize(*ins, vm, K, W, H, cut, **kw)
        return float((out * G.double()).sum() + (alpha * A.double()).sum())

    h = 1e-6
    for k, name in enumerate(rg.NAMES):
        fd = torch.zeros_like(grads[k])
        flat = fd.view(-1)
        for i in range(flat.numel()):
            d = torch.zeros_like(flat)
            d[i] = h
            flat[i] = (loss_at(k, d.view_as(fd)) - loss_at(k, -d.view_as(fd))) / (2 * h)
        fro, top = rg.errors(grads[k], fd)
        print(f"{name}: autograd against central differences: {fro:.2e} (Frobenius), {top:.2e} (max)")
        assert fro < 1e-6 and top < 1e-6, name  # (central differences at h = 1e-6 in float64: ~1e-9 truncation + 1e-10 rounding)


def test_the_entry_point_is_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gwbp.h")).read(), flags=re.S)
    assert re.search(r"GWBP_API int gwbp_render_pixels_backward\(", hdr)
    assert "gwbp_render_pixels_backward" in _lib.ARGTYPES and "gwbp_render_pixels_backward" in _lib.EXPORTS
    mp = open(os.path.join(_lib.CSRC, "gwbp.map")).read()
    assert re.search(r"global:\s*gwbp_\*;", mp) and "gwbp_render_pixels_backward" in mp
    assert _lib.lib().gwbp_render_pixels_backward.argtypes == _lib.ARGTYPES["gwbp_render_pixels_backward"]


def test_render_pixels_backward_refuses_bad_arguments_before_any_device_call():
    """D = 0, D = 33, a null v_out, a null v_g2d, a null table and ldc < D: GWBP_EINVAL with a message.  Every pointer is a fake aligned
    host address and the workspace is never touched: these calls return before any HIP call (this test runs without a GPU)."""
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

    def call(colors=fake, ldc=4, D=4, v_out=fake, v_alpha=fake, v_colors=fake, v_g2d=fake):
        rc_ = L.gwbp_render_pixels_backward(C.byref(caps), fake, nbytes, C.byref(view), colors, C.c_int64(ldc), D, v_out, v_alpha,
                                            v_colors, v_g2d, None)
        return rc_, L.gwbp_last_error_string()

    for kw, msg in ((dict(D=0, ldc=0), b"1 <= D <= 32"), (dict(D=33, ldc=33), b"1 <= D <= 32"), (dict(v_out=None), b"null v_out"),
                    (dict(v_g2d=None), b"null v_g2d"), (dict(colors=None), b"null colors"), (dict(D=4, ldc=3), b"row stride 3 below D = 4"),
                    (dict(v_alpha=odd), b"4-B aligned"), (dict(v_g2d=odd), b"4-B aligned")):
        rc_, err = call(**kw)
        assert rc_ == -1 and msg in err, (kw, rc_, err)
