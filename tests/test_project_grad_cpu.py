"""No-GPU checks behind the camera gradient: csrc/project_grad.h -- the per-Gaussian vjp k_project_bwd evaluates -- compiled for the
host (tests/project_grad_host.cpp) against torch's float64 autograd of project_torch; the yardstick's view-matrix gradient against
finite differences of its own loss; the registration and argument checks of gwbp_project_backward; se3_exp and pose_error.

Bound.  In float64 the hand-written chain IS project_torch's function: 1e-9 Frobenius-relative, the figure tests/test_raster_grad_cpu.py
uses for "in float64 the restatement is the function".  A float32 intermediate that slipped in shows about 1e-7, a wrong term 1e-3 or
more.  Measured here (printed by the test): 5e-17 .. 3e-15 over the three cameras, both modes and all five tensors, and 1.1e-13 for the
means and the view matrix of the classic fisheye case -- all below 1e-10.  Both sides get eps2d as gwbp_view stores it (the float32 0.3,
widened): with the double 0.3 on one side only, every figure sits at 2e-8.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import camera_grad_ref as cg
import raster_grad_ref as rg
import ref_camera_np as rc
from gsbp_amd import _lib
from gsbp_amd.pose import pose_error, se3_exp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-9
EPS2D = float(np.float32(0.3))  # the value gwbp_view stores, widened: what the vjp and the truth are both given
_D = C.POINTER(C.c_double)


@pytest.fixture(scope="session")
def host(tmp_path_factory):
    """tests/project_grad_host.cpp built with the system C++ compiler into a temporary directory and loaded through ctypes."""
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) found")
    so = str(tmp_path_factory.mktemp("project_grad") / "libproject_grad_host.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-o", so,
                           os.path.join(ROOT, "tests", "project_grad_host.cpp")])
    lib = C.CDLL(so)
    lib.project_grad_host.restype = C.c_int
    lib.project_grad_host.argtypes = ([C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 6
                                      + [_D] * 5)
    return lib


def run_host(lib, inputs, vm, K, W, H, model, mode, visible, v_g2d, eps2d=EPS2D):
    """The shim on float32 inputs -> (v_means, v_quats, v_scales, v_opacities, v_viewmat [4, 4]) as float64 tensors."""
    means, quats, scales, opac = (cg.np_f32(t) for t in inputs)
    n = means.shape[0]
    view16 = np.concatenate([cg.np_f32(vm)[:3, :3].reshape(-1), cg.np_f32(vm)[:3, 3],
                             np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)]).astype(np.float32)
    vis = np.ascontiguousarray(np.asarray(visible).astype(np.uint8))
    v = cg.np_f32(v_g2d)
    outs = [np.full(shape, np.nan) for shape in ((n, 3), (n, 4), (n, 3), (n,), (12,))]
    rc_ = lib.project_grad_host(n, _lib.CAMERA_MODELS[model], int(mode == "antialiased"), view16.ctypes.data, W, H, eps2d,
                                means.ctypes.data, quats.ctypes.data, scales.ctypes.data, opac.ctypes.data, vis.ctypes.data,
                                v.ctypes.data, *(o.ctypes.data_as(_D) for o in outs))
    assert rc_ == 0
    v_vm = torch.zeros(4, 4, dtype=torch.float64)
    v_vm[:3, :3], v_vm[:3, 3] = torch.from_numpy(outs[4][:9].reshape(3, 3)), torch.from_numpy(outs[4][9:])
    return [torch.from_numpy(o) for o in outs[:4]] + [v_vm]


def visible_rows(sc, model, mode="classic"):
    """What a projection keeps, from the float64 camera reference; the hand-made rows the test is about are asserted, not assumed."""
    ins = [t.numpy() for t in sc["inputs"]]
    ref = rc.project(*ins, sc["vm"].numpy(), sc["K"].numpy(), sc["W"], sc["H"], model, antialiased=mode == "antialiased")
    return torch.from_numpy(ref["ok"].copy())


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("model", ["pinhole", "ortho", "fisheye"])
def test_vjp_equals_float64_autograd_of_project_torch(host, model, mode):
    sc = cg.scene(model)
    vis = visible_rows(sc, model, mode)
    n = sc["inputs"][0].shape[0]
    pc = cg.camera_pc(sc["inputs"][0], sc["vm"])
    assert int(vis[:-cg.N_HAND].sum()) > 200
    assert vis[cg.NORM_ROWS].all()  # the quaternions of norm 0.1 and 10
    norms = sc["inputs"][1][cg.NORM_ROWS].norm(dim=1)
    assert abs(float(norms[0]) - 0.1) < 1e-6 and abs(float(norms[1]) - 10.0) < 1e-4
    if model == "pinhole":
        xp, xn, yp, yn = cg.clamp_limits(sc["K"], sc["W"], sc["H"])
        tx, ty = (pc[:, 0] / pc[:, 2])[cg.CLAMP_ROWS], (pc[:, 1] / pc[:, 2])[cg.CLAMP_ROWS]
        assert tx[0] > xp + 0.2 and tx[1] < -xn - 0.2 and ty[2] > yp + 0.2 and ty[3] < -yn - 0.2  # each clamp binds, on its side
        assert vis[cg.CLAMP_ROWS].all()  # ... on rows wide enough that the projection keeps them
    if model == "fisheye":
        assert vis[cg.AXIS_ROW] and float(pc[cg.AXIS_ROW, :2].abs().max()) < 1e-6  # below the 1e-7 terms' reach: rho = eps + ~0
    v_g2d = cg.random_v_g2d(n)
    truth = cg.projection_truth(*sc["inputs"], v_g2d, sc["vm"], sc["K"], sc["W"], sc["H"], EPS2D, model, mode, vis)
    got = run_host(host, sc["inputs"], sc["vm"], sc["K"], sc["W"], sc["H"], model, mode, vis, v_g2d)
    figures = {name: cg.fro_rel(g, t) for name, g, t in zip(("means", "quats", "scales", "opacities", "viewmat"), got, truth)}
    print(f"{model} {mode}: " + "  ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert all(torch.isfinite(t).all() for t in truth)
    assert all(float(t.abs().max()) > 0 for t in truth)
    assert not truth[4][3].any() and not got[4][3].any()
    for k, v in figures.items():
        assert v <= BOUND, (k, v)
    hidden = ~vis
    assert int(hidden.sum()) > 0
    for g in got[:4]:
        assert not g[hidden].any()
    if model == "pinhole":  # a clamped ratio passes no gradient into the Jacobian: the rows agree with autograd one by one as well
        for g, t in zip(got[:4], truth[:4]):
            assert cg.fro_rel(g[cg.CLAMP_ROWS], t[cg.CLAMP_ROWS]) <= BOUND


def test_exactly_on_the_fisheye_axis_the_vjp_is_finite(host):
    """x = y = 0 exactly (identity view): torch's sqrt has no gradient there (its autograd returns NaN for the mean), the cone
    rho = sqrt(x^2 + y^2) has none either; the vjp takes zero through rho and everything it returns is finite.  The row next to the axis
    (x = 1e-9) agrees with autograd, which is finite there."""
    means = torch.tensor([[0.0, 0.0, 2.5], [1e-9, 0.0, 2.5]])
    quats = torch.tensor([[0.9, 0.1, -0.3, 0.2], [0.9, 0.1, -0.3, 0.2]])
    scales = torch.tensor([[0.1, 0.07, 0.12], [0.1, 0.07, 0.12]])
    opac = torch.tensor([0.6, 0.6])
    K = torch.tensor([[60.0, 0, 32], [0, 60.0, 32], [0, 0, 1]])
    v = cg.random_v_g2d(2, seed=3)
    for mode in ("classic", "antialiased"):
        got = run_host(host, (means, quats, scales, opac), torch.eye(4), K, 64, 64, "fisheye", mode, [1, 1], v)
        assert all(torch.isfinite(g).all() for g in got)
        near = [1]
        truth = cg.projection_truth(means[near], quats[near], scales[near], opac[near], v[near], torch.eye(4), K, 64, 64, EPS2D,
                                    "fisheye", mode, None)
        one = run_host(host, (means[near], quats[near], scales[near], opac[near]), torch.eye(4), K, 64, 64, "fisheye", mode, [1],
                       v[near])
        assert all(cg.fro_rel(g, t) <= BOUND for g, t in zip(one, truth))


def test_hidden_rows_are_zero_and_add_nothing_to_the_view_sum(host):
    sc = cg.scene("pinhole")
    n = sc["inputs"][0].shape[0]
    vis = torch.rand(n, generator=torch.Generator().manual_seed(5)) < 0.5
    v_g2d = cg.random_v_g2d(n)
    # (a hidden row is never evaluated: non-finite inputs there must not reach anything)
    poisoned = [t.clone() for t in sc["inputs"]]
    poisoned[0][~vis] = float("nan")
    poisoned[2][~vis] = 0.0
    masked = run_host(host, poisoned, sc["vm"], sc["K"], sc["W"], sc["H"], "pinhole", "antialiased", vis, v_g2d)
    packed = run_host(host, [t[vis] for t in sc["inputs"]], sc["vm"], sc["K"], sc["W"], sc["H"], "pinhole", "antialiased",
                      torch.ones(int(vis.sum()), dtype=torch.bool), v_g2d[vis])
    for m, p in zip(masked[:4], packed[:4]):
        assert not m[~vis].any() and torch.equal(m[vis], p)
    assert torch.equal(masked[4], packed[4])  # the same rows added in the same order: the same bits


@pytest.mark.parametrize("kw", [dict(), dict(rasterize_mode="antialiased", render_mode="RGB+D")], ids=["plain", "antialiased-D"])
def test_the_yardsticks_viewmat_gradient_equals_finite_differences_of_its_own_loss(kw):
    """T0 with the mask held fixed: the loss is a smooth function of the twelve numbers of [R | t], and the float64 autograd
    gradient of the yardstick with the view matrix as a leaf equals central differences -- the idiom of
    tests/test_raster_grad_cpu.py for the other five tensors.  Under RGB+D the depth column adds its own share."""
    cfg, sc = cg.scene_np("T0")
    g = torch.Generator().manual_seed(29)
    inputs = (sc["means"], sc["quats"], sc["scales"], 0.9 * sc["opac"], torch.rand(cfg.n_gaussians, 3, generator=g))
    vm, K, W, H = sc["vms"][0], sc["K"], cfg.width, cfg.height
    Dp = 4 if "D" in kw.get("render_mode", "RGB") else 3
    G, A = torch.randn(H, W, Dp, generator=g), torch.randn(H, W, generator=g)
    cut = cg.fixed_cut(inputs, vm, K, W, H, **{k: v for k, v in kw.items() if k == "rasterize_mode"})
    assert 20_000 < int(cut["mask"].sum()) < W * H * cfg.n_gaussians
    grads, _ = cg.gradients(torch.float64, inputs, G, A, vm, K, W, H, cut, **kw)
    ins = [t.double() for t in inputs]
    raw = rg.rasterize(*ins, vm.double(), K, W, H, cut, **kw)[2]
    assert float(raw.max()) < 0.95  # (nothing near the clamp at 0.999, where the loss has a kink)

    def loss_at(delta):
        out, alpha, _ = rg.rasterize(*ins, vm.double() + delta, K, W, H, cut, **kw)
        return float((out * G.double()).sum() + (alpha * A.double()).sum())

    h = 1e-6
    fd = torch.zeros(4, 4, dtype=torch.float64)
    for i in range(3):
        for j in range(4):
            d = torch.zeros(4, 4, dtype=torch.float64)
            d[i, j] = h
            fd[i, j] = (loss_at(d) - loss_at(-d)) / (2 * h)
    fro, top = rg.errors(grads[5], fd)
    print(f"viewmat {kw}: autograd against central differences: {fro:.2e} (Frobenius), {top:.2e} (max)")
    assert not grads[5][3].any()
    assert fro < 1e-6 and top < 1e-6  # (central differences at h = 1e-6 in float64: ~1e-9 truncation + 1e-10 rounding)


def test_the_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gwbp.h")).read(), flags=re.S)
    mp = open(os.path.join(_lib.CSRC, "gwbp.map")).read()
    assert re.search(r"global:\s*gwbp_\*;", mp)
    for name in ("gwbp_project_backward", "gwbp_project_backward_blocks"):
        assert re.search(r"GWBP_API int %s\(" % name, hdr)
        assert name in _lib.ARGTYPES and name in _lib.EXPORTS and name in mp
        assert getattr(_lib.lib(), name).argtypes == _lib.ARGTYPES[name]
    assert "project_grad.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    L = _lib.lib()
    assert [L.gwbp_project_backward_blocks(n) for n in (0, 1, 256, 257, 1_000_000)] == [0, 1, 1, 2, 3907]
    assert L.gwbp_project_backward_blocks(-1) == -1


def test_project_backward_refuses_bad_arguments_before_any_device_call():
    """Each null input, all outputs null, v_viewmat without scratch, misaligned pointers, an unknown camera or mode: GWBP_EINVAL with a
    message.  Every pointer is a fake aligned host address and the workspace is never touched: these calls return before any HIP call
    (this test runs without a GPU)."""
    L = _lib.lib()
    caps = _lib.Caps(10, 1 << 16, 1 << 20, 64, 64)
    nbytes = C.c_size_t(0)
    assert L.gwbp_workspace_size(C.byref(caps), C.byref(nbytes)) == 0
    view = _lib.View()
    view.width, view.height = 64, 64
    view.K[0] = view.K[4] = 50.0
    buf = (C.c_char * 512)()
    fake = C.c_void_p((C.addressof(buf) + 255) & ~255)
    odd, four = C.c_void_p(fake.value + 2), C.c_void_p(fake.value + 4)
    names = ("means", "quats", "scales", "opacities", "v_g2d", "v_means", "v_quats", "v_scales", "v_opacities", "v_viewmat", "scratch")

    def call(camera=0, mode=0, **over):
        args = [over.get(k, fake) for k in names]
        rc_ = L.gwbp_project_backward(C.byref(caps), fake, nbytes, C.byref(view), camera, mode, *args, None)
        return rc_, L.gwbp_last_error_string()

    cases = [(dict(camera=3), b"unknown camera model 3"), (dict(mode=2), b"unknown rasterize mode 2")]
    cases += [({k: None}, f"null {k}".encode()) for k in names[:5]]
    cases += [({k: None for k in names[5:10]}, b"every output is null"), (dict(scratch=None), b"v_viewmat needs the scratch"),
              (dict(quats=four), b"16-B aligned"), (dict(v_quats=four), b"16-B aligned"), (dict(means=odd), b"4-B aligned"),
              (dict(v_g2d=odd), b"4-B aligned"), (dict(v_opacities=odd), b"4-B aligned"), (dict(v_viewmat=four), b"8-B aligned"),
              (dict(scratch=four), b"8-B aligned")]
    for kw, msg in cases:
        rc_, err = call(**kw)
        assert rc_ == -1 and msg in err, (kw, rc_, err)


def test_run_localize_parses_its_documented_options():
    import sys
    sys.path.insert(0, ROOT)
    import run_localize
    ap = run_localize.build_parser()
    a = ap.parse_args(["--synthetic", "T0", "--field", "t.pt", "--target", "m.npy", "--weights", "w.pt", "--init-view", "1", "--perturb",
                       "0.01,0,-0.02,0.1,0,0", "--steps", "7", "--lr", "0.01", "--loss", "cosine", "--camera-model", "fisheye", "--out",
                       "pose.json"])
    assert a.perturb == [0.01, 0.0, -0.02, 0.1, 0.0, 0.0] and a.steps == 7 and a.loss == "cosine" and a.init_pose is None
    for bad in (["--target", "m.pt", "--out", "o.json"],                                                   # no initial pose
                ["--target", "m.pt", "--out", "o.json", "--init-view", "0", "--init-pose", "p.json"],      # two of them
                ["--target", "m.pt", "--out", "o.json", "--init-view", "0", "--perturb", "1,2,3"]):        # a twist has six numbers
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_se3_exp_and_pose_error():
    assert torch.equal(se3_exp(torch.zeros(6, dtype=torch.float64)), torch.eye(4, dtype=torch.float64))
    assert torch.equal(se3_exp(torch.zeros(6)), torch.eye(4))
    g = torch.Generator().manual_seed(13)
    for _ in range(20):
        w = torch.randn(3, generator=g, dtype=torch.float64)
        w = w / w.norm() * torch.rand(1, generator=g, dtype=torch.float64)  # up to 1 rad
        tw = torch.cat([w, torch.randn(3, generator=g, dtype=torch.float64)])
        E = se3_exp(tw)
        R = E[:3, :3]
        assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12 and abs(float(torch.det(R)) - 1.0) < 1e-12
        assert torch.equal(E[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))
        vm = se3_exp(torch.tensor([0.3, -0.2, 0.5, 0.1, 2.0, -1.0], dtype=torch.float64))
        angle, dist = pose_error(E @ vm, vm)
        assert abs(angle - float(w.norm())) < 1e-12 and abs(dist - float(E[:3, 3].norm())) < 1e-12
    # the Jacobian at zero: the six generators of se(3), rotations first
    J = torch.autograd.functional.jacobian(se3_exp, torch.zeros(6, dtype=torch.float64))  # [4, 4, 6]
    gen = torch.zeros(4, 4, 6, dtype=torch.float64)
    gen[2, 1, 0], gen[1, 2, 0] = 1, -1
    gen[0, 2, 1], gen[2, 0, 1] = 1, -1
    gen[1, 0, 2], gen[0, 1, 2] = 1, -1
    gen[0, 3, 3] = gen[1, 3, 4] = gen[2, 3, 5] = 1
    assert float((J - gen).abs().max()) < 1e-14
    # a pure rotation about the camera centre leaves the centre where it is; a pure translation turns nothing
    vm = se3_exp(torch.tensor([0.3, -0.2, 0.5, 0.1, 2.0, -1.0], dtype=torch.float64))
    angle, dist = pose_error(se3_exp(torch.tensor([0.0, 0.04, 0.0, 0, 0, 0], dtype=torch.float64)) @ vm, vm)
    assert abs(angle - 0.04) < 1e-14 and dist < 1e-14
    angle, dist = pose_error(se3_exp(torch.tensor([0, 0, 0, 0.03, -0.04, 0.0], dtype=torch.float64)) @ vm, vm)
    assert angle < 1e-14 and abs(dist - 0.05) < 1e-14
