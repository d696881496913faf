"""The camera gradient on the GPU: k_project_bwd alone (Engine.project_backward) against torch's float64 autograd of project_torch,
and rasterization(camera_grad=True) -- the blend backward, then the projection backward -- against the dense yardstick with the view
matrix as a sixth leaf (tests/camera_grad_ref.py), in the FACTOR x float32-floor rule of tests/test_gpu_raster_grad.py.

Bounds of the kernel alone.  It evaluates project_grad.h in float64 on the stored float32 inputs, which tests/test_project_grad_cpu.py
holds within 1e-9 Frobenius-relative of that autograd (measured: 3e-15, 1e-13 under the fisheye camera).  v_viewmat stays float64: 1e-9.
The per-Gaussian outputs are that double rounded once to float32: 2^-24 + 1e-9 < 6.1e-8.
"""
import functools

import pytest
import torch

import camera_grad_ref as cg
import gsbp_amd
import raster_grad_ref as rg
import test_gpu_raster_grad as base
from gsbp_amd import rasterization
from gsbp_amd.pose import pose_error, refine_pose
from test_gpu_raster_grad import FACTOR, check  # noqa: F401  (the project's rule: kernel error <= FACTOR x the float32 floor)

pytestmark = pytest.mark.gpu
BOUND_VIEW = 1e-9
BOUND_ROW = 2.0 ** -24 + 1e-9
B = 256  # k_project_bwd's block (kScanBlock)
OUT_NAMES = ("means", "quats", "scales", "opacities", "viewmat")


# ---- the kernel alone ----------------------------------------------------------------------------------------------------------------
def project_and_backward(dev, sc, model, mode, v_g2d, needs=(True,) * 4, want_viewmat=True, calls=1):
    """Project the scene under (model, mode) on a fresh engine, then Engine.project_backward `calls` times on the same inputs."""
    ins = [t.to(dev).contiguous() for t in sc["inputs"]]
    eng = gsbp_amd.Engine(ins[0].shape[0], sc["W"], sc["H"], device=dev)
    view = eng.view(sc["vm"], sc["K"], sc["W"], sc["H"], camera_model=model, rasterize_mode=mode)
    proj = eng.project(view, *ins, want_outputs=True)
    v = v_g2d.to(dev)
    outs = [eng.project_backward(view, *ins, v, needs, want_viewmat) for _ in range(calls)]
    return outs, (proj["radii"] > 0).cpu(), float(view.eps2d)


def against_autograd(sc, model, mode, got, vis, eps2d, v_g2d, label):
    truth = cg.projection_truth(*sc["inputs"], v_g2d, sc["vm"], sc["K"], sc["W"], sc["H"], eps2d, model, mode, vis)
    figures = {}
    for name, g, t in zip(OUT_NAMES, got, truth):
        assert g.dtype == (torch.float64 if name == "viewmat" else torch.float32), name
        if float(t.norm()) == 0.0:  # (nothing visible: the truth is all zero, and so must the kernel's be)
            assert not g.any(), name
            continue
        figures[name] = cg.fro_rel(g, t)
    print(f"{label}: " + "  ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    for name, f in figures.items():
        assert f <= (BOUND_VIEW if name == "viewmat" else BOUND_ROW), (label, name, f)
    for g in got[:4]:
        assert not g.cpu()[~vis].any()
    assert not got[4][3].any()
    return figures


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("model", ["pinhole", "ortho", "fisheye"])
def test_kernel_against_float64_autograd(dev, model, mode):
    sc = cg.scene(model)
    n = sc["inputs"][0].shape[0]
    v_g2d = cg.random_v_g2d(n)
    (got,), vis, eps2d = project_and_backward(dev, sc, model, mode, v_g2d)
    assert int(vis[:-cg.N_HAND].sum()) > 200 and vis[cg.NORM_ROWS].all()
    print(f"{model} {mode}: {int(vis.sum())} of {n} rows visible")
    pc = cg.camera_pc(sc["inputs"][0], sc["vm"])
    if model == "pinhole":  # the hand-made rows beyond each clamp limit: clamped, and kept by k_project
        xp, xn, yp, yn = cg.clamp_limits(sc["K"], sc["W"], sc["H"])
        tx, ty = (pc[:, 0] / pc[:, 2])[cg.CLAMP_ROWS], (pc[:, 1] / pc[:, 2])[cg.CLAMP_ROWS]
        assert tx[0] > xp + 0.2 and tx[1] < -xn - 0.2 and ty[2] > yp + 0.2 and ty[3] < -yn - 0.2
        assert vis[cg.CLAMP_ROWS].all()
    if model == "fisheye":
        assert vis[cg.AXIS_ROW] and float(pc[cg.AXIS_ROW, :2].abs().max()) < 1e-6
    against_autograd(sc, model, mode, got, vis, eps2d, v_g2d, f"{model} {mode}")


def _last_rows(n, cull_block=None):
    """The last n rows of T0 + the hand-made rows (the hand-made ones are always among them); cull_block: the rows of that block of B
    are mirrored to behind the camera."""
    sc = cg.scene("pinhole")
    ins = [t[-n:].clone() for t in sc["inputs"]]
    if cull_block is not None:
        rows = slice(cull_block * B, (cull_block + 1) * B)
        R, t = sc["vm"][:3, :3].double(), sc["vm"][:3, 3].double()
        pc = cg.camera_pc(ins[0][rows], sc["vm"])
        pc[:, 2] = -pc[:, 2]
        ins[0][rows] = ((pc - t) @ R).float()
    return dict(sc, inputs=tuple(t.contiguous() for t in ins))


@pytest.mark.parametrize("n, cull", [(1, None), (B - 1, None), (B, None), (B + 1, None), (2 * B + 1, None), (2 * B + 1, 1)],
                         ids=["1", "B-1", "B", "B+1", "2B+1", "2B+1-block-1-culled"])
def test_block_boundaries_of_the_reduction(dev, n, cull):
    sc = _last_rows(n, cull)
    v_g2d = cg.random_v_g2d(n, seed=11)
    (got,), vis, eps2d = project_and_backward(dev, sc, "pinhole", "antialiased", v_g2d)
    assert vis[-1] and int(vis.sum()) >= 1
    if cull is not None:
        assert not vis[cull * B:(cull + 1) * B].any() and vis[:B].any() and vis[2 * B:].any()
    against_autograd(sc, "pinhole", "antialiased", got, vis, eps2d, v_g2d, f"N={n} cull={cull}")


def test_two_calls_give_the_same_bits(dev):
    sc = cg.scene("fisheye")
    v_g2d = cg.random_v_g2d(sc["inputs"][0].shape[0])
    (a, b), _, _ = project_and_backward(dev, sc, "fisheye", "antialiased", v_g2d, calls=2)
    for name, x, y in zip(OUT_NAMES, a, b):
        assert torch.equal(x, y), name


def test_needs_and_want_viewmat_do_not_change_what_is_computed(dev):
    sc = cg.scene("pinhole")
    v_g2d = cg.random_v_g2d(sc["inputs"][0].shape[0])
    (full,), _, _ = project_and_backward(dev, sc, "pinhole", "classic", v_g2d)
    (view_only,), _, _ = project_and_backward(dev, sc, "pinhole", "classic", v_g2d, needs=(False,) * 4)
    (rows_only,), _, _ = project_and_backward(dev, sc, "pinhole", "classic", v_g2d, want_viewmat=False)
    assert all(x is None for x in view_only[:4]) and torch.equal(view_only[4], full[4])
    assert rows_only[4] is None and all(torch.equal(x, y) for x, y in zip(rows_only[:4], full[:4]))
    (some,), _, _ = project_and_backward(dev, sc, "pinhole", "classic", v_g2d, needs=(False, True, False, True), want_viewmat=False)
    assert some[0] is None and some[2] is None and torch.equal(some[1], full[1]) and torch.equal(some[3], full[3])
    with pytest.raises(gsbp_amd.GwbpError):
        project_and_backward(dev, sc, "pinhole", "classic", v_g2d, needs=(False,) * 4, want_viewmat=False)


# ---- rasterization(camera_grad=True) against the yardstick -------------------------------------------------------------------------
CASES = {name: base.CASES[name] for name in ("t0", "fisheye", "ortho", "antialiased", "backgrounds")}
CASES["rgb+d"] = lambda: dict(base._t0(), render_mode="RGB+D")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case, the kernels' cut, G, A and the yardstick's six float64 and float32 gradients: computed once, shared, never modified."""
    case = CASES[name]()
    dev = torch.device("cuda:0")
    cut = rg.kernel_cut(dev, *case["inputs"][:4], case["vm"], case["K"], case["W"], case["H"], **base._view_kw(case))
    G, A = base._weights(case)
    kw = {k: case[k] for k in ("camera_model", "rasterize_mode", "render_mode", "background") if k in case}
    truth, _ = cg.gradients(torch.float64, case["inputs"], G, A, case["vm"], case["K"], case["W"], case["H"], cut, **kw)
    floor, _ = cg.gradients(torch.float32, case["inputs"], G, A, case["vm"], case["K"], case["W"], case["H"], cut, **kw)
    return dict(case=case, G=G, A=A, truth=truth, floor=floor)


def kernel_gradients(dev, case, G, A, leaves=(True,) * 5, vms=None, pick=0):
    """The six gradients of rasterization(camera_grad=True); leaves: which of the five Gaussian tensors require grad (None for the
    others); vms [C, 4, 4]: more cameras in one call, the loss on camera `pick`."""
    ins = [t.to(dev).requires_grad_(bool(on)) for t, on in zip(case["inputs"], leaves)]
    vm = (case["vm"][None] if vms is None else vms).to(dev).requires_grad_(True)
    kw = dict(base._view_kw(case), render_mode=case.get("render_mode", "RGB"), want_meta=False, camera_grad=True)
    if case.get("background") is not None:
        kw["backgrounds"] = case["background"].to(dev)[None].expand(vm.shape[0], -1)
    out, alphas, _ = rasterization(*ins, vm, case["K"].to(dev)[None].expand(vm.shape[0], -1, -1), case["W"], case["H"], **kw)
    loss = (out[pick] * G.to(dev)).sum() + (alphas[pick, ..., 0] * A.to(dev)).sum()
    loss.backward()
    assert vm.grad.dtype == torch.float32 and vm.grad.shape == vm.shape and not vm.grad[:, 3].any()
    return [None if t.grad is None else t.grad.cpu() for t in ins] + [vm.grad.cpu()]


def rows_of(name, kernel, truth, floor, tensors=range(6)):
    rows = []
    for i in tensors:
        (ffro, ftop), (kfro, ktop) = rg.errors(floor[i], truth[i]), rg.errors(kernel[i], truth[i])
        rows.append(dict(case=name, tensor=cg.NAMES[i], floor_fro=ffro, floor_max=ftop, kernel_fro=kfro, kernel_max=ktop))
        print(f"{name:12s} {cg.NAMES[i]:9s} floor {ffro:.2e} / {ftop:.2e}   kernel {kfro:.2e} / {ktop:.2e}   ratio "
              f"{kfro / max(ffro, 1e-300):.2f} / {ktop / max(ftop, 1e-300):.2f}")
    return rows


def run_case(dev, name):
    ref = reference(name)
    kernel = kernel_gradients(dev, ref["case"], ref["G"], ref["A"])
    return rows_of(name, kernel, ref["truth"], ref["floor"]), kernel


@pytest.mark.parametrize("name", list(CASES))
def test_all_six_gradients_against_the_yardstick(dev, name):
    ref = reference(name)
    assert float(ref["truth"][5].abs().max()) > 0 and not ref["truth"][5][3].any()
    rows, kernel = run_case(dev, name)
    assert not kernel[5][0, 3].any()
    check(rows)


def test_camera_only(dev):
    """Only viewmats requires grad: the same view-matrix gradient, by the same rule, and nothing else gets a .grad."""
    ref = reference("t0")
    kernel = kernel_gradients(dev, ref["case"], ref["G"], ref["A"], leaves=(False,) * 5)
    assert all(g is None for g in kernel[:5])
    check(rows_of("camera-only", kernel, ref["truth"], ref["floor"], tensors=[5]))


def test_two_cameras_in_one_call(dev):
    """C = 2: each camera's [4, 4] gradient is its own single-camera call's, by the same rule; the other camera's stays zero."""
    cfg, sc = cg.scene_np("T0")
    for pick, name in enumerate(("stale-view-0", "stale-view-1")):  # (test_gpu_raster_grad's two T0 views)
        CASES.setdefault(name, base.CASES[name])
        ref = reference(name)
        kernel = kernel_gradients(dev, ref["case"], ref["G"], ref["A"], vms=sc["vms"][:2], pick=pick)
        assert not kernel[5][1 - pick].any()
        check(rows_of(f"C=2 camera {pick}", kernel[:5] + [kernel[5][pick][None]], ref["truth"], ref["floor"]))


def test_what_still_raises(dev):
    case = base._t0(3)
    K, W, H = case["K"].to(dev)[None], case["W"], case["H"]

    def leaves(c=case):
        return [t.to(dev) for t in c["inputs"]], case["vm"].to(dev)[None].requires_grad_(True)

    ins, vm = leaves()
    out, _, _ = rasterization(*ins, vm, K, W, H, want_meta=False)  # the default call: opt-in only
    with pytest.raises(NotImplementedError, match="viewmats"):
        out.sum().backward()
    with pytest.raises(NotImplementedError, match="camera_grad"):
        rasterization(*ins, vm, K, W, H, want_meta=False)[0].sum().backward()
    with pytest.raises(NotImplementedError, match="Ks"):
        rasterization(*ins, vm, K.clone().requires_grad_(True), W, H, want_meta=False, camera_grad=True)
    sh = base._t0(sh=True)
    ins_sh, _ = leaves(sh)
    with pytest.raises(NotImplementedError, match="sh_degree"):
        rasterization(*ins_sh, vm, K, W, H, sh_degree=3, want_meta=False, camera_grad=True)
    wide, _ = leaves(base._t0(48))
    with pytest.raises(NotImplementedError, match="at most 32 channels"):
        rasterization(*wide, vm, K, W, H, want_meta=False, camera_grad=True)
    # camera_grad=True with nothing to differentiate is the plain call
    out, _, _ = rasterization(*ins, vm.detach(), K, W, H, want_meta=False, camera_grad=True)
    assert not out.requires_grad


# ---- the refiner ---------------------------------------------------------------------------------------------------------------------
def gpu_refine(dev, case, **kw):
    """refine_pose on the case of camera_grad_ref.pose_case: the target is rasterization()'s own D = 3 render from the true pose."""
    gauss = [t.to(dev) for t in case["inputs"]]
    table = case["table"].to(dev)
    with torch.no_grad():
        target = rasterization(*gauss, table, case["vm_true"].to(dev)[None], case["K"].to(dev)[None], case["W"], case["H"],
                               want_meta=False)[0][0]
    return refine_pose(*gauss, table, target, case["vm0"], case["K"], case["W"], case["H"], steps=cg.POSE_STEPS, lr=cg.POSE_LR, **kw)


def test_refine_pose_moves_towards_the_true_pose(dev):
    """Conditions, not measurements: the loss ends below where it started and so do both components of the pose error.  The float64
    dense yardstick under the same Adam loop reaches loss x 0.0019, angle x 0.107, distance x 0.107 (camera_grad_ref.yardstick_refine;
    tools/time_raster_grad.py records its factors and this run's)."""
    case = cg.pose_case()
    res = gpu_refine(dev, case)
    loss, angle, dist = cg.pose_factors(res, case)
    print(f"refine_pose: loss x {loss:.4f}, angle x {angle:.4f}, distance x {dist:.4f} in {cg.POSE_STEPS} steps")
    assert len(res["history"]) == cg.POSE_STEPS and res["viewmat"].shape == (4, 4) and res["twist"].shape == (6,)
    assert res["history"][-1] < res["history"][0]
    a0, d0 = pose_error(case["vm0"], case["vm_true"])
    a1, d1 = pose_error(res["viewmat"], case["vm_true"])
    assert a1 < a0 and d1 < d0
