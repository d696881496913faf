"""The yardsticks of the camera gradient: tests/raster_grad_ref.py's dense restatement with the view matrix as a sixth leaf, the float64
autograd of project_torch as the truth of the projection backward alone, and the scene both are asked on -- T0 with a few hand-made
rows appended that sit where the projection's function changes form.

The cut (which pairs count, in which order, which rows are visible) comes from the kernels through raster_grad_ref.kernel_cut, or from
a fixed rule in the CPU self-test, exactly as for the other five tensors.
"""
import numpy as np
import torch

import raster_grad_ref as rg
from gsbp_amd.projection import CLAMP_MARGIN, project_torch
from util import scene_np

NAMES = rg.NAMES + ("viewmat",)


def gradients(dtype, inputs, G, A, viewmat, K, W, H, cut, **kw):
    """The six gradients (NAMES' order; the last one [4, 4], its bottom row zero) of sum(out G) + sum(alpha_img A) in `dtype`."""
    ins = [t.detach().cpu().to(dtype).requires_grad_(True) for t in inputs]
    vm = viewmat.detach().cpu().to(dtype).requires_grad_(True)
    out, alpha, _ = rg.rasterize(*ins, vm, K.cpu(), W, H, cut, **kw)
    loss = (out * G.cpu().to(dtype)).sum() + (alpha * A.cpu().to(dtype)).sum()
    grads = torch.autograd.grad(loss, ins + [vm], allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(grads, ins + [vm])], loss.detach()


def projection_truth(means, quats, scales, opacities, v_g2d, viewmat, K, W, H, eps2d, model, mode, visible):
    """(v_means, v_quats, v_scales, v_opacities, v_viewmat [4, 4]) in float64: torch.autograd.grad of project_torch on the float32
    values widened, fed the v_g2d rows (mx, my, ca, cb, cc, o) as the gradients of its three outputs."""
    ins = [t.detach().cpu().double().requires_grad_(True) for t in (means, quats, scales, opacities)]
    vm = viewmat.detach().cpu().double().requires_grad_(True)
    out = project_torch(*ins, vm, K.cpu(), W, H, eps2d, model, mode, visible)
    v = v_g2d.detach().cpu().double()
    return torch.autograd.grad(out, ins + [vm], (v[:, :2], v[:, 2:5], v[:, 5]))


def fixed_cut(inputs, vm, K, W, H, **kw):
    """A cut for a run without the kernels: every row visible, the front stage's order, and the pairs the blend's own rule without
    termination keeps (o exp(-sigma) >= 1/255), decided once in float64 and then held fixed."""
    n = inputs[0].shape[0]
    ins = [t.double() for t in inputs]
    depths = (ins[0] @ vm.double()[:3, :3].T + vm.double()[:3, 3])[:, 2].float()
    cut = dict(mask=torch.ones(W * H, n, dtype=torch.bool), visible=torch.ones(n, dtype=torch.bool))
    cut["order"] = rg.depth_order(depths, cut["visible"])
    raw = rg.render(*ins, vm, K, W, H, cut, **kw)[2]
    return dict(cut, mask=(raw >= 1.0 / 255.0)[:, torch.argsort(cut["order"])])


def fro_rel(got, truth):
    got, truth = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(truth).detach().cpu().double()
    return float((got - truth).norm()) / float(truth.norm())


def clamp_limits(K, W, H):
    """(x+ , x-, y+, y-) limits of x/z and y/z inside the pinhole Jacobian, in float64."""
    fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    tx, ty = 0.5 * W / fx, 0.5 * H / fy
    return ((W - cx) / fx + CLAMP_MARGIN * tx, cx / fx + CLAMP_MARGIN * tx, (H - cy) / fy + CLAMP_MARGIN * ty,
            cy / fy + CLAMP_MARGIN * ty)


N_HAND = 7
CLAMP_ROWS = slice(-7, -3)   # x/z beyond +limit, beyond -limit, y/z beyond +limit, beyond -limit
AXIS_ROW = -3                # camera-space x = y = 0 to float32 rounding
NORM_ROWS = slice(-2, None)  # quaternions of norm 0.1 and 10


def hand_rows(vm, K, W, H):
    """Seven Gaussians placed in the CAMERA space of `vm`: four whose x/z or y/z lies 0.25 beyond one clamp limit of the pinhole
    Jacobian, wide enough (0.9 in each axis at depth 3) that their 3-sigma square still reaches the image; one on the optical axis;
    two in front of the camera whose quaternions have norm 0.1 and 10."""
    xp, xn, yp, yn = clamp_limits(K, W, H)
    z = 3.0
    pc = torch.tensor([[(xp + 0.25) * z, 0.1, z], [-(xn + 0.25) * z, -0.2, z], [0.15, (yp + 0.25) * z, z], [-0.1, -(yn + 0.25) * z, z],
                       [0.0, 0.0, 2.5], [0.2, -0.1, 3.0], [-0.3, 0.15, 3.5]], dtype=torch.float64)
    R, t = vm[:3, :3].double(), vm[:3, 3].double()
    means = ((pc - t) @ R).float()  # R^T (pc - t)
    g = torch.Generator().manual_seed(41)
    quats = torch.randn(N_HAND, 4, generator=g)
    quats = quats / quats.norm(dim=1, keepdim=True)
    quats[-2] *= 0.1
    quats[-1] *= 10.0
    scales = torch.cat([0.9 * (0.8 + 0.4 * torch.rand(4, 3, generator=g)), 0.05 + 0.1 * torch.rand(3, 3, generator=g)])
    opac = 0.3 + 0.5 * torch.rand(N_HAND, generator=g)
    return means, quats, scales, opac


def camera_pc(means, vm):
    """Camera-space positions in float64 of float32 means."""
    return means.double() @ vm[:3, :3].double().T + vm[:3, 3].double()


def scene(model="pinhole", view=0, n=None):
    """T0 (its first n rows) with the hand-made rows of `view` appended: dict(inputs (means, quats, scales, opac), vm, K, W, H).  The
    ortho camera gets test_gpu_raster_grad's focal length (0.4 W): T0's x, y reach +-1.7."""
    cfg, sc = scene_np("T0")
    vm, K = sc["vms"][view], sc["K"].clone()
    if model == "ortho":
        K[0, 0] = K[1, 1] = 0.4 * cfg.width
    hand = hand_rows(vm, K, cfg.width, cfg.height)
    base = [sc[k][:n] for k in ("means", "quats", "scales", "opac")]
    return dict(inputs=tuple(torch.cat([b, h]).contiguous() for b, h in zip(base, hand)), vm=vm, K=K, W=cfg.width, H=cfg.height)


# The pose-refinement case of the tests and of tools/time_raster_grad.py: T0 seen from its view 0, started a few hundredths of a radian
# and of the scene's extent (2) away.  twist0, lr and steps were chosen on the float64 dense yardstick below (no kernel involved): with
# them its loss and both components of its pose error end below where they started (profiles/project_backward.json has the factors).
POSE_TWIST0 = (0.03, -0.02, 0.025, 0.05, -0.04, 0.06)
POSE_LR, POSE_STEPS = 5e-3, 50


def pose_case():
    """dict(inputs, table [N, 3], vm_true, vm0 (float64), K, W, H) of the refinement case."""
    from gsbp_amd.pose import se3_exp
    cfg, sc = scene_np("T0")
    table = torch.rand(cfg.n_gaussians, 3, generator=torch.Generator().manual_seed(31))
    vm_true = sc["vms"][0]
    vm0 = se3_exp(torch.tensor(POSE_TWIST0, dtype=torch.float64)) @ vm_true.double()
    return dict(inputs=(sc["means"], sc["quats"], sc["scales"], sc["opac"]), table=table, vm_true=vm_true, vm0=vm0, K=sc["K"],
                W=cfg.width, H=cfg.height)


def yardstick_refine(case, steps=POSE_STEPS, lr=POSE_LR):
    """refine_pose's Adam loop (pose.optimize_twist) driven by the float64 dense restatement on the CPU, the cut re-decided at every
    pose by fixed_cut's rule; the target is the restatement's own render from vm_true."""
    from gsbp_amd.pose import optimize_twist, pose_loss
    ins = [t.double() for t in case["inputs"]] + [case["table"].double()]
    K, W, H = case["K"], case["W"], case["H"]

    def render(vm):
        cut = fixed_cut(ins, vm.detach(), K, W, H)
        return rg.render(*ins, vm, K, W, H, cut)[0]

    target = render(case["vm_true"].double()).detach()
    return optimize_twist(lambda vm: pose_loss(render(vm), target, None, "l2"), case["vm0"], steps, lr)


def pose_factors(res, case):
    """(final loss / first loss, final angle / initial angle, final distance / initial distance) of a refinement result."""
    from gsbp_amd.pose import pose_error
    a0, d0 = pose_error(case["vm0"], case["vm_true"])
    a1, d1 = pose_error(res["viewmat"], case["vm_true"])
    return res["history"][-1] / res["history"][0], a1 / a0, d1 / d0


def random_v_g2d(n, seed=7):
    return torch.randn(n, 6, generator=torch.Generator().manual_seed(seed))


def np_f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))
