"""The camera side of a lifted scene: where was this image, or this feature map, taken from?

`rasterization(camera_grad=True)` differentiates a render with respect to its view matrix (gwbp_project_backward sums the projection's
gradient over the Gaussians; the depth column of the "D" render modes adds its own through torch).  On top of that:

    se3_exp(twist)            the rigid motion of a 6-vector (rotation vector, then translation), differentiable, exact at zero
    pose_error(vm_a, vm_b)    (angle in radians, distance of the camera centres) between two world-to-camera matrices
    refine_pose(...)          Adam on the six numbers of a twist applied in front of an initial view matrix, against a target image
                              or feature map of at most 32 channels
    PoseAdjust                a learnt [V, 9] correction per view (translation + 6-D rotation), the reference trainer's CameraOptModule
    PoseTraining              train_scene's pose_opt / pose_noise state: the corrections, their Adam and the pose_err monitor

In refine_pose the Gaussians are fixed and only the camera moves; PoseTraining moves the cameras while train_scene trains the Gaussians.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from ._lib import GwbpError
from .rasterization import GEOMETRY_GRAD_MAX_DIM, rasterization


def se3_exp(twist: torch.Tensor) -> torch.Tensor:
    """[6] (rotation vector w, translation v) -> the [4, 4] rigid motion exp([[w]x, v], [0, 0]]) in closed form, computed in float64
    and returned in the dtype of `twist`: R = I + a K + b K^2, t = (I + b K + c K^2) v with K = [w]x, a = sin(th) / th,
    b = (1 - cos(th)) / th^2, c = (th - sin(th)) / th^3.  Below th = 0.1 the three are their Taylor series in th^2 (through th^8: 3e-18),
    so that the map is the identity at zero and differentiable there."""
    if twist.shape != (6,):
        raise ValueError(f"twist must have shape [6], got {tuple(twist.shape)}")
    tw = twist.double()
    w, v = tw[:3], tw[3:]
    t = (w * w).sum()
    small = t < 1e-2
    th = torch.sqrt(torch.where(small, torch.ones_like(t), t))  # (no sqrt at zero: its gradient is infinite there)
    half = torch.sin(0.5 * th)
    a = torch.where(small, 1 + t * (-1 / 6 + t * (1 / 120 + t * (-1 / 5040 + t / 362880))), torch.sin(th) / th)
    b = torch.where(small, 0.5 + t * (-1 / 24 + t * (1 / 720 + t * (-1 / 40320 + t / 3628800))), 2 * half * half / (th * th))
    c = torch.where(small, 1 / 6 + t * (-1 / 120 + t * (1 / 5040 + t * (-1 / 362880 + t / 39916800))),
                    (th - torch.sin(th)) / (th * th * th))
    zero = torch.zeros_like(t)
    K = torch.stack([torch.stack([zero, -w[2], w[1]]), torch.stack([w[2], zero, -w[0]]), torch.stack([-w[1], w[0], zero])])
    K2 = K @ K
    eye = torch.eye(3, dtype=torch.float64, device=tw.device)
    top = torch.cat([eye + a * K + b * K2, ((eye + b * K + c * K2) @ v)[:, None]], dim=1)
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64, device=tw.device)
    return torch.cat([top, bottom], dim=0).to(twist.dtype)


def pose_error(vm_a: torch.Tensor, vm_b: torch.Tensor) -> Tuple[float, float]:
    """(angle of the relative rotation in radians, distance between the two camera centres) of two world-to-camera matrices."""
    a, b = vm_a.detach().double().cpu(), vm_b.detach().double().cpu()
    Ra, Rb = a[:3, :3], b[:3, :3]
    D = Ra @ Rb.T
    skew = torch.stack([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    angle = torch.atan2(0.5 * skew.norm(), 0.5 * (torch.trace(D) - 1.0))
    ca, cb = -(Ra.T @ a[:3, 3]), -(Rb.T @ b[:3, 3])
    return float(angle), float((ca - cb).norm())


def rotation_6d(d6: torch.Tensor) -> torch.Tensor:
    """[..., 6] -> [..., 3, 3]: the rotation whose ROWS are the Gram-Schmidt basis of the two 3-vectors of d6 and their cross product
    (Zhou et al., "On the Continuity of Rotation Representations in Neural Networks", 2019), as the reference trainer builds it."""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.linalg.cross(b1, b2, dim=-1)), dim=-2)


def rigid_inverse(mats: torch.Tensor) -> torch.Tensor:
    """The inverse of rigid motions [..., 4, 4] in closed form: [[R^T, -R^T t], [0, 1]] (no factorisation, nothing read on the host)."""
    Rt = mats[..., :3, :3].transpose(-1, -2)
    top = torch.cat([Rt, -(Rt @ mats[..., :3, 3:])], dim=-1)
    return torch.cat([top, mats[..., 3:, :]], dim=-2)


class PoseAdjust:
    """A learnt correction per view, the reference trainer's CameraOptModule restated for view matrices.  `table` [V, 9] on the device:
    a translation delta dx and a 6-D rotation delta that is added to (1, 0, 0, 0, 1, 0) and made orthonormal by Gram-Schmidt (R).  The
    reference right-multiplies the camera-to-world matrix by T = [R | dx]; the view matrix of that camera is inverse(c2w @ T) =
    inverse(T) @ viewmat = [[R^T, -R^T dx], [0, 1]] @ viewmat, which needs no matrix inverse.  Plain torch on 4x4 matrices."""

    def __init__(self, n_views: int, device=None, dtype=torch.float32):
        if isinstance(n_views, bool) or not isinstance(n_views, int) or n_views < 1:
            raise ValueError(f"PoseAdjust needs a positive number of views, got {n_views!r}")
        self.table = torch.zeros(n_views, 9, device=device, dtype=dtype)
        self.identity = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], device=device, dtype=dtype)

    def zero_init(self) -> "PoseAdjust":
        with torch.no_grad():
            self.table.zero_()
        return self

    def random_init(self, std: float, seed: int = 0) -> "PoseAdjust":
        """Normal draws of standard deviation std, from torch.Generator().manual_seed(seed) on the host."""
        draw = torch.randn(self.table.shape, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float64) * float(std)
        with torch.no_grad():
            self.table.copy_(draw.to(self.table.dtype))
        return self

    def inverse_transforms(self, rows: torch.Tensor) -> torch.Tensor:
        """inverse(T) [..., 4, 4] of table rows [..., 9]."""
        R = rotation_6d(rows[..., 3:] + self.identity)
        Rt = R.transpose(-1, -2)
        top = torch.cat([Rt, -(Rt @ rows[..., :3, None])], dim=-1)
        bottom = torch.zeros_like(top[..., :1, :])
        bottom[..., 3] = 1.0
        return torch.cat([top, bottom], dim=-2)

    def apply(self, viewmat: torch.Tensor, v: int) -> torch.Tensor:
        """The view matrix [4, 4] of view v's camera after its correction, in the table's dtype; the identity at a zero row."""
        return self.inverse_transforms(self.table[v]) @ viewmat.to(self.table.dtype)

    def apply_all(self, viewmats: torch.Tensor) -> torch.Tensor:
        """apply() for all V views at once: [V, 4, 4]."""
        return self.inverse_transforms(self.table) @ viewmats.to(self.table.dtype)


def check_pose_options(fn: str, n_views: int, pose_opt, pose_opt_lr, pose_opt_reg, pose_noise) -> bool:
    """True when fn()'s pose keywords ask for anything; raises GwbpError for a value that is negative, not finite or no number, and for
    pose_opt or pose_noise without a view."""
    if not isinstance(pose_opt, bool):
        raise GwbpError(f"{fn}(): pose_opt must be a bool, got {pose_opt!r}")
    for name, value in (("pose_opt_lr", pose_opt_lr), ("pose_opt_reg", pose_opt_reg), ("pose_noise", pose_noise)):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(float(value)) or float(value) < 0.0:
            raise GwbpError(f"{fn}(): {name} must be a finite number >= 0, got {value!r}")
    active = pose_opt or float(pose_noise) > 0.0
    if active and n_views < 1:
        raise GwbpError(f"{fn}(): pose_opt and pose_noise need at least one view")
    return active


class PoseTraining:
    """What train.train_scene(pose_opt=..., pose_noise=...) keeps beside its loop: the fixed perturbation (pose_noise > 0: a PoseAdjust drawn
    once from `seed` with std = pose_noise, the reference's pose_perturb), the learnt correction behind it (pose_opt: a zero PoseAdjust
    whose table is a leaf of its own torch.optim.Adam(lr=pose_opt_lr, weight_decay=pose_opt_reg); step s of `steps` runs at
    pose_opt_lr * 0.01 ** (s / steps), the reference's ExponentialLR), and the monitor.  dtype: float32 as train_scene runs it; a
    float64 yardstick of the same loop passes torch.float64."""

    def __init__(self, viewmats: torch.Tensor, steps: int, seed: int, pose_opt: bool, pose_opt_lr: float, pose_opt_reg: float,
                 pose_noise: float, dtype=torch.float32):
        n_views, dev = int(viewmats.shape[0]), viewmats.device
        self.viewmats, self.steps, self.lr0 = viewmats.detach().to(dtype), max(int(steps), 1), float(pose_opt_lr)
        self.noise = PoseAdjust(n_views, dev, dtype).random_init(float(pose_noise), seed) if float(pose_noise) > 0.0 else None
        self.adjust = self.opt = None
        if pose_opt:
            self.adjust = PoseAdjust(n_views, dev, dtype)
            self.adjust.table.requires_grad_(True)
            self.opt = torch.optim.Adam([self.adjust.table], lr=self.lr0, weight_decay=float(pose_opt_reg))
        # the perturbed views are fixed: computed once; the true camera-to-world matrices are the monitor's other side
        self.noisy = self.viewmats if self.noise is None else self.noise.apply_all(self.viewmats)
        self.c2w_true = rigid_inverse(self.viewmats) if self.noise is not None else None
        self.errors = []

    def view(self, v: int) -> torch.Tensor:
        """The view matrix step renders view v with; under pose_opt attached to the table, whose gradient is cleared here."""
        if self.adjust is None:
            return self.noisy[v]
        self.opt.zero_grad(set_to_none=True)
        return self.adjust.apply(self.noisy[v], v)

    def all_views(self) -> torch.Tensor:
        with torch.no_grad():
            return self.noisy if self.adjust is None else self.adjust.apply_all(self.noisy)

    def step(self, step: int) -> None:
        """Behind the backward of step `step`: the monitor's value, then the optimiser's step at the step's rate."""
        if self.c2w_true is not None:
            self.errors.append((self.c2w_true - rigid_inverse(self.all_views())).abs().mean())
        if self.opt is not None:
            self.opt.param_groups[0]["lr"] = self.lr0 * 0.01 ** (step / self.steps)
            self.opt.step()

    def history(self) -> dict:
        """pose_err (under pose_noise: per step, the mean absolute difference between the true and the used camera-to-world matrices
        over all views, as the reference monitors it, read from the device once here), pose_adjust [V, 9] (under pose_opt) and viewmats
        [V, 4, 4], the views as they ended."""
        out = dict(viewmats=self.all_views())
        if self.adjust is not None:
            out["pose_adjust"] = self.adjust.table.detach().clone()
        if self.c2w_true is not None:
            out["pose_err"] = torch.stack(self.errors).cpu().tolist() if self.errors else []
        return out


def pose_loss(out: torch.Tensor, target: torch.Tensor, weights: Optional[torch.Tensor], loss: str,
              ssim_lambda: float = 0.2) -> torch.Tensor:
    """The refiner's loss of a render [H, W, D] against its target: "l2": the (weighted) mean over pixels of the squared distance,
    "cosine": of one minus the cosine of the two D-vectors, "photometric": photometric.photometric_loss, the trainer's
    (1 - ssim_lambda) L1 + ssim_lambda (1 - SSIM) from the fused kernels (device tensors only)."""
    if loss == "photometric":
        from .photometric import photometric_loss
        return photometric_loss(out, target, ssim_lambda=ssim_lambda, weights=weights)
    if loss == "l2":
        per = ((out - target) ** 2).sum(dim=-1)
    elif loss == "cosine":
        per = 1.0 - torch.nn.functional.cosine_similarity(out, target, dim=-1, eps=1e-8)
    else:
        raise ValueError(f"loss must be l2, cosine or photometric, got {loss!r}")
    if weights is None:
        return per.mean()
    return (per * weights).sum() / weights.sum().clamp_min(1e-12)


def optimize_twist(value_of, viewmat0: torch.Tensor, steps: int, lr: float):
    """Adam on a twist in front of viewmat0 (float64, on its device): value_of(viewmat [4, 4] float64) is the differentiable loss.
    Returns dict(viewmat float64, twist, history); history[k] is the loss before the update of step k."""
    vm0 = viewmat0.detach().double()
    twist = torch.zeros(6, dtype=torch.float64, device=vm0.device, requires_grad=True)
    opt = torch.optim.Adam([twist], lr=lr)
    history = []
    for _ in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        value = value_of(se3_exp(twist) @ vm0)
        value.backward()
        opt.step()
        history.append(float(value.detach()))
    with torch.no_grad():
        viewmat = se3_exp(twist) @ vm0
    return dict(viewmat=viewmat, twist=twist.detach().clone(), history=history)


def refine_pose(means, quats, scales, opacities, table, target, viewmat0, K, width, height, *, steps: int = 100, lr: float = 5e-3,
                weights=None, loss: str = "l2", camera_model: str = "pinhole", rasterize_mode: str = "classic", eps2d: float = 0.3,
                ssim_lambda: float = 0.2):
    """Refine a camera pose against `target` [H, W, D], the image or feature map seen from the unknown pose: Adam on the six numbers
    of a twist, viewmat = se3_exp(twist) @ viewmat0, one rasterization(camera_grad=True) of `table` [N, D] (float32, D <= 32) per step.
    weights [H, W] or None weighs the pixels.  Returns dict(viewmat [4, 4] float32, twist [6] float64, history: the loss of each step,
    taken before that step's update).  The Gaussians and the table are detached.  loss: "l2", "cosine" or "photometric" (pose_loss;
    ssim_lambda belongs to the last)."""
    if table.dim() != 2 or table.shape[1] > GEOMETRY_GRAD_MAX_DIM or table.dtype != torch.float32:
        raise ValueError(f"table must be float32 [N, D] with D <= {GEOMETRY_GRAD_MAX_DIM}, got {table.dtype} {tuple(table.shape)}")
    width, height = int(width), int(height)
    if tuple(target.shape) != (height, width, table.shape[1]):
        raise ValueError(f"target has shape {tuple(target.shape)}, expected {(height, width, table.shape[1])}")
    if weights is not None and tuple(weights.shape) != (height, width):
        raise ValueError(f"weights has shape {tuple(weights.shape)}, expected {(height, width)}")
    dev = means.device
    gauss = [t.detach() for t in (means, quats, scales, opacities, table)]
    target = target.detach().to(dev, torch.float32)
    weights = None if weights is None else weights.detach().to(dev, torch.float32)
    vm0 = viewmat0.detach().to(dev, torch.float64)
    Ks = K.detach().to(dev, torch.float32)[None]

    def value_of(vm):
        out, _, _ = rasterization(*gauss, vm.float()[None], Ks, width, height, eps2d=eps2d, camera_model=camera_model,
                                  rasterize_mode=rasterize_mode, want_meta=False, camera_grad=True)
        return pose_loss(out[0], target, weights, loss, ssim_lambda)

    res = optimize_twist(value_of, vm0, steps, lr)
    res["viewmat"] = res["viewmat"].float()
    return res
