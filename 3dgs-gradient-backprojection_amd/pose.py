"""The camera side of a lifted scene: where was this image, or this feature map, taken from?

`rasterization(camera_grad=True)` differentiates a render with respect to its view matrix (gwbp_project_backward sums the projection's
gradient over the Gaussians; the depth column of the "D" render modes adds its own through torch).  On top of that:

    se3_exp(twist)            the rigid motion of a 6-vector (rotation vector, then translation), differentiable, exact at zero
    pose_error(vm_a, vm_b)    (angle in radians, distance of the camera centres) between two world-to-camera matrices
    refine_pose(...)          Adam on the six numbers of a twist applied in front of an initial view matrix, against a target image
                              or feature map of at most 32 channels

The Gaussians are fixed; only the camera moves.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

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
