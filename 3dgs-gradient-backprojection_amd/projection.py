"""The projection kernel and the SH colour kernel restated in differentiable torch ops.

`rasterization()` differentiates the per-pixel blend with a HIP kernel (gwbp_render_pixels_backward), which leaves the gradient with
respect to each projected record: 2-D mean, conic, opacity.  The chain rule from there back to means / quats / scales / opacities and
the view matrix is N-sized and a second HIP kernel (gwbp_project_backward, csrc/project_grad.h).  `project_torch` is the function that
kernel differentiates, and what the tests measure it against with torch autograd: k_project's arithmetic (csrc/project.hip) for the
three camera models and both rasterize modes, operation by operation where that matters for the FUNCTION (the pinhole clamp of x/z and
y/z inside the Jacobian, the eps2d low-pass, the antialiasing compensation), not for the bits.  It never decides what is visible: the
rows the kernel kept (`radii > 0`) come in as `visible`, every other row is zero and takes no gradient.

`sh_colors_torch` is k_sh_colors (csrc/render.hip) the same way: same basis constants, "+0.5", clamp at 0.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch

CLAMP_MARGIN = 0.3  # kClampMargin: x/z clamp margin in tan_fov units
FISHEYE_EPS = 1e-7


def _rotations(quats: torch.Tensor) -> torch.Tensor:
    """[n,4] (w, x, y, z), any norm -> [n,3,3]."""
    q = quats / quats.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def _camera(model: str, pc: torch.Tensor, fx, fy, cx, cy, W: int, H: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(u, v, J [n,2,3]) of camera-space points under gsplat's ideal camera models."""
    x, y, z = pc.unbind(1)
    zero = torch.zeros_like(x)
    if model == "ortho":
        one = torch.ones_like(x)
        J = torch.stack([fx * one, zero, zero, zero, fy * one, zero], dim=1)
        return fx * x + cx, fy * y + cy, J.reshape(-1, 2, 3)
    if model == "fisheye":
        eps = FISHEYE_EPS
        rho = torch.sqrt(x * x + y * y) + eps
        theta = torch.atan2(rho, z + eps)
        xx, yy, xy = x * x + eps, y * y, x * y
        r2 = xx + yy
        iR2 = 1.0 / (r2 + z * z)
        a, b = z * iR2 / r2, theta / rho / r2
        J = torch.stack([fx * (xx * a + yy * b), fx * xy * (a - b), -(fx * x * iR2),
                         fy * xy * (a - b), fy * (yy * a + xx * b), -(fy * y * iR2)], dim=1)
        s = theta / rho
        return fx * (x * s) + cx, fy * (y * s) + cy, J.reshape(-1, 2, 3)
    if model != "pinhole":
        raise ValueError(f"camera_model must be pinhole, ortho or fisheye, got {model!r}")
    tan_x, tan_y = 0.5 * W / fx, 0.5 * H / fy
    lim_xp, lim_xn = (W - cx) / fx + CLAMP_MARGIN * tan_x, cx / fx + CLAMP_MARGIN * tan_x
    lim_yp, lim_yn = (H - cy) / fy + CLAMP_MARGIN * tan_y, cy / fy + CLAMP_MARGIN * tan_y
    rz = 1.0 / z
    # torch.clamp: a clamped x/z passes no gradient to the Jacobian, as in gsplat; the mean itself uses the unclamped ratio
    txc = z * torch.clamp(x * rz, min=-lim_xn, max=lim_xp)
    tyc = z * torch.clamp(y * rz, min=-lim_yn, max=lim_yp)
    J = torch.stack([fx * rz, zero, -(fx * txc * rz * rz), zero, fy * rz, -(fy * tyc * rz * rz)], dim=1)
    return fx * (x * rz) + cx, fy * (y * rz) + cy, J.reshape(-1, 2, 3)


def project_torch(means: torch.Tensor, quats: torch.Tensor, scales: torch.Tensor, opacities: torch.Tensor, viewmat: torch.Tensor,
                  K: torch.Tensor, W: int, H: int, eps2d: float = 0.3, camera_model: str = "pinhole",
                  rasterize_mode: str = "classic", visible: Optional[torch.Tensor] = None):
    """(means2d [N,2], conics [N,3], opac_eff [N]) of one view: what k_project files for the blend, as a differentiable function of
    means [N,3], quats [N,4], scales [N,3], opacities [N] in their own dtype.  opac_eff is the opacity times the antialiasing
    compensation sqrt(max(0, det(S) / det(S + eps2d I))) under rasterize_mode="antialiased", the opacity itself otherwise.
    visible (bool [N], the kernel's radii > 0; None: every row): rows outside it are zero and take no gradient.  No culling
    decision is made here."""
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError(f"rasterize_mode must be classic or antialiased, got {rasterize_mode!r}")
    n = means.shape[0]
    dt, dev = means.dtype, means.device
    idx = None
    if visible is not None:
        idx = torch.nonzero(visible.to(dev))[:, 0]
        means, quats, scales, opacities = (t.index_select(0, idx) for t in (means, quats, scales, opacities))
    # (a view matrix that requires grad stays attached: the yardstick of the camera gradient differentiates it)
    vm, Km = (viewmat if viewmat.requires_grad else viewmat.detach()).to(dev, dt), K.detach().to(dev, dt)
    R, t = vm[:3, :3], vm[:3, 3]
    fx, fy, cx, cy = Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2]
    pc = means @ R.T + t
    M = _rotations(quats) * scales[:, None, :]
    cov_cam = R @ (M @ M.transpose(1, 2)) @ R.T
    u, v, J = _camera(camera_model, pc, fx, fy, cx, cy, int(W), int(H))
    S2 = J @ cov_cam @ J.transpose(1, 2)
    c00, c01, c11 = S2[:, 0, 0], S2[:, 0, 1], S2[:, 1, 1]
    det_orig = c00 * c11 - c01 * c01
    c00, c11 = c00 + eps2d, c11 + eps2d
    det = c00 * c11 - c01 * c01
    opac = opacities
    if rasterize_mode == "antialiased":
        ratio = det_orig / det
        pos = ratio > 0
        comp = torch.where(pos, torch.sqrt(torch.where(pos, ratio, torch.ones_like(ratio))), torch.zeros_like(ratio))
        opac = opacities * comp
    means2d = torch.stack([u, v], dim=1)
    conics = torch.stack([c11 / det, -c01 / det, c00 / det], dim=1)
    if idx is None:
        return means2d, conics, opac
    return (means2d.new_zeros(n, 2).index_copy(0, idx, means2d), conics.new_zeros(n, 3).index_copy(0, idx, conics),
            opac.new_zeros(n).index_copy(0, idx, opac))


# the real SH basis every 3DGS code base uses (k_sh_colors' constants)
_C0 = 0.28209479177387814
_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
_C3 = (0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 1.445305721320277)


def sh_colors_torch(degree: int, means: torch.Tensor, coeffs: torch.Tensor,
                    campos: Union[torch.Tensor, Sequence[float]]) -> torch.Tensor:
    """[N,K,3] SH coefficients (K >= (degree + 1)^2, degree <= 3) -> [N,3] colours toward `campos`: + 0.5, clamped at 0, differentiable
    in the coefficients and, through the view direction, in means."""
    if not 0 <= degree <= 3 or coeffs.dim() != 3 or coeffs.shape[2] != 3 or coeffs.shape[1] < (degree + 1) ** 2:
        raise ValueError(f"bad SH arguments (degree={degree}, coefficients {tuple(coeffs.shape)})")
    cp = torch.as_tensor(campos, dtype=means.dtype, device=means.device)
    d = means - cp
    d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)
    x, y, z = d.unbind(1)
    b = [torch.full_like(x, _C0)]
    if degree >= 1:
        b += [-_C1 * y, _C1 * z, -_C1 * x]
    if degree >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [_C2[0] * xy, -_C2[0] * yz, _C2[1] * (2 * zz - xx - yy), -_C2[0] * xz, _C2[2] * (xx - yy)]
        if degree >= 3:
            b += [-_C3[0] * y * (3 * xx - yy), _C3[1] * xy * z, -_C3[2] * y * (4 * zz - xx - yy),
                  _C3[3] * z * (2 * zz - 3 * xx - 3 * yy), -_C3[2] * x * (4 * zz - xx - yy), _C3[4] * z * (xx - yy),
                  -_C3[0] * x * (xx - 3 * yy)]
    basis = torch.stack(b, dim=1)  # [N, (degree + 1)^2]
    rgb = (basis[:, :, None] * coeffs[:, :basis.shape[1], :]).sum(dim=1)
    return (rgb + 0.5).clamp_min(0.0)
