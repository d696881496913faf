"""What a training loop over a splat dict is made of, and the trainer's evaluation without LPIPS.  The loops themselves -- polish_scene
on a FIXED set of Gaussians, train_scene with a strategy's rounds -- are train.py; this is the layer below them, below densify.py and
mcmc.py, and what a loop written elsewhere imports:

    PARAM_KEYS, DEFAULT_LRS                      the trainer's parameter names, their keys in a splat dict and their learning rates
    work, opt = trainable(splats, params, lrs, "my_loop")          # detached leaves, one Adam group each
    for step, v in enumerate(view_schedule(n_views, seed, steps)):  # the seeded view of each step
        image = render_splats(work, viewmats[v], view_K(K, v), W, H, sh_degree=scheduled_sh_degree(step, interval, table_sh_degree(work)))
    splat_geometry, means_group, means_lr_at     the activations, the means' Adam group and its decayed rate
    check_sh_degree_interval, check_adam, check_means_lr_final, means_lr_decay     the loops' keyword checks
    table = score_image_views(splats, viewmats, K, W, H, image_fn)      # per view: psnr, ssim, l1, mse

A render is rasterization() (whose backward is the HIP blend and projection backward) on the SH colours of sh.sh_colors.  A splat dict
carries the reference's key names (means, scaling, rotation, opacity, features_dc [N, 1, 3], features_rest [N, K - 1, 3]),
pre-activation; the parameters go by the trainer's names.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Sequence

import torch

from ._lib import GwbpError
from .photometric import image_metrics
from .projection import sh_colors_torch
from .rasterization import SH_CAMERA_GRAD_MESSAGE, rasterization, sh_kernel_enabled
from .sh import sh_colors

# the trainer's name of a parameter -> its key in a splat dict (pre-activation: scales are logs, opacities logits)
PARAM_KEYS = {"means": "means", "scales": "scaling", "quats": "rotation", "opacities": "opacity", "sh0": "features_dc",
              "shN": "features_rest"}
# the reference trainer's learning rates (its means rate is further multiplied by the scene's scale there; here it is not)
DEFAULT_LRS = {"means": 1.6e-4, "scales": 5e-3, "quats": 1e-3, "opacities": 5e-2, "sh0": 2.5e-3, "shN": 2.5e-3 / 20}


def table_sh_degree(splats: Dict[str, torch.Tensor]) -> int:
    """The SH degree the coefficient count of features_dc and features_rest gives."""
    k = splats["features_dc"].shape[1] + (splats["features_rest"].shape[1] if "features_rest" in splats else 0)
    degree = int(round(math.sqrt(k))) - 1
    if (degree + 1) ** 2 != k:
        raise GwbpError(f"{k} SH coefficients per Gaussian are no full degree")
    return degree


def scheduled_sh_degree(step: int, interval: Optional[int], table_degree: int) -> Optional[int]:
    """The reference trainer's sh_degree_to_use of step `step`: min(step // interval, the table's degree); None without an interval."""
    return None if interval is None else min(step // interval, table_degree)


def check_sh_degree_interval(interval, fn: str) -> Optional[int]:
    if interval is None:
        return None
    if isinstance(interval, bool) or not isinstance(interval, int) or interval < 1:
        raise GwbpError(f"{fn}(): sh_degree_interval must be None or a positive int, got {interval!r}")
    return interval


def splat_geometry(splats: Dict[str, torch.Tensor]):
    """(means, quats, scales, opacities) as the trainer renders them: scales = exp, opacities = sigmoid, raw quats."""
    return (splats["means"], splats["rotation"], torch.exp(splats["scaling"]), torch.sigmoid(splats["opacity"]))


def render_splats(splats: Dict[str, torch.Tensor], viewmat, K, width: int, height: int, return_meta: bool = False,
                  sh_degree: Optional[int] = None, geometry=None, return_alpha: bool = False, pose_grad: bool = False, **raster_kw):
    """The [H, W, 3] image of a splat dict from one camera, as the trainer renders it: scales = exp, opacities = sigmoid, raw quats,
    the SH colours of features_dc and features_rest.  Differentiable in every tensor of the dict.
    sh_degree: the degree to evaluate, at most the one the tables' coefficient count gives (None: that one).  Below it the rows above
    (sh_degree + 1)^2 are not read, and their gradients are zeros, not None.
    The colours come from sh.sh_colors on the two tables as they are stored (no torch.cat, one HIP kernel forward and one backward) and
    go to rasterization() as an [N, 3] table; camera_grad=True is refused as rasterization() refuses it beside sh_degree.
    pose_grad=True with a viewmat that requires grad also differentiates the view matrix: the SH centre -(R^T t) is computed in torch on
    the device and stays attached, sh_colors(campos_grad=True) carries the colour gradient to it, and the table goes to
    rasterization(camera_grad=True); the view matrix is not read on the host for the colours.  Under torch.no_grad() or with a viewmat
    that does not require grad it is the plain call.
    return_meta: (image, meta) -- the eager part of rasterization()'s meta, which under means2d_grad=True holds the means2d leaf.
    geometry: splat_geometry(splats) computed by the caller, who hands the same activations to a second render (train_scene's
    feature term); None computes them here.
    return_alpha: also hand back the [H, W, 1] alpha map of the same render, behind the image: (image, alpha) or (image, alpha, meta).
    With render_mode="RGB+D" in raster_kw the image is [H, W, 4], the accumulated depth last (what depth.depth_point_loss takes)."""
    table = table_sh_degree(splats)
    degree = table if sh_degree is None else sh_degree
    if isinstance(degree, bool) or not isinstance(degree, int) or not 0 <= degree <= table:
        raise GwbpError(f"sh_degree must be an int in [0, {table}] (the tables' degree), got {sh_degree!r}")
    means, dc, rest = splats["means"], splats["features_dc"], splats.get("features_rest")
    if raster_kw.get("camera_grad") and not pose_grad and torch.is_grad_enabled() and viewmat.requires_grad:
        raise NotImplementedError(SH_CAMERA_GRAD_MESSAGE)
    geometry = splat_geometry(splats) if geometry is None else geometry
    if pose_grad and torch.is_grad_enabled() and viewmat.requires_grad:
        if not means.is_cuda:
            raise GwbpError("render_splats(pose_grad=True) needs HIP tensors (there is no CPU path)")
        campos = -(viewmat[:3, :3].T @ viewmat[:3, 3])  # on the device, attached: no host read of the view matrix
        if sh_kernel_enabled():
            colors = sh_colors(degree, means, dc, campos.float(), rest=rest, campos_grad=True)
        else:  # (set_sh_kernel(False): the torch form with the same attached centre, the other side of a timing)
            colors = sh_colors_torch(degree, means, dc if rest is None else torch.cat([dc, rest], dim=1), campos)
        out, alphas, meta = rasterization(*geometry, colors, viewmat[None], K[None], width, height, sh_degree=None, want_meta=False,
                                          **dict(raster_kw, camera_grad=True))
        return _render_result(out, alphas, meta, return_alpha, return_meta)
    if not sh_kernel_enabled() or not means.is_cuda:  # (set_sh_kernel(False): the route before the kernels; CPU tensors: its error)
        sh = dc if rest is None else torch.cat([dc, rest], dim=1)
        out, alphas, meta = rasterization(*geometry, sh, viewmat[None], K[None], width, height, sh_degree=degree, want_meta=False, **raster_kw)
        return _render_result(out, alphas, meta, return_alpha, return_meta)
    vm_h = viewmat.detach().cpu()  # the camera centre as rasterization() computes it beside sh_degree
    colors = sh_colors(degree, means, dc, (-(vm_h[:3, :3].T @ vm_h[:3, 3])).tolist(), rest=rest)
    out, alphas, meta = rasterization(*geometry, colors, viewmat[None], K[None], width, height, sh_degree=None, want_meta=False, **raster_kw)
    return _render_result(out, alphas, meta, return_alpha, return_meta)


def _render_result(out, alphas, meta, return_alpha: bool, return_meta: bool):
    if not return_alpha:  # (the returns before the keyword existed)
        return (out[0], meta) if return_meta else out[0]
    return (out[0], alphas[0], meta) if return_meta else (out[0], alphas[0])


def view_K(K, v):
    return K if K.dim() == 2 else K[v]


ADAM_KINDS = ("torch", "fused", "visible")


def check_adam(adam, fn: str) -> str:
    if adam not in ADAM_KINDS:
        raise GwbpError(f"{fn}(): adam must be one of {list(ADAM_KINDS)}, got {adam!r}")
    return adam


def check_means_lr_final(value, fn: str) -> Optional[float]:
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (0.0 < float(value) and math.isfinite(float(value))):
        raise GwbpError(f"{fn}(): means_lr_final must be None or a positive finite number, got {value!r}")
    return float(value)


def means_lr_at(lr0: float, final: float, step: int, steps: int) -> float:
    """The means group's learning rate of step `step` (from 0) of `steps`: lr0 * final ** (step / steps), the reference trainer's
    exponential decay (its final is 0.01), in closed form on the host."""
    return float(lr0) * float(final) ** (step / steps)


def means_group(opt, work: Dict[str, torch.Tensor]):
    """The optimiser's group that holds work["means"], or None when the means are not trained."""
    return next((g for g in opt.param_groups if g["params"][0] is work["means"]), None)


def means_lr_decay(opt, work: Dict[str, torch.Tensor], final: Optional[float], fn: str):
    """What fn(means_lr_final=final) decays: (the means' group, its first rate, final); None without the keyword."""
    group = means_group(opt, work) if final is not None else None
    if final is not None and group is None:
        raise GwbpError(f"{fn}(): means_lr_final decays the means group's rate, and the means are not among params")
    return None if group is None else (group, group["lr"], final)


def trainable(splats: Dict[str, torch.Tensor], params: Sequence[str], lrs: Optional[Dict[str, float]], fn: str, adam: str = "torch"):
    """(work, optimizer) of fn(): `splats` detached, each named parameter a float32 leaf of its own, and torch.optim.Adam with ONE
    tensor per group at lrs[name] over DEFAULT_LRS, eps 1e-15 as in the reference trainer (densify._relocate_adam relies on that layout).
    adam: "torch" is that optimiser; "fused" and "visible" build adam.SplatAdam over the same groups (one HIP kernel per tensor; the
    caller of "visible" hands step() the view's radii)."""
    check_adam(adam, fn)
    unknown = [p for p in params if p not in PARAM_KEYS]
    if unknown or not params:
        raise GwbpError(f"params must be names out of {sorted(PARAM_KEYS)}, got {list(params)}")
    if not splats["means"].is_cuda:
        raise GwbpError(f"{fn}() needs HIP tensors (there is no CPU path)")
    if "features_dc" not in splats:
        raise GwbpError(f"the splat dict has no features_dc: {fn}() renders SH colours")
    rates = dict(DEFAULT_LRS, **(lrs or {}))
    work = {k: (t.detach() if torch.is_tensor(t) else t) for k, t in splats.items()}
    groups = []
    for name in params:
        key = PARAM_KEYS[name]
        if key not in work:
            raise GwbpError(f"the splat dict has no {key!r} (parameter {name!r})")
        work[key] = work[key].float().clone().requires_grad_(True)
        groups.append(dict(params=[work[key]], lr=float(rates[name])))
    if adam != "torch":
        from .adam import SplatAdam
        return work, SplatAdam(groups, eps=1e-15)
    return work, torch.optim.Adam(groups, eps=1e-15)


def view_schedule(n_views: int, seed: int, steps: int):
    """The view of each step: a fresh permutation per pass over the views, drawn on the host from `seed` (an int or the caller's generator)."""
    gen = seed if isinstance(seed, torch.Generator) else torch.Generator().manual_seed(int(seed))
    order = []
    for _ in range(int(steps)):
        if not order:
            order = torch.randperm(n_views, generator=gen).tolist()
        yield order.pop(0)


def score_image_views(splats: Dict[str, torch.Tensor], viewmats, K, width, height, image_fn: Callable[[int], torch.Tensor],
                      **raster_kw) -> Dict:
    """The reference's evaluation without LPIPS: every view rendered and compared with its image.  Returns {"views": [{"view": v,
    "psnr", "ssim", "l1", "mse"}, ...], "mean": the same four averaged over the views}."""
    rows = []
    with torch.no_grad():
        for v in range(viewmats.shape[0]):
            image = render_splats(splats, viewmats[v], view_K(K, v), int(width), int(height), **raster_kw)
            rows.append(dict(view=v, **image_metrics(image.clamp(0.0, 1.0), image_fn(v))))
    keys = ("psnr", "ssim", "l1", "mse")
    return dict(views=rows, mean={k: sum(r[k] for r in rows) / len(rows) for k in keys} if rows else {})
