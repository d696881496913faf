"""Depth supervision of training (csrc/depth_loss.hip, csrc/depth_math.h).

    out, alphas, _ = rasterization(..., render_mode="RGB+D")          # the accumulated depth in the last channel
    loss = depth_point_loss(out[0], alphas[0], points, depths)         # the reference trainer's depth_loss: mean |1 / d - 1 / depths|
    loss = depth_map_loss(out[0], alphas[0], depth_map, kind="depth")  # or against a depth map (RGB-D, monocular depth)

Both are torch.autograd.Functions over one HIP kernel forward and one backward, differentiable with respect to the render and the
alpha map; the expected depth render[..., channel] / max(alpha, 1e-10) is formed inside the kernels, per sample, so no ED render, no
copy of the depth channel and no image-sized temporary exist.  There is no torch fallback: CPU tensors raise GwbpError.

Coordinates.  A point (x, y) is in the reference's coordinates, those of grid_sample(align_corners=True) over x / (W - 1) * 2 - 1:
x is a column INDEX, column j is sampled at x = j.  That is half a pixel off the rasteriser's pixel centres (pixel j covers
[j, j + 1) and is evaluated at j + 0.5); the reference trains with it, so it is kept.

Two departures from the reference's torch expression, both where it gives NaN: a sample whose depth is not positive (an empty pixel)
contributes 1 / depths to the loss and EXACT ZEROS to the gradient, and no points at all (or no valid pixel) give loss 0 and zero
gradients.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib
from ._lib import GwbpError
from .engine import depth_image_args, depth_map_args, depth_point_args
from .rasterization import engine_on

__all__ = ["depth_point_loss", "depth_map_loss", "sample_expected_depth"]
DEPTH_KINDS = tuple(_lib.DEPTH_KINDS)  # train_scene(depth_kind=...): depth_map_loss's kinds


def _scale(fn: str, scale) -> float:
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise GwbpError(f"{fn}: scale must be a number, got {scale!r}")
    return float(scale)


class _DepthPointLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, render, alpha, points, depths, channel, scale):
        loss, _ = engine_on(render.device).depth_points_loss(render.detach(), alpha.detach(), points, depths, channel, scale)
        ctx.save_for_backward(render, alpha, points, depths)
        ctx.args = (channel, scale)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        render, alpha, points, depths = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None, None, None
        channel, scale = ctx.args
        v_render, v_alpha = engine_on(render.device).depth_points_backward(render, alpha, points, depths, g, channel, scale)
        return (v_render if ctx.needs_input_grad[0] else None, v_alpha.reshape(alpha.shape) if ctx.needs_input_grad[1] else None,
                None, None, None, None)


class _DepthMapLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, render, alpha, depth, weights, kind, channel, scale):
        loss, sums = engine_on(render.device).depth_map_loss(render.detach(), alpha.detach(), depth, weights, kind, channel, scale)
        ctx.save_for_backward(render, alpha, depth, sums, *(() if weights is None else (weights,)))
        ctx.args = (kind, channel, scale)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        render, alpha, depth, sums, *rest = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None, None, None, None
        kind, channel, scale = ctx.args
        v_render, v_alpha = engine_on(render.device).depth_map_backward(render, alpha, depth, sums, g, rest[0] if rest else None, kind,
                                                                        channel, scale)
        return (v_render if ctx.needs_input_grad[0] else None, v_alpha.reshape(alpha.shape) if ctx.needs_input_grad[1] else None,
                None, None, None, None, None)


def depth_point_loss(render, alpha, points, depths, channel: int = -1, scale: float = 1.0) -> torch.Tensor:
    """scale * mean_i |1 / d_i - 1 / depths_i|, the reference trainer's depth term, as a float32 0-dim device tensor whose backward
    reaches `render` and `alpha`.  render: float32 [H, W, D'] of an accumulated-depth mode (RGB+D, D), its depth in `channel`; alpha:
    [H, W] or [H, W, 1]; points: float32 [M, 2], (x, y) as column and row indices (see the module's note); depths: float32 [M], the
    points' true depths.  d_i is the bilinear sample, with zero padding, of render[..., channel] / max(alpha, 1e-10).
    The loss is summed in float64 in a fixed order (the same bits every call); the backward adds with float atomics where points
    share a pixel and is not bit-reproducible.  d_i <= 0: 1 / depths_i in the loss, exact zeros in the gradient.  M = 0: 0.
    Non-finite inputs and depths <= 0 are not masked."""
    fn = "depth_point_loss"
    depth_image_args(fn, render, alpha, channel)
    depth_point_args(fn, render, points, depths)
    if points.requires_grad or depths.requires_grad:
        raise GwbpError(f"{fn}: points and depths receive no gradient: detach them")
    return _DepthPointLoss.apply(render, alpha, points, depths, channel, _scale(fn, scale))


def depth_map_loss(render, alpha, depth, weights: Optional[torch.Tensor] = None, kind: str = "disparity", channel: int = -1,
                   scale: float = 1.0) -> torch.Tensor:
    """scale * sum w t / sum w over the valid pixels -- depth > 0, and weights > 0 where weights are given -- of the expected depth
    e = render[..., channel] / max(alpha, 1e-10) against the float32 [H, W] map `depth`: t = |1 / e - 1 / depth| (kind "disparity",
    1 / e read as 0 where e <= 0) or |e - depth| (kind "depth").  A float32 0-dim device tensor whose backward reaches `render` and
    `alpha`; no atomics, forward and backward give the same bits every call.  No valid pixel: 0 and zero gradients.  A pixel with
    e <= 0 takes a zero gradient."""
    fn = "depth_map_loss"
    depth_image_args(fn, render, alpha, channel)
    depth_map_args(fn, render, depth, weights, kind)
    if depth.requires_grad or (weights is not None and weights.requires_grad):
        raise GwbpError(f"{fn}: the depth map and the weights receive no gradient: detach them")
    return _DepthMapLoss.apply(render, alpha, depth, weights, kind, channel, _scale(fn, scale))


def sample_expected_depth(render, alpha, points, channel: int = -1) -> torch.Tensor:
    """The samples d_i [M] depth_point_loss compares, under the same bilinear rule and by the same kernel (its per-point output): what
    a caller who makes depth points from a render of its own uses (run_train.py --synthetic --depth-loss)."""
    fn = "sample_expected_depth"
    with torch.no_grad():
        ones = torch.ones(points.shape[0], device=points.device) if torch.is_tensor(points) and points.dim() == 2 else None
        depth_image_args(fn, render, alpha, channel)
        depth_point_args(fn, render, points, ones)
        _, per_point = engine_on(render.device).depth_points_loss(render, alpha, points, ones, channel, 1.0, want_per_point=True)
    return per_point[:, 0].contiguous()


def check_depth_options(fn: str, depth_fn, depth_lambda, depth_scale, depth_kind, raster_kw) -> dict:
    """The keywords fn()'s colour render takes under its depth keywords, {} without a depth_fn whatever the others are; GwbpError for a
    depth_fn that is no callable, a render_mode among raster_kw, an unknown kind, a value that is not finite or no number."""
    if depth_fn is None:
        return {}
    if not callable(depth_fn):
        raise GwbpError(f"{fn}(): depth_fn must be a callable of the view's index, got {type(depth_fn).__name__}")
    if "render_mode" in raster_kw:
        raise GwbpError(f"{fn}(depth_fn=...) renders with render_mode='RGB+D': leave render_mode out of the raster keywords")
    if depth_kind not in DEPTH_KINDS:
        raise GwbpError(f"{fn}(): depth_kind must be one of {list(DEPTH_KINDS)}, got {depth_kind!r}")
    for name, value in (("depth_lambda", depth_lambda), ("depth_scale", depth_scale)):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(float(value)):
            raise GwbpError(f"{fn}(): {name} must be a finite number, got {value!r}")
    return dict(render_mode="RGB+D", return_alpha=True)


def depth_term(image, alpha, target, kind: str, scale: float, v: int) -> torch.Tensor:
    """View v's depth loss against target = depth_fn(v): a (points, depths) pair, an [H, W] map, or None (no supervision: a device 0)."""
    if target is None:
        return torch.zeros((), device=image.device)
    if isinstance(target, (tuple, list)) and len(target) == 2:
        return depth_point_loss(image, alpha, target[0], target[1], scale=float(scale))
    if torch.is_tensor(target):
        return depth_map_loss(image, alpha, target, kind=kind, scale=float(scale))
    raise GwbpError(f"depth_fn({v}) must return a (points, depths) pair, an [H, W] tensor or None, got {type(target).__name__}")
