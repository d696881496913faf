"""The photometric loss 3DGS scenes are trained with, and the two metrics they are scored with, fused (csrc/ssim.hip):

    loss = photometric_loss(render, image)        # (1 - ssim_lambda) F.l1_loss(render, image) + ssim_lambda (1 - SSIM(image, render))
    m    = image_metrics(render, image)           # psnr, ssim, l1, mse
    smap = ssim_map(render, image)                # [H', W', D], the SSIM of every window and channel
    g    = gaussian_window()                      # the 11 float32 taps

SSIM is the 11-tap Gaussian-window form (sigma 1.5, C1 = 0.01^2, C2 = 0.03^2, data range 1) computed per channel.  Written in torch it
is five 11 x 11 depthwise convolutions forward, as many backward and a dozen image-sized temporaries; here one call runs a forward
kernel, a reduce and a backward kernel and moves about eleven image-sized reads and writes in total.

padding="valid" (the default) averages the windows wholly inside the image, H, W >= 11; as far as we know that is what torchmetrics'
StructuralSimilarityIndexMeasure(data_range=1.0), which the reference trainer uses, computes with its defaults (it reflect-pads and
crops the padded border off the map) -- the library was not at hand to check, so the formula of DESIGN.md 4 is the contract, not the
library.  padding="same" covers all H W windows with zeros outside the image, as the fused-ssim kernels of CUDA trainers do.

Non-finite inputs are not masked: they propagate into the sums, the loss and the gradient.  There is no PyTorch fallback for the
first-order path: CPU tensors raise GwbpError, and so does a missing library.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import GwbpError
from .rasterization import engine_on

SSIM_TILE = _lib.SSIM_TILE  # (GWBP_SSIM_TILE_Y, GWBP_SSIM_TILE_X): the pixels of one workgroup's tile
SSIM_WINDOW, SSIM_SIGMA = 11, 1.5
SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2
PADDINGS = tuple(_lib.SSIM_PADDINGS)


def gaussian_window() -> torch.Tensor:
    """The window: g[i] = exp(-(i - 5)^2 / (2 1.5^2)), i = 0 .. 10, normalised to sum 1 in float64 and rounded to float32 once
    (csrc/ssim_math.h holds the same 11 numbers as constants)."""
    i = torch.arange(SSIM_WINDOW, dtype=torch.float64)
    g = torch.exp(-(i - SSIM_WINDOW // 2) ** 2 / (2 * SSIM_SIGMA ** 2))
    return (g / g.sum()).float()


def _pair(fn: str, a, b):
    if not torch.is_tensor(a) or not torch.is_tensor(b) or not a.is_cuda or not b.is_cuda:
        raise GwbpError(f"{fn}() needs HIP tensors (there is no CPU path)")
    if a.dim() != 3 or a.shape != b.shape:
        raise GwbpError(f"{fn}() takes two [H, W, D] images of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise GwbpError(f"{fn}() takes float32 images, got {a.dtype} and {b.dtype}")
    return a.detach(), b.detach()


def ssim_map(a, b, padding: str = "valid") -> torch.Tensor:
    """The SSIM of every window and channel of two float32 [H, W, D] images: [H - 10, W - 10, D] ("valid") or [H, W, D] ("same")."""
    a, b = _pair("ssim_map", a, b)
    return engine_on(a.device).image_loss(a, b, 0.0, padding, want_map=True)[1]


def image_sums(a, b, weights=None, padding: str = "valid") -> torch.Tensor:
    """The float64 [8] table of the pair on the device: sum w ssim over windows and channels, sum w |a - b|, sum w (a - b)^2 over
    elements, Wv = sum of w over windows, Wa = sum of w over pixels, the number of windows, H W, D.  weights: optional [H, W]."""
    a, b = _pair("image_sums", a, b)
    return engine_on(a.device).image_loss(a, b, 0.0, padding, pixel_weights=weights)[0]


def _ratio(num, den):
    """num / den, 0 where den == 0 (a term whose weight sum is zero contributes nothing), on the device."""
    return torch.where(den != 0, num / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(num))


def table_loss(table: torch.Tensor, ssim_lambda: float) -> torch.Tensor:
    """loss = (1 - lambda) sum w |x - y| / (D Wa) + lambda (1 - sum w ssim / (D Wv)) of a table, float64 0-d, no host read."""
    D = table[7]
    l1 = _ratio(table[1], D * table[4])
    ss = torch.where(table[3] != 0, 1.0 - _ratio(table[0], D * table[3]), torch.zeros_like(l1))
    return (1.0 - float(ssim_lambda)) * l1 + float(ssim_lambda) * ss


def image_metrics(a, b, weights=None, padding: str = "valid") -> Dict[str, float]:
    """The reference's evaluation of a render `a` against its image `b` (without LPIPS): psnr = -10 log10(mse), ssim = the mean of
    the SSIM map, l1 and mse the means over the elements -- weighted means with `weights`.  Returns floats (one host read)."""
    t = image_sums(a, b, weights, padding).cpu().tolist()
    D = t[7]
    mse = t[2] / (D * t[4]) if t[4] != 0 else 0.0
    return dict(psnr=-10.0 * math.log10(mse) if mse > 0 else math.inf, ssim=t[0] / (D * t[3]) if t[3] != 0 else 0.0,
                l1=t[1] / (D * t[4]) if t[4] != 0 else 0.0, mse=mse)


def _blur(v, g):
    p = torch.nn.functional.pad(v, (0, 0, 5, 5))
    h = sum(g[i] * p[:, i:i + v.shape[1]] for i in range(SSIM_WINDOW))
    p = torch.nn.functional.pad(h, (0, 0, 0, 0, 5, 5))
    return sum(g[j] * p[j:j + v.shape[0]] for j in range(SSIM_WINDOW))


def _literal(x, y, ssim_lambda, padding, weights):
    """The definition in plain torch, with history: what a second-order use differentiates."""
    H, W, D = x.shape
    g = gaussian_window().to(x.device)
    c1, c2 = torch.tensor(SSIM_C1).float().item(), torch.tensor(SSIM_C2).float().item()
    mu1, mu2 = _blur(x, g), _blur(y, g)
    s1, s2, s12 = _blur(x * x, g) - mu1 * mu1, _blur(y * y, g) - mu2 * mu2, _blur(x * y, g) - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    w = torch.ones(H, W, device=x.device) if weights is None else weights.to(x.dtype)
    wv = w
    if padding == "valid":
        wv = torch.zeros_like(w)
        wv[5:H - 5, 5:W - 5] = w[5:H - 5, 5:W - 5]
    l1 = _ratio((w[..., None] * (x - y).abs()).sum(), D * w.sum())
    ss = torch.where(wv.sum() != 0, 1.0 - _ratio((wv[..., None] * ssim).sum(), D * wv.sum()), torch.zeros_like(l1))
    return (1.0 - ssim_lambda) * l1 + ssim_lambda * ss


class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, render, target, ssim_lambda, padding, weights):
        table, _, grad = engine_on(render.device).image_loss(render.detach(), target, ssim_lambda, padding, pixel_weights=weights,
                                                             want_grad=True)
        ctx.save_for_backward(render, target, grad)
        ctx.args = (ssim_lambda, padding, weights)
        return table_loss(table, ssim_lambda).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        render, target, grad = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        if torch.is_grad_enabled():
            # backward(create_graph=True): the literal expression's gradient, with its history
            with torch.enable_grad():
                lit = _literal(render, target, *ctx.args)
                return torch.autograd.grad(lit, render, grad_outputs=g, create_graph=True)[0], None, None, None, None
        return grad * g, None, None, None, None


def photometric_loss(render, target, ssim_lambda: float = 0.2, padding: str = "valid", weights: Optional[torch.Tensor] = None):
    """(1 - ssim_lambda) F.l1_loss(render, target) + ssim_lambda (1 - SSIM(target, render)), the loss of the reference trainer, as a
    float32 scalar whose backward hands d / d(render) out: the forward's one gwbp_image_loss call also produced it.
    render: float32 [H, W, D], 1 <= D <= 32, or the [C, H, W, D] batch rasterization() returns -- then one call per image and the
    mean.  A slice `out[..., :3]` of a wider render goes in without a copy.  target: the same shape; it receives no gradient.
    weights: optional [H, W] (or [C, H, W]) pixel weights: both terms become weighted means (a window counts with the weight of
    its centre); a term whose weights sum to zero contributes 0.  padding: "valid" (H, W >= 11) or "same".
    backward(create_graph=True) differentiates the literal torch expression instead."""
    if padding not in PADDINGS:
        raise GwbpError(f"padding must be one of {PADDINGS}, got {padding!r}")
    if not torch.is_tensor(render) or not torch.is_tensor(target) or not render.is_cuda or not target.is_cuda:
        raise GwbpError("photometric_loss() needs HIP tensors (there is no CPU path)")
    if render.shape != target.shape or render.dim() not in (3, 4):
        raise GwbpError(f"render and target must be [H, W, D] or [C, H, W, D] of one shape, got {tuple(render.shape)} and "
                        f"{tuple(target.shape)}")
    if target.requires_grad:
        raise GwbpError("the target receives no gradient: detach it")
    lam = float(ssim_lambda)
    if render.dim() == 3:
        return _PhotometricLoss.apply(render, target, lam, padding, weights)
    if render.shape[0] < 1:
        raise GwbpError("an empty batch has no loss")
    if weights is not None and weights.dim() != 3:
        raise GwbpError(f"a batch takes [C, H, W] weights, got {tuple(weights.shape)}")
    per = [_PhotometricLoss.apply(render[i], target[i], lam, padding, None if weights is None else weights[i])
           for i in range(render.shape[0])]
    return torch.stack(per).mean()
