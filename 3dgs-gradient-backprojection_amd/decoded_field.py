"""A latent feature field and its decoder, fitted on frozen Gaussians (the reference's comparison baseline,
f3dgs/simple_trainer_feature_3dgs.py: every Gaussian carries a d-channel latent, a [d, D] decoder `conv` turns a rendered latent
image into the D-channel feature map, and both are trained with F.l1_loss(render(features) @ conv, feature_map)).

    loss = decoded_loss(render, conv, feature_map)                # replaces F.l1_loss(render @ conv, feature_map) in that trainer
    out  = decoded_field_gradients(means, quats, scales, opacities, latents, conv, feature_map, viewmat, K, W, H)
    latents, conv, history = fit_decoded_field(means, quats, scales, opacities, viewmats, K, W, H, feature_fn, dim)
    field = decode_field(latents, conv)                           # [N, D] for prompt_mask, fit_pca, score_field_views

Written literally, render @ conv, the difference, its sign and the gradient image are [H, W, D] tensors each.  Here one call of
gwbp_decode_loss (csrc/decode_loss.hip) yields the loss and both gradients and makes none of them; the gradient of the latent table
then flows through the scatter kernel that rasterization()'s backward already uses.  The scene stays frozen: nothing here
differentiates with respect to means, quats, scales or opacities.  There is no PyTorch fallback for the first-order path: CPU
tensors raise, and so does a missing library.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

from ._lib import GwbpError
from ._views import front, require_device
from ._views import raster_kw as merged_raster_kw
from .polish import view_schedule
from .rasterization import PIXEL_RENDER_MAX_DIM, engine_on, get_engine

REDUCTIONS = ("mean", "sum")


def _literal(rendered, decoder, target, loss, pixel_weights, reduction):
    """The definitions of Engine.decode_loss in plain torch, with history: what a second-order use differentiates."""
    y = rendered @ decoder
    m = target.to(y.dtype)
    good = torch.isfinite(m).all(dim=-1, keepdim=True)
    e = torch.where(good, y - torch.where(good, m, torch.zeros_like(m)), torch.zeros_like(y))
    t = e.abs() if loss == "l1" else e * e
    if pixel_weights is not None:
        t = t * pixel_weights.to(y.dtype)[..., None]
    return t.mean() if reduction == "mean" else t.sum()


class _DecodedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rendered, decoder, target, loss, pixel_weights, reduction):
        h, w, _ = rendered.shape
        scale = 1.0 / max(1, h * w * decoder.shape[1]) if reduction == "mean" else 1.0
        value, g_rendered, g_decoder, _ = engine_on(rendered.device).decode_loss(
            rendered.detach(), decoder.detach(), target, loss=loss, scale=scale, pixel_weights=pixel_weights)
        ctx.save_for_backward(rendered, decoder, target, g_rendered, g_decoder)
        ctx.args = (loss, pixel_weights, reduction)
        return value.to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        rendered, decoder, target, g_rendered, g_decoder = ctx.saved_tensors
        if torch.is_grad_enabled():
            # backward(create_graph=True): the literal expression's gradients, with their history
            with torch.enable_grad():
                lit = _literal(rendered, decoder, target, *ctx.args)
                wanted = [t for t, need in zip((rendered, decoder), ctx.needs_input_grad[:2]) if need]
                grads = list(torch.autograd.grad(lit, wanted, grad_outputs=g, create_graph=True))
            out = [grads.pop(0) if need else None for need in ctx.needs_input_grad[:2]]
            return out[0], out[1], None, None, None, None
        return (g_rendered * g if ctx.needs_input_grad[0] else None, g_decoder * g if ctx.needs_input_grad[1] else None,
                None, None, None, None)


def decoded_loss(rendered, decoder, target, loss: str = "l1", pixel_weights: Optional[torch.Tensor] = None,
                 reduction: str = "mean") -> torch.Tensor:
    """F.l1_loss(rendered @ decoder, target) (loss="l1") or F.mse_loss (loss="l2") without the [H, W, D] tensors: a float32
    scalar whose backward hands d/d(rendered) and d/d(decoder) out -- both come from the forward's one gwbp_decode_loss call.
    rendered: float32 [H, W, d], or the [1, H, W, d] batch rasterization() returns for one camera; d % 16 == 0, 16 <= d <= 128.
    decoder: float32 [d, D], D % 16 == 0, 16 <= D <= 2048.  target: the view's [H, W, D] map, float32 / float16 / bfloat16 read as
    stored (unit channel stride); it receives no gradient.  pixel_weights: optional [H, W] weights c_p (bool, uint8, float16,
    bfloat16, float32): every term of pixel p is multiplied by c_p.  reduction: "mean" divides by H W D, "sum" does not.
    A pixel whose target row holds a non-finite value adds nothing to the loss or the gradients.
    backward(create_graph=True) differentiates the literal torch expression instead (second order: [H, W, D] tensors)."""
    if loss not in ("l1", "l2"):
        raise GwbpError(f"loss must be 'l1' or 'l2', got {loss!r}")
    if reduction not in REDUCTIONS:
        raise GwbpError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    if not torch.is_tensor(rendered) or not rendered.is_cuda:
        raise GwbpError("decoded_loss() needs HIP tensors (there is no CPU path)")
    if rendered.dim() == 4:
        if rendered.shape[0] != 1:
            raise GwbpError(f"a batch of {rendered.shape[0]} cameras: call decoded_loss() once per view")
        rendered = rendered[0]
    if torch.is_tensor(target) and target.requires_grad:
        raise GwbpError("the target map receives no gradient: detach it")
    return _DecodedLoss.apply(rendered, decoder, target, loss, pixel_weights, reduction)


def decoded_field_gradients(means, quats, scales, opacities, latents, decoder, feature_map, viewmat, K, width, height,
                            loss: str = "l1", pixel_weights: Optional[torch.Tensor] = None, reduction: str = "mean",
                            **raster_kw) -> Dict[str, torch.Tensor]:
    """One view of the fit without autograd: front stage, render of `latents` [N, d], gwbp_decode_loss (its gradient image
    written over the render), and the scatter of that image into grad_latents.  Returns {"loss": float64 0-d, "grad_latents":
    float32 [N, d], "grad_decoder": float32 [d, D], "table": float64 [8] = loss, n_pixels, n_bad, P, d, D, 0, 0}: the values
    decoded_loss(rasterization(..., latents, ...)[0], decoder, feature_map).backward() leaves in latents.grad and decoder.grad.
    The engine and the front cache are rasterization()'s.  raster_kw: near_plane, far_plane, eps2d, radius_clip, camera_model,
    rasterize_mode."""
    if reduction not in REDUCTIONS:
        raise GwbpError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    require_device("decoded_field_gradients", means)
    if not torch.is_tensor(latents) or latents.dim() != 2 or latents.shape[0] != means.shape[0] or latents.dtype != torch.float32:
        raise GwbpError(f"latents must be float32 [N, d] with N = {means.shape[0]}")
    kw = merged_raster_kw("decoded_field_gradients", raster_kw)
    width, height = int(width), int(height)
    n, d = latents.shape
    # d <= 128: the 128-channel scatter kernel, as rasterization()'s backward picks it (the flag must be in place before the blend)
    get_engine(means.device, n, width, height).set_narrow_scatter(True)
    eng, view, _ = front("decoded_field_gradients", means, quats, scales, opacities, viewmat, K, width, height, kw, want_store=True)
    table_in = latents.detach().contiguous()
    rendered = eng.render(view, table_in) if d > PIXEL_RENDER_MAX_DIM else eng.render_pixels(view, table_in)[0]
    scale = 1.0 / max(1, height * width * int(decoder.shape[1])) if reduction == "mean" else 1.0
    value, g_rendered, g_decoder, table = eng.decode_loss(rendered, decoder.detach(), feature_map, loss=loss, scale=scale,
                                                          pixel_weights=pixel_weights, grad_rendered=rendered)
    g_latents = torch.zeros(n, d, device=means.device)
    eng.scatter(view, g_rendered, g_latents, None)
    return dict(loss=value, grad_latents=g_latents, grad_decoder=g_decoder, table=table)


def fit_decoded_field(means, quats, scales, opacities, viewmats, K, width, height,
                      feature_fn: Callable[[int], torch.Tensor], dim: int, latent_dim: int = 128, steps: int = 1000,
                      lr: float = 2.5e-3, loss: str = "l1", init=None,
                      pixel_weight_fn: Optional[Callable[[int], Optional[torch.Tensor]]] = None, seed: int = 0,
                      callback: Optional[Callable] = None, **raster_kw):
    """Fit a [N, latent_dim] latent table and a [latent_dim, dim] decoder to the views' maps on frozen Gaussians: one view per
    step, in a shuffled order drawn per pass over the views from torch.Generator().manual_seed(seed); torch.optim.Adam on both
    tensors (the reference trains `features` and `conv` with lr 2.5e-3 each).  Returns (latents, decoder, history): float32
    device tensors and the list of the steps' losses (floats; read from the device once, behind the loop).
    feature_fn(v): the view's [H, W, dim] map as decoded_loss takes its target.  init: None -- the reference's: zero latents and
    a torch.rand decoder (drawn on the host from the same seeded generator) -- or (latents0, decoder0) to continue from.
    pixel_weight_fn(v): the view's [H, W] weights or None.  callback(step, loss, latents, decoder) runs after every step with the
    loss as a device tensor.  viewmats [V, 4, 4]; K [3, 3] or [V, 3, 3]."""
    require_device("fit_decoded_field", means)
    dev, n = means.device, means.shape[0]
    gen = torch.Generator().manual_seed(int(seed))
    if init is None:
        latents = torch.zeros(n, int(latent_dim), device=dev)
        decoder = torch.rand(int(latent_dim), int(dim), generator=gen).to(dev)
    else:
        latents, decoder = (t.detach().to(device=dev, dtype=torch.float32).clone() for t in init)
        if tuple(latents.shape) != (n, decoder.shape[0]) or decoder.shape[1] != int(dim):
            raise GwbpError(f"init must be (latents [N, d], decoder [d, {dim}]), got {tuple(latents.shape)} and "
                            f"{tuple(decoder.shape)}")
    latents.requires_grad_(True)
    decoder.requires_grad_(True)
    opt = torch.optim.Adam([latents, decoder], lr=lr)
    vm_host, k_host = viewmats.detach().cpu(), K.detach().cpu()
    losses = []
    for step, v in enumerate(view_schedule(viewmats.shape[0], gen, steps)):  # (gen: the draws follow the decoder's above)
        out = decoded_field_gradients(means, quats, scales, opacities, latents, decoder, feature_fn(v), vm_host[v],
                                      k_host if k_host.dim() == 2 else k_host[v], width, height, loss=loss,
                                      pixel_weights=pixel_weight_fn(v) if pixel_weight_fn is not None else None, **raster_kw)
        latents.grad, decoder.grad = out["grad_latents"], out["grad_decoder"]
        opt.step()
        losses.append(out["loss"])
        if callback is not None:
            callback(step, out["loss"], latents, decoder)
    history = torch.stack(losses).cpu().tolist() if losses else []
    return latents.detach(), decoder.detach(), history


def decode_field(latents: torch.Tensor, decoder: torch.Tensor) -> torch.Tensor:
    """The [N, D] field latents @ decoder, for the calls that take a finished field (prompt_mask, fit_pca, score_field_views).
    A 2-D prompt mask needs no decode: by linearity render_prompt_mask(latents, prompts @ decoder.T, ...) scores the same
    pixels."""
    if latents.dim() != 2 or decoder.dim() != 2 or latents.shape[1] != decoder.shape[0]:
        raise GwbpError(f"latents must be [N, d] and decoder [d, D], got {tuple(latents.shape)} and {tuple(decoder.shape)}")
    return latents.detach() @ decoder.detach()
