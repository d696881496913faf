"""render_latents: one view's render of a latent table of up to 128 channels, differentiable in the Gaussians AND in the table.

rasterization() offers geometry gradients beside tables of at most 32 channels (its blend backward keeps a pixel's channels twice in
registers) and refuses them beside wider ones; that stays.  A Feature-3DGS step renders a [N, 128] latent table next to the colours and its
loss reaches means, quats, scales and opacities through that render as well.  This operator is that second render:

Forward  = project -> bin/sort -> blend_weights (the weight store) -> render (d > 16) or render_pixels
Backward = gwbp_render_dots_backward (v_g2d: the channels enter through one dot product per pair)
           -> gwbp_project_backward (means, quats, scales, opacities)
           and gwbp_scatter of the incoming gradient over the weight store (latents).

camera_grad=True also returns the view matrix's gradient from the same gwbp_project_backward call (the blend depends on the view only
through the projection).  Not offered here: gradients w.r.t. K, means2d_grad, half tables, backgrounds.
"""
from __future__ import annotations

import torch

from ._lib import GwbpError
from .rasterization import PIXEL_RENDER_MAX_DIM, get_engine, run_front

LATENT_MAX_DIM = 128  # gwbp_render_dots_backward holds a pixel's v_out row in registers


class _RenderLatents(torch.autograd.Function):
    @staticmethod
    def forward(ctx, latents, means, quats, scales, opacities, viewmat, K, width, height, kw, camera_grad):
        eng = get_engine(means.device, means.shape[0], width, height)
        view = eng.view(viewmat, K, width, height, **kw)
        eng.set_narrow_scatter(True)
        wide = latents.shape[1] > PIXEL_RENDER_MAX_DIM
        _, _, alphas, _ = run_front(eng, view, means, quats, scales, opacities, wide, False, want_store=True)
        if wide:
            out = eng.render(view, latents.detach())
        else:
            out, alphas = eng.render_pixels(view, latents.detach())
        ctx.eng, ctx.view, ctx.gen, ctx.camera_grad = eng, view, eng.generation, camera_grad
        ctx.save_for_backward(latents, means, quats, scales, opacities)
        return out, alphas

    @staticmethod
    def backward(ctx, g_out, g_alpha):
        needs = ctx.needs_input_grad
        want_viewmat = bool(ctx.camera_grad and needs[5])
        if (needs[5] and not want_viewmat) or needs[6]:
            raise NotImplementedError("render_latents differentiates latents, means, quats, scales and opacities, viewmat under "
                                      "camera_grad=True, not K")
        eng, view = ctx.eng, ctx.view
        latents, means, quats, scales, opacities = ctx.saved_tensors
        if eng.generation != ctx.gen or eng.n != means.shape[0]:
            # the workspace was reused by another call since forward: rebuild this view's lists and weight store
            eng = get_engine(means.device, means.shape[0], view.width, view.height)
            eng.set_narrow_scatter(True)
            eng.front_cache = None
            run_front(eng, view, means, quats, scales, opacities, False, False, want_store=True)
        if g_out is None:
            g_out = torch.zeros(view.height, view.width, latents.shape[1], device=means.device)
        g_out = g_out.detach().contiguous()
        v_latents = None
        if needs[0]:
            v_latents = torch.zeros(latents.shape, device=means.device, dtype=torch.float32)
            eng.scatter(view, g_out, v_latents, None)
        grads = (None,) * 5
        if any(needs[1:5]) or want_viewmat:
            v_g2d = eng.render_dots_backward(view, latents.detach(), g_out, g_alpha.detach() if g_alpha is not None else None)
            grads = eng.project_backward(view, means.detach(), quats.detach(), scales.detach(), opacities.detach(), v_g2d,
                                         needs=needs[1:5], want_viewmat=want_viewmat)
        v_viewmat = grads[4].to(torch.float32) if want_viewmat else None
        return (v_latents, *grads[:4], v_viewmat, None, None, None, None, None)


def render_latents(means, quats, scales, opacities, latents, viewmat, K, width, height, near_plane: float = 0.01,
                   far_plane: float = 1e10, radius_clip: float = 0.0, eps2d: float = 0.3, rasterize_mode: str = "classic",
                   camera_model: str = "pinhole", camera_grad: bool = False):
    """(render [H, W, d], alpha [H, W]) of one view of the float32 table latents [N, d], d <= 128, with gradients w.r.t. means [N, 3],
    quats [N, 4], scales [N, 3], opacities [N] and latents.  viewmat [4, 4], K [3, 3]; the keywords are rasterization()'s and mean the
    same.  The gradients of the four Gaussian tensors use float atomics and are not bit-reproducible from run to run.
    camera_grad=True: a viewmat that requires grad also receives its gradient, float32 [4, 4] with a zero bottom row, summed by
    Engine.project_backward(want_viewmat=True) in a fixed order; without the keyword such a viewmat is refused in the backward."""
    for t, name in ((means, "means"), (quats, "quats"), (scales, "scales"), (opacities, "opacities"), (latents, "latents")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise GwbpError(f"render_latents needs HIP tensors, {name} is not one (there is no CPU path)")
    if latents.dtype != torch.float32:
        raise GwbpError(f"latents must be float32, got {latents.dtype} (half latent tables are not differentiated)")
    if latents.dim() != 2 or latents.shape[0] != means.shape[0] or not 1 <= latents.shape[1] <= LATENT_MAX_DIM:
        raise GwbpError(f"latents must be [N, d] with N = {means.shape[0]} and 1 <= d <= {LATENT_MAX_DIM}, got {tuple(latents.shape)}")
    kw = dict(near_plane=near_plane, far_plane=far_plane, eps2d=eps2d, radius_clip=radius_clip, camera_model=camera_model,
              rasterize_mode=rasterize_mode)
    return _RenderLatents.apply(latents.contiguous(), means, quats, scales, opacities, viewmat, K, int(width), int(height), kw,
                                bool(camera_grad))
