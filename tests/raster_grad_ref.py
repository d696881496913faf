"""The yardstick of the geometry gradients of rasterization(): a dense restatement of one view's render in torch, in any dtype.

Every Gaussian meets every pixel in one [H*W, N] table.  The projection is gsbp_amd.projection.project_torch in the requested dtype
(pinned against the CPU checker's projection and tests/ref_camera_np.py by tests/test_raster_grad_cpu.py); the Gaussians are ordered
as the front stage orders them, by the float32 depth bits and then by index; WHICH (pixel, Gaussian) pairs count is never decided
here: the bool mask comes from the kernels (kernel_cut: project + bin_sort + blend_weights + dump_pairs) -- or, in the CPU self-test,
from a fixed rule -- so that no cut (alpha >= 1/255, sigma >= 0, T <= 1e-4 termination, visibility) is re-decided in another
precision.  On the mask

    alpha = min(0.999, o exp(-sigma)),  T = exclusive cumulative product of (1 - alpha) along the sorted axis,
    out = sum alpha T c,  alpha_img = 1 - T_end

and torch autograd of  sum(out G) + sum(alpha_img A)  gives all five gradients.  The float64 run is the truth; the float32 run of the
same code against it is the noise floor the kernel path is measured in.

rasterize() adds what rasterization() wraps around the render -- the SH colours, the depth column, the ED division, the background --
with the same torch expressions, so that a test compares like with like.
"""
import numpy as np
import torch

from gsbp_amd.projection import project_torch, sh_colors_torch

ALPHA_MAX = 0.999
NAMES = ("means", "quats", "scales", "opacities", "colors")


def depth_order(depths, visible):
    """The front stage's order of the Gaussians: ascending float32 depth BITS, ties by index, what the projection culled last."""
    bits = torch.as_tensor(depths, dtype=torch.float32).contiguous().view(torch.int32).to(torch.int64)
    bits = torch.where(torch.as_tensor(visible), bits, torch.full_like(bits, 1 << 40))
    return torch.argsort(bits, stable=True)


def pairs_mask(gid, pix, n_pixels, n_gaussians):
    """bool [H*W, N] of the (pixel, Gaussian) pairs a dump of the weight store lists."""
    mask = torch.zeros(n_pixels, n_gaussians, dtype=torch.bool)
    mask[torch.as_tensor(pix).long().cpu(), torch.as_tensor(gid).long().cpu()] = True
    return mask


def kernel_cut(dev, means, quats, scales, opacities, viewmat, K, W, H, **view_kw):
    """What the kernels decide for one view: dict(mask bool [H*W, N], order int64 [N], visible bool [N]), all on the CPU."""
    import gsbp_amd
    n = means.shape[0]
    eng = gsbp_amd.Engine(n, W, H, device=dev)
    view = eng.view(viewmat, K, W, H, **view_kw)
    g = [t.detach().to(dev, torch.float32).contiguous() for t in (means, quats, scales, opacities)]
    while True:
        proj = eng.project(view, *g, want_outputs=True)
        eng.bin_sort(view)
        eng.blend_weights(view)
        st = eng.stats()
        if not st["overflow"]:
            break
        eng.grow(st)
    gid, pix, _ = eng.dump_pairs(view)
    visible = (proj["radii"] > 0).cpu()
    return dict(mask=pairs_mask(gid, pix, W * H, n), order=depth_order(proj["depths"].cpu(), visible), visible=visible)


def render(means, quats, scales, opacities, colors, viewmat, K, W, H, cut, eps2d=0.3, camera_model="pinhole",
           rasterize_mode="classic"):
    """(out [H,W,D], alpha_img [H,W], raw [H*W,N]) in the dtype of means; raw = o exp(-sigma) before the clamp, zero outside the
    mask, in the sorted order (for a test that wants to know how far its pairs are from the clamp)."""
    dt = means.dtype
    m2d, con, oe = project_torch(means, quats, scales, opacities, viewmat, K, W, H, eps2d, camera_model, rasterize_mode,
                                 cut["visible"])
    order, mask = cut["order"], cut["mask"][:, cut["order"]]
    m2d, con, oe, colors = m2d[order], con[order], oe[order], colors[order]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    px, py = xs.reshape(-1, 1) + 0.5, ys.reshape(-1, 1) + 0.5
    dx, dy = m2d[None, :, 0] - px, m2d[None, :, 1] - py
    sigma = 0.5 * (con[None, :, 0] * dx * dx + con[None, :, 2] * dy * dy) + con[None, :, 1] * dx * dy
    sigma = torch.where(mask, sigma, torch.zeros_like(sigma))  # (no exp of what the mask drops: inf * 0 in its gradient)
    raw = torch.where(mask, oe[None, :] * torch.exp(-sigma), torch.zeros_like(sigma))
    alpha = torch.clamp(raw, max=ALPHA_MAX)
    t_incl = torch.cumprod(1.0 - alpha, dim=1)
    t_excl = torch.cat([torch.ones_like(t_incl[:, :1]), t_incl[:, :-1]], dim=1)
    out = (alpha * t_excl) @ colors
    return out.reshape(H, W, -1), (1.0 - t_incl[:, -1]).reshape(H, W), raw


def rasterize(means, quats, scales, opacities, colors, viewmat, K, W, H, cut, eps2d=0.3, camera_model="pinhole",
              rasterize_mode="classic", render_mode="RGB", background=None, sh_degree=None, campos=None):
    """rasterization()'s (render_colors [H,W,D'], render_alphas [H,W]) of one camera, its wrappers included; returns raw as well."""
    dt = means.dtype
    vm = viewmat.to(dt)
    cols = colors if sh_degree is None else sh_colors_torch(sh_degree, means, colors, campos)
    if "D" in render_mode:
        z = (means @ vm[:3, :3].T + vm[:3, 3])[:, 2:3]
        cols = z if render_mode in ("D", "ED") else torch.cat([cols, z], dim=1)
    out, alpha, raw = render(means, quats, scales, opacities, cols, viewmat, K, W, H, cut, eps2d, camera_model, rasterize_mode)
    if render_mode in ("ED", "RGB+ED"):
        out = torch.cat([out[..., :-1], out[..., -1:] / alpha[..., None].clamp_min(1e-10)], dim=-1)
    if background is not None:
        out = out + (1.0 - alpha[..., None]) * background.to(dt)
    return out, alpha, raw


def gradients(dtype, inputs, G, A, viewmat, K, W, H, cut, **kw):
    """The five gradients (NAMES' order) of sum(out G) + sum(alpha_img A) in `dtype`, the loss and raw; inputs: the five float32 CPU
    tensors, G [H,W,D'] and A [H,W] the seeded weights."""
    ins = [t.detach().cpu().to(dtype).requires_grad_(True) for t in inputs]
    out, alpha, raw = rasterize(*ins, viewmat.cpu(), K.cpu(), W, H, cut, **kw)
    loss = (out * G.cpu().to(dtype)).sum() + (alpha * A.cpu().to(dtype)).sum()
    grads = torch.autograd.grad(loss, ins, allow_unused=True)  # (render_mode "D" / "ED" does not read the colours: zeros)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(grads, ins)], loss.detach(), raw.detach()


def errors(got, truth):
    """(Frobenius-relative error, max-abs error relative to the truth's max-abs) of one gradient tensor, in float64."""
    got, truth = got.detach().cpu().double(), truth.detach().cpu().double()
    diff = got - truth
    fro, top = float(truth.norm()), float(truth.abs().max())
    if top == 0.0:  # nothing to be relative to: any difference at all is an error of 1
        bad = float(diff.abs().max()) > 0.0
        return float(bad), float(bad)
    return float(diff.norm()) / fro, float(diff.abs().max()) / top


def report(name, kernel_grads, truth, floor32):
    """One dict per gradient tensor: the float32 restatement's error (the floor) and the kernel path's, both against float64."""
    rows = []
    for n, k, t, f in zip(NAMES, kernel_grads, truth, floor32):
        (ffro, ftop), (kfro, ktop) = errors(f, t), errors(k, t)
        rows.append(dict(case=name, tensor=n, floor_fro=ffro, floor_max=ftop, kernel_fro=kfro, kernel_max=ktop))
    return rows


def np_f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))
