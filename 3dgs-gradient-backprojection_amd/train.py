"""The training loops: Adam on the pre-activation tensors of a splat dict under the photometric loss the reference trainer uses
(f3dgs/simple_trainer_feature_3dgs.py: (1 - 0.2) L1 + 0.2 (1 - SSIM)), on a fixed set of Gaussians or on one that grows and shrinks.

    splats, losses = polish_scene(splats, viewmats, K, W, H, image_fn, params=("opacities", "sh0"), steps=300)
    splats, history = train_scene(splats, viewmats, K, W, H, image_fn, steps=7000, cfg=DensifyConfig())
    splats, history = train_scene(splats, viewmats, K, W, H, image_fn, steps=30000, strategy=MCMCConfig(), opacity_reg=0.01, scale_reg=0.01)

polish_scene re-fits a scene whose N is fixed (the opacities after apply_mask3d took Gaussians away, a touch-up before a lift);
train_scene is the trainer: the SH schedule, the feature, depth and pose terms, and a strategy.  Both run one loop (_run) over one step
(_step).  What a strategy does at a step is its rounds object, densify.DensifyRounds or mcmc.MCMCRounds: means2d_grad (does the colour
render report means2d.grad), after_backward(meta, step), and after_step(work, opt, carried, step) -> (work, carried) behind the
optimiser's step; a fixed set is no rounds object.  The pieces of a step are polish.py's; depth.py and pose.py check their own keywords.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from ._lib import GwbpError
from .decoded_field import decoded_loss
from .densify import GEOMETRY_KEYS, DensifyConfig, DensifyRounds
from .depth import check_depth_options, depth_term
from .latent_render import render_latents
from .mcmc import MCMCConfig, MCMCRounds
from .photometric import photometric_loss
from .polish import (PARAM_KEYS, check_adam, check_means_lr_final, check_sh_degree_interval, means_lr_at, means_lr_decay,
                     render_splats, scheduled_sh_degree, splat_geometry, table_sh_degree, trainable, view_K, view_schedule)
from .pose import PoseTraining, check_pose_options

LATENT_RENDER_KW = ("near_plane", "far_plane", "radius_clip", "eps2d", "rasterize_mode", "camera_model")  # render_latents' keywords


def _step(work: Dict[str, torch.Tensor], opt, step: int, v: int, *, viewmats, K, width, height, image_fn, steps, ssim_lambda, adam, render_kw,
          table_degree, interval=None, decay=None, rounds=None, poses=None, depth=None, feature=None, opacity_reg=0.0, scale_reg=0.0) -> Dict:
    """Step `step` on view v: render, loss, backward, the strategy's look at the gradients, the optimisers.  What a call's steps share
    comes by keyword: render_kw is the colour render's (means2d_grad, the depth and pose modes, the caller's own); interval is
    sh_degree_interval; decay is None or (the means' group, its first rate, means_lr_final) -- a round swaps a group's leaf, never the
    group --; rounds is the strategy's rounds object, None on a fixed set; depth is None or (depth_fn, depth_lambda, depth_scale,
    depth_kind); feature is None or (feature_fn, feature_weight, feature_loss, decoder, the decoder's Adam, render_latents' keywords).
    Returns the step's entries of the history, detached: loss, n, sh_degree and, where the term is on, means_lr, depth_loss,
    feature_loss.  Nothing of the graph, of meta or of the render outlives the call: a round behind it finds the old workspace free."""
    opt.zero_grad(set_to_none=True)
    degree = table_degree if interval is None else scheduled_sh_degree(step, interval, table_degree)
    record = dict(sh_degree=degree)
    geometry = splat_geometry(work) if feature is not None else None  # (one exp and one sigmoid for both renders)
    viewmat = viewmats[v] if poses is None else poses.view(v)
    image, *alpha, meta = render_splats(work, viewmat, view_K(K, v), width, height, return_meta=True,
                                        sh_degree=None if interval is None else degree, geometry=geometry, **render_kw)
    loss = photometric_loss(image[..., :3] if depth is not None else image, image_fn(v), ssim_lambda=ssim_lambda)
    if depth is not None:
        depth_fn, depth_lambda, depth_scale, depth_kind = depth
        d_loss = depth_term(image, alpha[0], depth_fn(v), depth_kind, depth_scale, v)
        record["depth_loss"] = d_loss.detach()
        loss = loss + float(depth_lambda) * d_loss
    if feature is not None:
        feature_fn, feature_weight, feature_loss, decoder, opt_dec, latent_kw = feature
        opt_dec.zero_grad(set_to_none=True)
        latent_map, _ = render_latents(*geometry, work["features"], viewmat, view_K(K, v), width, height, **latent_kw)
        f_loss = decoded_loss(latent_map, decoder, feature_fn(v), loss=feature_loss)
        record["feature_loss"] = f_loss.detach()
        loss = loss + float(feature_weight) * f_loss
    if opacity_reg != 0.0:
        loss = loss + opacity_reg * torch.sigmoid(work["opacity"]).mean()
    if scale_reg != 0.0:
        loss = loss + scale_reg * torch.exp(work["scaling"]).mean()
    loss.backward()
    if rounds is not None:
        rounds.after_backward(meta, step)
    if decay is not None:
        group, lr0, final = decay
        group["lr"] = record["means_lr"] = means_lr_at(lr0, final, step, int(steps))
    if adam == "visible":
        opt.step(visible=meta["radii"])
    else:
        opt.step()
    if feature is not None:
        opt_dec.step()
    if poses is not None:
        poses.step(step)
    record.update(loss=loss.detach(), n=int(work["means"].shape[0]))
    return record


def _run(work: Dict[str, torch.Tensor], opt, carried: Dict[str, torch.Tensor], seed, **shared):
    """The loop over _step(**shared): (work, history) with history = loss, n, rounds, resets, carry, sh_degree and means_lr, depth_loss,
    feature_loss where the term is on.  A step's view comes from the seeded schedule; the losses are read once behind the loop."""
    rounds = shared.get("rounds")
    history = dict(loss=[], n=[], rounds=[] if rounds is None else rounds.rounds, resets=[] if rounds is None else rounds.resets,
                   carry=None, sh_degree=[])
    history.update({key: [] for key, term in (("means_lr", "decay"), ("depth_loss", "depth"), ("feature_loss", "feature"))
                    if shared.get(term) is not None})
    for step, v in enumerate(view_schedule(shared["viewmats"].shape[0], seed, shared["steps"])):
        for key, value in _step(work, opt, step, v, **shared).items():
            history[key].append(value)
        if rounds is not None:
            work, carried = rounds.after_step(work, opt, carried, step)
    history["carry"] = carried
    for key in ("loss", "depth_loss", "feature_loss"):
        if key in history:
            history[key] = torch.stack(history[key]).cpu().tolist() if history[key] else []
    return {k: (t.detach() if torch.is_tensor(t) else t) for k, t in work.items()}, history


def polish_scene(splats: Dict[str, torch.Tensor], viewmats, K, width, height, image_fn: Callable[[int], torch.Tensor],
                 params: Sequence[str] = ("opacities", "sh0"), steps: int = 300, ssim_lambda: float = 0.2,
                 lrs: Optional[Dict[str, float]] = None, seed: int = 0, sh_degree_interval: Optional[int] = None,
                 adam: str = "torch", means_lr_final: Optional[float] = None,
                 **raster_kw) -> Tuple[Dict[str, torch.Tensor], List[float]]:
    """Adam on the named parameters of `splats` against the views' images.  Returns (a new splat dict -- the named tensors replaced by
    their polished values, the others shared -- and the steps' losses, read from the device once behind the loop).
    params: names out of means, scales, quats, opacities, sh0, shN; one Adam group each at lrs[name] (default: the reference
    trainer's, DEFAULT_LRS; eps 1e-15 as there).  Each step takes one view, drawn from torch.Generator().manual_seed(seed) on the
    host as a fresh permutation per pass over the views.  image_fn(v): the view's float32 [H, W, 3] image in [0, 1] on the device.
    viewmats [V, 4, 4]; K [3, 3] or [V, 3, 3].  raster_kw: camera_model, rasterize_mode and the other keywords of rasterization().
    sh_degree_interval: None renders every step at the tables' SH degree; an int renders step s (from 0) at min(s // interval, that
    degree), the reference trainer's schedule (its interval is 1000).  Coefficient rows above a step's degree get zero gradients.
    adam: "torch" steps torch.optim.Adam (the default, and the code path before the keyword existed); "fused" steps adam.SplatAdam, the
    same arithmetic in one HIP kernel per tensor; "visible" steps it on the Gaussians the step's view saw (radii > 0; the step then
    renders with means2d_grad=True, which is what reports the radii): a Gaussian the view did not see keeps every bit of its parameters
    and of both Adam moments -- the moments do not decay, and no stale momentum moves it.
    means_lr_final: None, or the factor the means group's learning rate has decayed by at the end: step s of `steps` runs with
    lr0 * means_lr_final ** (s / steps), the reference trainer's schedule (its value is 0.01); no other group's rate changes."""
    interval = check_sh_degree_interval(sh_degree_interval, "polish_scene")
    final = check_means_lr_final(means_lr_final, "polish_scene")
    work, opt = trainable(splats, params, lrs, "polish_scene", adam)
    table_degree = table_sh_degree(work)
    decay = means_lr_decay(opt, work, final, "polish_scene")
    render_kw = dict(means2d_grad=True, **raster_kw) if adam == "visible" else raster_kw  # (means2d_grad is what reports the radii)
    work, history = _run(work, opt, {}, seed, viewmats=viewmats, K=K, width=int(width), height=int(height), image_fn=image_fn, steps=steps,
                         ssim_lambda=ssim_lambda, adam=adam, render_kw=render_kw, table_degree=table_degree, interval=interval, decay=decay)
    return work, history["loss"]


def _feature_leaves(work: Dict, opt, lrs, feature_dim, latent_dim, decoder, decoder_lr, seed):
    """train_scene's feature term: (work with the float32 leaf `features` [N, latent_dim] in an Adam group of its own, the decoder
    leaf [latent_dim, feature_dim], the decoder's own Adam)."""
    n, dev = int(work["means"].shape[0]), work["means"].device
    if decoder is None:
        if feature_dim is None:
            raise GwbpError("train_scene(feature_fn=...) needs feature_dim (the channels of the maps) or a decoder")
        decoder = torch.rand(int(latent_dim), int(feature_dim), generator=torch.Generator().manual_seed(int(seed)))
    decoder = decoder.detach().to(device=dev, dtype=torch.float32).clone()
    if decoder.dim() != 2 or (feature_dim is not None and decoder.shape[1] != int(feature_dim)):
        raise GwbpError(f"decoder must be [latent_dim, {feature_dim}], got {tuple(decoder.shape)}")
    d = int(decoder.shape[0])
    feats = work.get("features")
    feats = torch.zeros(n, d, device=dev) if feats is None else feats.detach().to(device=dev, dtype=torch.float32).clone()
    if tuple(feats.shape) != (n, d):
        raise GwbpError(f"splats['features'] must be [{n}, {d}] (the decoder's rows), got {tuple(feats.shape)}")
    work = dict(work, features=feats.requires_grad_(True))
    opt.add_param_group(dict(params=[work["features"]], lr=float((lrs or {}).get("features", 2.5e-3))))
    decoder.requires_grad_(True)
    return work, decoder, torch.optim.Adam([decoder], lr=float(decoder_lr), eps=1e-15)


def train_scene(splats: Dict[str, torch.Tensor], viewmats, K, width, height, image_fn: Callable[[int], torch.Tensor], steps: int,
                cfg: Optional[DensifyConfig] = None, params: Sequence[str] = tuple(PARAM_KEYS), lrs: Optional[Dict[str, float]] = None,
                seed: int = 0, ssim_lambda: float = 0.2, carry: Optional[Dict[str, torch.Tensor]] = None, strategy=None,
                opacity_reg: float = 0.0, scale_reg: float = 0.0, sh_degree_interval: Optional[int] = None,
                feature_fn: Optional[Callable[[int], torch.Tensor]] = None, feature_dim: Optional[int] = None, latent_dim: int = 128,
                feature_weight: float = 1.0, feature_loss: str = "l1", decoder_lr: float = 2.5e-3, decoder=None, adam: str = "torch",
                means_lr_final: Optional[float] = None, depth_fn: Optional[Callable[[int], object]] = None, depth_lambda: float = 1e-2,
                depth_scale: float = 1.0, depth_kind: str = "disparity", pose_opt: bool = False, pose_opt_lr: float = 1e-5,
                pose_opt_reg: float = 1e-6, pose_noise: float = 0.0, **raster_kw):
    """polish_scene's loop with the schedule: Adam on the named parameters under the photometric loss, the set growing and shrinking
    on the way.  Step s (from 0) renders one view with means2d_grad=True, runs the backward, adds the view into the statistics while
    s < refine_stop_iter, steps the optimiser, runs a densify round when s > refine_start_iter, s % refine_every == 0 and
    s % reset_every >= pause_refine_after_reset, and resets the opacities when s > 0 and s % reset_every == 0 (both only below
    refine_stop_iter; a reset at step 0 would cap the opacities of the scene that was handed in before anything was learnt).
    Returns (the trained splat dict, history): history = dict(loss = the steps' losses, read once behind the loop; n = the number
    of Gaussians each step rendered; rounds = one dict per densify round: step, n_before, n_after, pruned, kept, cloned, split;
    resets = the steps of the opacity resets; carry = the relocated `carry` tables).
    The view of a step and the split noise come from seeded generators: the same call gives the same schedule of rounds.
    strategy: None or a DensifyConfig (the same as cfg=) runs the loop above; an mcmc.MCMCConfig runs gsplat's MCMCStrategy instead:
    no means2d gradient, no statistics and no opacity reset; after the optimiser step a relocate round and an add round when
    refine_start_iter < s < refine_stop_iter and s % refine_every == 0, and noise on the means at EVERY step, scaled by the means
    group's current learning rate (none when the means are not trained).  history["rounds"] then holds step, n_before, n_after,
    relocated, added.
    opacity_reg, scale_reg: weights of mean(sigmoid(opacity)) and mean(exp(scaling)), added to the loss when they are not zero (the
    reference's mcmc configuration sets both to 0.01).
    sh_degree_interval: None renders every step at the tables' SH degree; an int renders step s at min(s // interval, that degree), the
    reference trainer's schedule (its interval is 1000); rows above a step's degree get zero gradients.  history["sh_degree"]: the
    degree each step rendered at, one int per step.
    feature_fn(v): the view's [H, W, feature_dim] map as decoded_loss takes its target.  None: no feature term.  Set, every step renders
    twice, as the reference's Feature-3DGS trainer does: the SH colours, and render_latents of `features` [N, latent_dim] (splats["features"]
    if the dict has it, zeros otherwise: the reference's start), which `decoder` [latent_dim, feature_dim] (the caller's -- its row
    count then IS the latent dimension and the latent_dim keyword is not read -- or a torch.rand draw on the host from
    torch.Generator().manual_seed(seed)) turns into the feature map; the step's loss is the
    photometric loss + feature_weight * decoded_loss(render, decoder, feature_fn(v), loss=feature_loss), and its gradient reaches means,
    rotation, scaling and opacity as well as the latents.  exp(scaling) and sigmoid(opacity) are computed once and handed to both
    renders; of raster_kw the latent render takes the view's keywords (near_plane, far_plane, radius_clip, eps2d, rasterize_mode,
    camera_model).  The densify statistics come from the colour render alone.  `features` is a leaf of the returned dict with an Adam
    group of its own (lrs["features"], default 2.5e-3) and follows every round row by row like any other per-Gaussian table; the
    decoder is NOT in the dict -- a round moves every tensor of N rows, and a decoder with latent_dim == N is no per-Gaussian table --
    but in a second torch.optim.Adam (decoder_lr, eps 1e-15).  history gains feature_loss (the term before its weight, per step)
    and decoder.
    adam: which optimiser steps the per-Gaussian tables.  "torch" (the default) is torch.optim.Adam, the code path before the keyword
    existed.  "fused" is adam.SplatAdam: the same arithmetic, one HIP kernel per tensor.  "visible" hands SplatAdam the radii of the
    step's colour render (which then runs with means2d_grad=True under the MCMC strategy too: that is what reports them), and only the
    Gaussians the view saw (radii > 0) are stepped -- gsplat's SelectiveAdam, the reference trainer's sparse_grad.  For a Gaussian the
    view did NOT see, nothing is read or written that step: its parameters and both Adam moments keep their bits, so the moments do
    not decay and no stale momentum moves it, and the gradient opacity_reg / scale_reg give it (the only one it has) is not applied.
    The step count, and with it the bias correction, advances for every table at every step.  The `features` leaf of the feature term
    is in the same optimiser and takes the same mask (the same view, the same geometry); the decoder keeps its torch.optim.Adam.
    means_lr_final: None, or the factor the means group's learning rate has decayed by at the end: step s of `steps` runs with
    lr0 * means_lr_final ** (s / steps), computed on the host and written into the group before the optimiser steps -- the reference
    trainer's schedule (its value is 0.01).  The MCMC noise, scaled by the group's current rate, follows it.  history["means_lr"] then
    holds the rate of every step; no other group's rate changes, and without the keyword no rate is touched.
    depth_fn(v): the view's depth supervision, or None for a view that has none.  None (the default): no depth term, and nothing of the
    step changes.  Set, the colour render runs with render_mode="RGB+D" (a render_mode in raster_kw then raises GwbpError), the
    photometric loss takes its channels 0:3, and the step adds depth_lambda * the depth loss with scale=depth_scale, as the reference
    trainer's depth_loss option does (its depth_lambda is 1e-2 and its scale the scene's scale): depth.depth_point_loss for a
    (points [M, 2], depths [M]) pair -- scene_io.view_depth_points makes one from a COLMAP model -- or depth.depth_map_loss(kind=
    depth_kind) for an [H, W] depth map.  Both read the render's accumulated depth and alpha in place.  The densify statistics see the
    gradient of the summed loss, as in the reference.  history["depth_loss"]: the term before its weight, one value per step (0 for a
    view without supervision), read once behind the loop.
    pose_noise > 0: a fixed pose.PoseAdjust, drawn once from `seed` with std = pose_noise, perturbs every view first (the reference's
    pose_perturb: captures whose COLMAP poses are slightly off).  pose_opt: a zero-initialised PoseAdjust is applied behind the noise and
    trained with the Gaussians by its own torch.optim.Adam(lr=pose_opt_lr, weight_decay=pose_opt_reg), step s at pose_opt_lr *
    0.01 ** (s / steps); the colour render then runs with pose_grad=True and the latent render with camera_grad=True (the depth column is
    a torch function of the view matrix already).  history gains viewmats [V, 4, 4] (the views as they ended), pose_adjust [V, 9] under
    pose_opt -- in history, not in the splat dict: a round moves every tensor of N rows, and V may equal N -- and under pose_noise
    pose_err: per step, the mean absolute difference between the true and the used camera-to-world matrices over all views, read once
    behind the loop.  A negative or non-finite value, and either option without a view, raise GwbpError.  pose.PoseTraining holds all of
    it; without these keywords nothing of the step changes."""
    if strategy is not None and cfg is not None:
        raise GwbpError("train_scene() takes cfg= or strategy=, not both")
    if strategy is not None and not isinstance(strategy, (DensifyConfig, MCMCConfig)):
        raise GwbpError(f"strategy must be None, a DensifyConfig or an MCMCConfig, got {type(strategy).__name__}")
    mcmc = strategy if isinstance(strategy, MCMCConfig) else None
    cfg = strategy if isinstance(strategy, DensifyConfig) else cfg if cfg is not None else DensifyConfig()
    opacity_reg, scale_reg = float(opacity_reg), float(scale_reg)
    interval = check_sh_degree_interval(sh_degree_interval, "train_scene")
    final = check_means_lr_final(means_lr_final, "train_scene")
    depth_kw = check_depth_options("train_scene", depth_fn, depth_lambda, depth_scale, depth_kind, raster_kw)
    posed = check_pose_options("train_scene", int(viewmats.shape[0]), pose_opt, pose_opt_lr, pose_opt_reg, pose_noise)
    work, opt = trainable(splats, params, lrs, "train_scene", check_adam(adam, "train_scene"))
    dev = work["means"].device
    poses = PoseTraining(viewmats.to(dev), steps, seed, pose_opt, pose_opt_lr, pose_opt_reg, pose_noise) if posed else None
    decay = means_lr_decay(opt, work, final, "train_scene")
    table_degree = table_sh_degree(work)
    for key in GEOMETRY_KEYS:  # what the rounds write must be float32 whether it is trained or not
        work[key] = work[key] if work[key].requires_grad else work[key].float()
    # ONE device generator: the split noise of the default strategy; under MCMC relocate, sample_add and inject_noise, in that order
    noise_gen = torch.Generator(device=dev).manual_seed(int(seed))
    rounds = MCMCRounds(mcmc, noise_gen) if mcmc is not None else DensifyRounds(cfg, work["means"].shape[0], dev, noise_gen)
    feature = None
    if feature_fn is not None:
        work, decoder, opt_dec = _feature_leaves(work, opt, lrs, feature_dim, latent_dim, decoder, decoder_lr, seed)
        latent_kw = {k: raster_kw[k] for k in LATENT_RENDER_KW if k in raster_kw}
        feature = (feature_fn, feature_weight, feature_loss, decoder, opt_dec, dict(latent_kw, camera_grad=True) if pose_opt else latent_kw)
    render_kw = dict(means2d_grad=rounds.means2d_grad or adam == "visible", **depth_kw, **(dict(pose_grad=True) if pose_opt else {}),
                     **raster_kw)
    work, history = _run(work, opt, dict(carry or {}), seed, viewmats=viewmats, K=K, width=int(width), height=int(height),
                         image_fn=image_fn, steps=steps, ssim_lambda=ssim_lambda, adam=adam, render_kw=render_kw, table_degree=table_degree,
                         interval=interval, decay=decay, rounds=rounds, poses=poses, opacity_reg=opacity_reg, scale_reg=scale_reg,
                         depth=None if depth_fn is None else (depth_fn, depth_lambda, depth_scale, depth_kind), feature=feature)
    if poses is not None:
        history.update(poses.history())
    if feature_fn is not None:  # (behind the pose entries, as the keys have always come)
        history.update(feature_loss=history.pop("feature_loss"), decoder=decoder.detach())
    return work, history
