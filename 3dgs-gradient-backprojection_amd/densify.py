"""Grow and prune the set of Gaussians while it is trained: gsplat 1.4.0's DefaultStrategy as DESIGN.md 4.0i states it (the rule
written there is the contract, not the library), on HIP kernels (csrc/densify.hip).

    state = DensifyState(n, device)
    ...  render with rasterization(means2d_grad=True), loss.backward()  ...
    state.update(meta)                                        # every step: one fused pass over meta["means2d"].grad
    splats, info = densify(splats, state, cfg, step, optimizer=opt, carry={"field": field})     # every refine_every steps
    reset_opacity(splats, opt, cfg)                           # every reset_every steps
    splats, history = train_scene(splats, viewmats, K, W, H, image_fn, steps=7000, cfg=DensifyConfig())
    splats = init_splats_from_points(points, rgb)             # the start: a COLMAP point cloud

A Gaussian whose screen-space gradient norm, averaged over the steps that saw it, is above grow_grad2d is duplicated when it is small
and split in two when it is not; one whose opacity is below prune_opa -- or, after the first opacity reset, whose size is above
prune_scale3d -- leaves.  One round is a plan (kind per Gaussian and the exclusive scan of the rows each leaves behind), an emit (the new
means, scales, rotations and opacities, children adjacent, in parent order) and a gather of every other per-Gaussian table, the Adam
moments among them.  One host read per round: the size of the new set.  Splat dicts carry the reference's key names, pre-activation
(polish.py).  There is no PyTorch fallback: CPU tensors raise GwbpError.

Not offered: absgrad, the radius criteria (grow_scale2d, prune_scale2d, refine_scale2d_stop_iter), revised_opacity, packed mode.
gsplat's other strategy, MCMCStrategy, is mcmc.py; train_scene(strategy=MCMCConfig(...)) runs it (without packed mode; the
counterpart of its sparse gradients is train_scene(adam="visible"): adam.SplatAdam steps the Gaussians a step's view saw).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import GwbpError, ptr
from ._views import ld, run
from .photometric import photometric_loss
from .polish import (PARAM_KEYS, check_adam, check_means_lr_final, check_sh_degree_interval, means_group, means_lr_at, render_splats,
                     scheduled_sh_degree, splat_geometry, table_sh_degree, trainable, view_K, view_schedule)
from .rasterization import release_engines

GEOMETRY_KEYS = ("means", "scaling", "rotation", "opacity")  # what the emit kernel writes; every other [N, ...] tensor is gathered
SH_C0 = 0.28209479177387814


def f32(x: float) -> float:
    """x rounded to float32 once (the thresholds are computed in float64 on the host)."""
    return C.c_float(x).value


@dataclass
class DensifyConfig:
    """gsplat's DefaultStrategy fields under its defaults; max_gaussians is ours: a round whose plan would exceed it keeps every clone
    and split as keep and still prunes."""
    prune_opa: float = 0.005
    grow_grad2d: float = 2e-4
    grow_scale3d: float = 0.01
    prune_scale3d: float = 0.1
    refine_start_iter: int = 500
    refine_stop_iter: int = 15000
    refine_every: int = 100
    reset_every: int = 3000
    pause_refine_after_reset: int = 0
    scene_scale: float = 1.0
    max_gaussians: Optional[int] = None

    def __post_init__(self):
        if not (0.0 < self.prune_opa < 0.5):
            raise GwbpError(f"prune_opa must be in (0, 0.5): the reset value is logit(2 prune_opa) (got {self.prune_opa})")
        if not (self.grow_grad2d >= 0.0):
            raise GwbpError(f"grow_grad2d must be >= 0 (got {self.grow_grad2d})")
        for name in ("grow_scale3d", "prune_scale3d", "scene_scale"):
            v = getattr(self, name)
            if not (v > 0.0 and math.isfinite(v)):
                raise GwbpError(f"{name} must be positive and finite (got {v})")
        for name in ("refine_every", "reset_every"):
            if int(getattr(self, name)) < 1:
                raise GwbpError(f"{name} must be at least 1 (got {getattr(self, name)})")
        for name in ("refine_start_iter", "refine_stop_iter", "pause_refine_after_reset"):
            if int(getattr(self, name)) < 0:
                raise GwbpError(f"{name} must be >= 0 (got {getattr(self, name)})")
        if self.max_gaussians is not None and int(self.max_gaussians) < 1:
            raise GwbpError(f"max_gaussians must be None or at least 1 (got {self.max_gaussians})")

    def thresholds(self) -> Tuple[float, float, float, float, float]:
        """(t_grad, t_small, t_big, t_opa, log16): every comparison of the plan happens in pre-activation space, so the thresholds
        are what moves -- float64 here, rounded to float32 once."""
        return (f32(self.grow_grad2d), f32(math.log(self.grow_scale3d * self.scene_scale)),
                f32(math.log(self.prune_scale3d * self.scene_scale)), f32(math.log(self.prune_opa / (1.0 - self.prune_opa))),
                f32(math.log(1.6)))

    def refines_at(self, step: int) -> bool:
        return (step < self.refine_stop_iter and step > self.refine_start_iter and step % self.refine_every == 0
                and step % self.reset_every >= self.pause_refine_after_reset)

    def resets_at(self, step: int) -> bool:
        return 0 < step < self.refine_stop_iter and step % self.reset_every == 0


def device_f32(t, name: str, tail=None) -> torch.Tensor:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise GwbpError(f"{name} must be a HIP tensor (there is no CPU path)")
    if t.dtype != torch.float32:
        raise GwbpError(f"{name} must be float32, got {t.dtype}")
    if tail is not None and tuple(t.shape[1:]) != tuple(tail):
        raise GwbpError(f"{name} has shape {tuple(t.shape)}, expected [N{''.join(', ' + str(d) for d in tail)}]")
    return t.detach().contiguous()


class DensifyState:
    """The running statistics of a round: grad2d [n], the sum of each Gaussian's screen-space gradient norms, and count [n], the
    number of (step, camera) pairs that saw it.  float32, zero at the start and after every round."""

    def __init__(self, n: int, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise GwbpError("DensifyState needs a HIP device (there is no CPU path)")
        self.n, self.device = int(n), device
        self.grad2d = torch.zeros(self.n, device=device)
        self.count = torch.zeros(self.n, device=device)

    def update(self, meta) -> None:
        """After loss.backward() of a rasterization(means2d_grad=True) call: one kernel adds the call's cameras into the statistics
        (gwbp_densify_accumulate), the norm in units of half the image times the number of cameras, as gsplat normalises it."""
        leaf = meta["means2d"]
        g = leaf.grad
        if g is None:
            raise GwbpError("meta['means2d'].grad is None: render with rasterization(means2d_grad=True) and run the backward first")
        radii = meta["radii"]
        n_cam = int(meta["n_cameras"])
        if tuple(g.shape) != (n_cam, self.n, 2) or tuple(radii.shape) != (n_cam, self.n) or radii.dtype != torch.int32:
            raise GwbpError(f"the state holds {self.n} Gaussians; meta has means2d.grad {tuple(g.shape)} and {radii.dtype} radii "
                            f"{tuple(radii.shape)} of {n_cam} cameras")
        g, radii = device_f32(g, "means2d.grad"), radii.contiguous()
        run("gwbp_densify_accumulate", self.device, C.c_int64(self.n), n_cam, ptr(g), ptr(radii),
            C.c_float(float(meta["width"]) / 2.0 * n_cam), C.c_float(float(meta["height"]) / 2.0 * n_cam), ptr(self.grad2d), ptr(self.count))


def as_rows(t: torch.Tensor, n: int) -> torch.Tensor:
    """A per-Gaussian float32 tensor as the [n, w] table the gather kernel reads: a view where the layout allows it."""
    if t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1) and (n <= 1 or t.stride(0) >= t.shape[1]):
        return t
    return t.reshape(n, -1) if t.is_contiguous() else t.contiguous().reshape(n, -1)


def gather_rows(table: torch.Tensor, parent: torch.Tensor, n: int, child=None, kind=None, mode: str = "copy") -> torch.Tensor:
    """out[r] = table[parent[r]] of a float32 per-Gaussian tensor [n, ...] (gwbp_densify_gather), shaped [n_out, ...].  mode "zero_new":
    the rows of a clone's copy and of both children of a split are zeros (gsplat's rule for optimiser moments)."""
    if mode not in _lib.DENSIFY_MODES:
        raise GwbpError(f"mode must be one of {sorted(_lib.DENSIFY_MODES)}, got {mode!r}")
    if not torch.is_tensor(table) or not table.is_cuda or table.dtype != torch.float32 or table.dim() < 1 or table.shape[0] != n:
        raise GwbpError(f"a gathered table must be a float32 HIP tensor [{n}, ...]")
    table = table.detach()
    n_out = int(parent.shape[0])
    out = torch.empty((n_out,) + tuple(table.shape[1:]), device=table.device)
    w = int(math.prod(table.shape[1:]))
    if n_out == 0 or w == 0:
        return out
    rows = as_rows(table, n)
    run("gwbp_densify_gather", table.device, C.c_int64(n), C.c_int64(n_out), int(w), ptr(rows), C.c_int64(ld(rows)), ptr(parent),
        ptr(child), ptr(kind), _lib.DENSIFY_MODES[mode], ptr(out), C.c_int64(w))
    return out


def plan(grad2d, count, scaling, opacity, thresholds: Sequence[float], prune_big: bool):
    """(kind uint8 [n], offsets int64 [n + 1]) of gwbp_densify_plan: what becomes of each Gaussian (0 pruned, 1 keep, 2 clone, 3 split)
    and the exclusive scan of the rows it leaves behind; offsets[n] is the size of the new set.  No host read."""
    scaling, opacity = device_f32(scaling, "scaling", (3,)), device_f32(opacity, "opacity", ())
    grad2d, count = device_f32(grad2d, "grad2d", ()), device_f32(count, "count", ())
    n, dev = scaling.shape[0], scaling.device
    if not (opacity.shape[0] == grad2d.shape[0] == count.shape[0] == n):
        raise GwbpError(f"{n} scaling rows, {opacity.shape[0]} opacities and statistics of {grad2d.shape[0]} Gaussians")
    kind = torch.empty(n, dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    need = C.c_size_t(0)
    _lib.check(_lib.lib().gwbp_densify_plan_workspace_size(C.c_int64(n), C.byref(need)), "gwbp_densify_plan_workspace_size")
    ws = torch.empty(max(1, int(need.value) // 8), dtype=torch.int64, device=dev)
    t = [C.c_float(float(v)) for v in thresholds]
    run("gwbp_densify_plan", dev, C.c_int64(n), ptr(grad2d), ptr(count), ptr(scaling), C.c_int64(3), ptr(opacity), *t, int(bool(prune_big)),
        ptr(kind), ptr(offsets), ptr(ws), C.c_size_t(ws.numel() * 8))
    return kind, offsets


def emit(kind, offsets, n_out: int, means, scaling, rotation, opacity, noise, log16: float):
    """The new set's geometry (gwbp_densify_emit): dict(parent int32 [n_out], child uint8 [n_out], means, scaling, rotation, opacity)."""
    means, scaling = device_f32(means, "means", (3,)), device_f32(scaling, "scaling", (3,))
    rotation, opacity = device_f32(rotation, "rotation", (4,)), device_f32(opacity, "opacity", ())
    n, dev = means.shape[0], means.device
    noise = device_f32(noise, "noise", (2, 3))
    if not (scaling.shape[0] == rotation.shape[0] == opacity.shape[0] == noise.shape[0] == kind.shape[0] == n and offsets.shape[0] == n + 1):
        raise GwbpError(f"emit: the tables of {n} Gaussians do not agree in their first dimension")
    out = dict(parent=torch.empty(n_out, dtype=torch.int32, device=dev), child=torch.empty(n_out, dtype=torch.uint8, device=dev),
               means=torch.empty(n_out, 3, device=dev), scaling=torch.empty(n_out, 3, device=dev),
               rotation=torch.empty(n_out, 4, device=dev), opacity=torch.empty(n_out, device=dev))
    run("gwbp_densify_emit", dev, C.c_int64(n), C.c_int64(n_out), ptr(kind), ptr(offsets), ptr(means), ptr(scaling), ptr(rotation),
        ptr(opacity), ptr(noise), C.c_float(float(log16)), ptr(out["parent"]), ptr(out["child"]), ptr(out["means"]), ptr(out["scaling"]),
        ptr(out["rotation"]), ptr(out["opacity"]))
    return out


def _plan_and_read(state, scaling, opacity, thresholds, prune_big):
    kind, offsets = plan(state.grad2d, state.count, scaling, opacity, thresholds, prune_big)
    # the one host read of a round: the size of the new set, with the four counts riding along
    host = torch.cat([offsets[-1:], torch.bincount(kind.to(torch.int64), minlength=4)]).cpu().tolist()
    return kind, offsets, int(host[0]), [int(v) for v in host[1:5]]


def densify(splats: Dict[str, torch.Tensor], state: DensifyState, cfg: DensifyConfig, step: int, *, optimizer=None,
            carry: Optional[Dict[str, torch.Tensor]] = None, generator: Optional[torch.Generator] = None):
    """One round: (new_splats, info).  Every float32 tensor of `splats` whose first dimension is N comes back with N' rows, in parent
    order with children adjacent; other entries are passed on.  info: parent int32 [N'], child uint8 [N'], kind uint8 [N] and the
    counts pruned, kept, cloned, split (parents of each kind; N' = kept + 2 (cloned + split)), n_before, n_after, and "carry".
    carry: further per-Gaussian float32 tables (feature fields, label weights stored as float); they come back relocated in
    info["carry"], a clone's and a split's children holding the parent's row.
    optimizer: a torch.optim.Adam whose groups hold one tensor of `splats` each (as polish_scene and train_scene build it): the
    parameters are replaced by the new leaves, exp_avg and exp_avg_sq follow with zeros on new rows (a clone's original keeps its
    moments), `step` is kept.
    generator: draws the split noise, torch.randn [N, 2, 3] (a CPU generator draws on the host); the same seed gives the same bits.
    prune_big, the size criterion of the prune, holds when step > cfg.reset_every.  `state` is reset to zeros of size N'."""
    for k in GEOMETRY_KEYS:
        if k not in splats:
            raise GwbpError(f"the splat dict has no {k!r}")
    if not splats["means"].is_cuda:
        raise GwbpError("densify() needs HIP tensors (there is no CPU path)")
    n, dev = int(splats["means"].shape[0]), splats["means"].device
    if state.n != n:
        raise GwbpError(f"the state holds {state.n} Gaussians, the splat dict {n}")
    rowwise = {k: t for k, t in splats.items() if torch.is_tensor(t) and t.dim() >= 1 and t.shape[0] == n and k not in GEOMETRY_KEYS}
    for k, t in list(rowwise.items()) + list((carry or {}).items()):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.shape[0] != n:
            raise GwbpError(f"{k!r} must be a float32 HIP tensor of {n} rows to follow the round (store labels as float, or relocate "
                            f"them with info['parent'])")
    thresholds = cfg.thresholds()
    prune_big = int(step) > cfg.reset_every
    scaling, opacity = splats["scaling"], splats["opacity"]
    kind, offsets, n_out, counts = _plan_and_read(state, scaling, opacity, thresholds, prune_big)
    if cfg.max_gaussians is not None and n_out > cfg.max_gaussians:
        # nothing grows in this round (no gradient is above +inf); the prune still runs.  The one round that reads the host twice
        kind, offsets, n_out, counts = _plan_and_read(state, scaling, opacity, (math.inf,) + tuple(thresholds[1:]), prune_big)
    if generator is not None and generator.device.type == "cpu":
        noise = torch.randn(n, 2, 3, generator=generator).to(dev)
    else:
        noise = torch.randn(n, 2, 3, generator=generator, device=dev)
    new = emit(kind, offsets, n_out, splats["means"], scaling, splats["rotation"], opacity, noise, thresholds[4])
    parent, child = new["parent"], new["child"]
    out = dict(splats)
    for k in GEOMETRY_KEYS:
        out[k] = new[k]
    for k, t in rowwise.items():
        out[k] = gather_rows(t, parent, n)
    if optimizer is not None:
        _relocate_adam(optimizer, splats, out, parent, child, kind, n)
    moved = {k: gather_rows(t, parent, n) for k, t in (carry or {}).items()}
    state.n = n_out
    state.grad2d, state.count = torch.zeros(n_out, device=dev), torch.zeros(n_out, device=dev)
    info = dict(parent=parent, child=child, kind=kind, pruned=counts[0], kept=counts[1], cloned=counts[2], split=counts[3],
                n_before=n, n_after=n_out, step=int(step), prune_big=bool(prune_big), carry=moved)
    return out, info


def swap_adam_leaves(optimizer, old: Dict, new: Dict, moments: Callable[[torch.Tensor], torch.Tensor]) -> None:
    """Swap the optimiser's parameters for the new set's leaves (densify, mcmc.sample_add): every group must hold one tensor of `old`;
    new[key] becomes a leaf and takes the group, the Adam moments follow as moments(table), `step` is kept."""
    if not isinstance(optimizer, torch.optim.Adam):
        raise GwbpError(f"densify() relocates the state of torch.optim.Adam, got {type(optimizer).__name__}")
    by_id = {id(t): k for k, t in old.items() if torch.is_tensor(t)}
    for group in optimizer.param_groups:
        if len(group["params"]) != 1 or id(group["params"][0]) not in by_id:
            raise GwbpError("every group of the optimizer must hold exactly one tensor of the splat dict")
        p = group["params"][0]
        key = by_id[id(p)]
        leaf = new[key].detach().requires_grad_(True)
        new[key] = leaf
        st = optimizer.state.pop(p, None)
        group["params"][0] = leaf
        if st:
            for name in ("exp_avg", "exp_avg_sq"):
                st[name] = moments(st[name])
            if "max_exp_avg_sq" in st:
                st["max_exp_avg_sq"] = moments(st["max_exp_avg_sq"])
            optimizer.state[leaf] = st


def _relocate_adam(optimizer, old: Dict, new: Dict, parent, child, kind, n: int) -> None:
    """Swap the optimiser's parameters for the new set's leaves and carry the Adam moments over (zero_new)."""
    swap_adam_leaves(optimizer, old, new, lambda t: gather_rows(t, parent, n, child, kind, "zero_new"))


def reset_opacity(splats: Dict[str, torch.Tensor], optimizer, cfg: DensifyConfig) -> Dict[str, torch.Tensor]:
    """gsplat's opacity reset: opacity = min(opacity, logit(2 prune_opa)) in place, and that parameter's Adam moments zeroed.  Plain
    torch: N-sized, once every reset_every steps."""
    cap = math.log(2.0 * cfg.prune_opa / (1.0 - 2.0 * cfg.prune_opa))
    p = splats["opacity"]
    with torch.no_grad():
        p.clamp_(max=cap)
    st = optimizer.state.get(p) if optimizer is not None else None
    if st:
        for name in ("exp_avg", "exp_avg_sq"):
            st[name].zero_()
    return splats


DEPTH_KINDS = tuple(_lib.DEPTH_KINDS)  # train_scene(depth_kind=...): depth.depth_map_loss's kinds
LATENT_RENDER_KW = ("near_plane", "far_plane", "radius_clip", "eps2d", "rasterize_mode", "camera_model")  # render_latents' keywords


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
    from .decoded_field import decoded_loss
    from .depth import depth_map_loss, depth_point_loss
    from .latent_render import render_latents
    from .mcmc import MCMCConfig, inject_noise, relocate, sample_add
    from .pose import PoseTraining, check_pose_options
    if strategy is not None and cfg is not None:
        raise GwbpError("train_scene() takes cfg= or strategy=, not both")
    if strategy is not None and not isinstance(strategy, (DensifyConfig, MCMCConfig)):
        raise GwbpError(f"strategy must be None, a DensifyConfig or an MCMCConfig, got {type(strategy).__name__}")
    mcmc = strategy if isinstance(strategy, MCMCConfig) else None
    cfg = strategy if isinstance(strategy, DensifyConfig) else cfg if cfg is not None else DensifyConfig()
    opacity_reg, scale_reg = float(opacity_reg), float(scale_reg)
    interval = check_sh_degree_interval(sh_degree_interval, "train_scene")
    final = check_means_lr_final(means_lr_final, "train_scene")
    depth_kw, depth_losses = {}, []
    if depth_fn is not None:
        if not callable(depth_fn):
            raise GwbpError(f"train_scene(): depth_fn must be a callable of the view's index, got {type(depth_fn).__name__}")
        if "render_mode" in raster_kw:
            raise GwbpError("train_scene(depth_fn=...) renders with render_mode='RGB+D': leave render_mode out of the raster keywords")
        if depth_kind not in DEPTH_KINDS:
            raise GwbpError(f"train_scene(): depth_kind must be one of {list(DEPTH_KINDS)}, got {depth_kind!r}")
        for name, value in (("depth_lambda", depth_lambda), ("depth_scale", depth_scale)):
            if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(float(value)):
                raise GwbpError(f"train_scene(): {name} must be a finite number, got {value!r}")
        depth_kw = dict(render_mode="RGB+D", return_alpha=True)
    posed = check_pose_options("train_scene", int(viewmats.shape[0]), pose_opt, pose_opt_lr, pose_opt_reg, pose_noise)
    work, opt = trainable(splats, params, lrs, "train_scene", check_adam(adam, "train_scene"))
    poses = PoseTraining(viewmats.to(work["means"].device), steps, seed, pose_opt, pose_opt_lr, pose_opt_reg, pose_noise) if posed else None
    pose_kw, latent_pose_kw = (dict(pose_grad=True), dict(camera_grad=True)) if pose_opt else ({}, {})
    decayed = means_group(opt, work) if final is not None else None
    if final is not None and decayed is None:
        raise GwbpError("train_scene(): means_lr_final decays the means group's rate, and the means are not among params")
    lr0, means_lrs = (None if decayed is None else decayed["lr"]), []
    table_degree, degrees = table_sh_degree(work), []
    dev, width, height = splats["means"].device, int(width), int(height)
    for key in GEOMETRY_KEYS:  # what the rounds write must be float32 whether it is trained or not
        work[key] = work[key] if work[key].requires_grad else work[key].float()
    noise_gen = torch.Generator(device=dev).manual_seed(int(seed))
    state = DensifyState(work["means"].shape[0], dev)
    carried = dict(carry or {})
    losses, sizes, rounds, resets = [], [], [], []
    opt_dec, feature_losses = None, []
    if feature_fn is not None:
        work, decoder, opt_dec = _feature_leaves(work, opt, lrs, feature_dim, latent_dim, decoder, decoder_lr, seed)
        latent_kw = {k: raster_kw[k] for k in LATENT_RENDER_KW if k in raster_kw}
    for step, v in enumerate(view_schedule(viewmats.shape[0], seed, steps)):
        opt.zero_grad(set_to_none=True)
        degrees.append(table_degree if interval is None else scheduled_sh_degree(step, interval, table_degree))
        geometry, f_loss = (splat_geometry(work) if feature_fn is not None else None), None  # (one exp and one sigmoid for both renders)
        viewmat = viewmats[v] if poses is None else poses.view(v)
        image, *alpha, meta = render_splats(work, viewmat, view_K(K, v), width, height, return_meta=True,
                                            means2d_grad=mcmc is None or adam == "visible",
                                            sh_degree=None if interval is None else degrees[-1], geometry=geometry, **depth_kw,
                                            **pose_kw, **raster_kw)
        loss = photometric_loss(image[..., :3] if depth_fn is not None else image, image_fn(v), ssim_lambda=ssim_lambda)
        if depth_fn is not None:
            target = depth_fn(v)
            if target is None:
                d_loss = torch.zeros((), device=dev)
            elif isinstance(target, (tuple, list)) and len(target) == 2:
                d_loss = depth_point_loss(image, alpha[0], target[0], target[1], scale=float(depth_scale))
            elif torch.is_tensor(target):
                d_loss = depth_map_loss(image, alpha[0], target, kind=depth_kind, scale=float(depth_scale))
            else:
                raise GwbpError(f"depth_fn({v}) must return a (points, depths) pair, an [H, W] tensor or None, got {type(target).__name__}")
            depth_losses.append(d_loss.detach())
            loss = loss + float(depth_lambda) * d_loss
            del target, d_loss
        if feature_fn is not None:
            opt_dec.zero_grad(set_to_none=True)
            latent_map, _ = render_latents(*geometry, work["features"], viewmat, view_K(K, v), width, height, **latent_kw,
                                           **latent_pose_kw)
            f_loss = decoded_loss(latent_map, decoder, feature_fn(v), loss=feature_loss)
            feature_losses.append(f_loss.detach())
            loss = loss + float(feature_weight) * f_loss
            del latent_map
        if opacity_reg != 0.0:
            loss = loss + opacity_reg * torch.sigmoid(work["opacity"]).mean()
        if scale_reg != 0.0:
            loss = loss + scale_reg * torch.exp(work["scaling"]).mean()
        loss.backward()
        if mcmc is None and step < cfg.refine_stop_iter:
            state.update(meta)
        if decayed is not None:  # (the rounds swap a group's leaf, never the group: `decayed` stays the means' group)
            decayed["lr"] = means_lr_at(lr0, final, step, int(steps))
            means_lrs.append(decayed["lr"])
        if adam == "visible":
            opt.step(visible=meta["radii"])
        else:
            opt.step()
        if opt_dec is not None:
            opt_dec.step()
        if poses is not None:
            poses.step(step)
        losses.append(loss.detach())
        sizes.append(int(work["means"].shape[0]))
        if mcmc is not None:
            if mcmc.refines_at(step):
                del image, alpha, meta, loss, f_loss, geometry, viewmat
                n_before = sizes[-1]
                work, moved = relocate(work, mcmc, optimizer=opt, carry=carried, generator=noise_gen)
                work, added = sample_add(work, mcmc, mcmc.n_new(n_before), optimizer=opt, carry=moved["carry"], generator=noise_gen)
                carried = added["carry"]
                rounds.append(dict(step=step, n_before=n_before, n_after=added["n_after"], relocated=moved["relocated"],
                                   added=added["added"]))
                if added["added"]:
                    release_engines(dev, keep_n=added["n_after"])
            rate = next((g["lr"] for g in opt.param_groups if g["params"][0] is work["means"]), None)
            if rate is not None:
                inject_noise(work, rate, mcmc, generator=noise_gen)
            continue
        if cfg.refines_at(step):
            del image, alpha, meta, loss, f_loss, geometry, viewmat  # (the graph holds the old set's workspace)
            work, info = densify(work, state, cfg, step, optimizer=opt, carry=carried, generator=noise_gen)
            carried = info["carry"]
            if info["n_after"] < 1:
                raise GwbpError(f"step {step}: the round pruned every Gaussian")
            rounds.append({k: info[k] for k in ("step", "n_before", "n_after", "pruned", "kept", "cloned", "split")})
            release_engines(dev, keep_n=info["n_after"])
        if cfg.resets_at(step):
            reset_opacity(work, opt, cfg)
            resets.append(step)
    history = dict(loss=torch.stack(losses).cpu().tolist() if losses else [], n=sizes, rounds=rounds, resets=resets, carry=carried,
                   sh_degree=degrees)
    if final is not None:
        history["means_lr"] = means_lrs
    if depth_fn is not None:
        history["depth_loss"] = torch.stack(depth_losses).cpu().tolist() if depth_losses else []
    if poses is not None:
        history.update(poses.history())
    if feature_fn is not None:
        history.update(feature_loss=torch.stack(feature_losses).cpu().tolist() if feature_losses else [], decoder=decoder.detach())
    return {k: (t.detach() if torch.is_tensor(t) else t) for k, t in work.items()}, history


def init_splats_from_points(points, rgb, sh_degree: int = 3, init_opacity: float = 0.1, init_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """A splat dict from a point cloud, as the reference trainer starts: means = the points, log-scales from the distance to the three
    nearest neighbours (spatial.init_scales), identity rotations, opacity logit(init_opacity), features_dc = (rgb - 0.5) / C0 and zero
    higher SH coefficients.  points [N, 3] on the HIP device; rgb [N, 3] in [0, 1] (uint8: divided by 255)."""
    from .spatial import init_scales
    if not torch.is_tensor(points) or not points.is_cuda:
        raise GwbpError("init_splats_from_points() needs HIP tensors (there is no CPU path)")
    if points.dim() != 2 or points.shape[1] != 3 or tuple(rgb.shape) != tuple(points.shape):
        raise GwbpError(f"points and rgb must be [N, 3], got {tuple(points.shape)} and {tuple(rgb.shape)}")
    if not (0.0 < init_opacity < 1.0) or sh_degree < 0:
        raise GwbpError(f"init_opacity must be in (0, 1) and sh_degree >= 0 (got {init_opacity}, {sh_degree})")
    dev, n = points.device, points.shape[0]
    means = points.float().contiguous()
    rgb = rgb.to(dev)
    rgb = rgb.float() / 255.0 if rgb.dtype == torch.uint8 else rgb.float()
    rotation = torch.zeros(n, 4, device=dev)
    rotation[:, 0] = 1.0
    return dict(means=means, scaling=init_scales(means, init_scale), rotation=rotation,
                opacity=torch.full((n,), math.log(init_opacity / (1.0 - init_opacity)), device=dev),
                features_dc=((rgb - 0.5) / SH_C0)[:, None, :].contiguous(),
                features_rest=torch.zeros(n, (sh_degree + 1) ** 2 - 1, 3, device=dev))
