"""Grow and prune the set of Gaussians while it is trained: gsplat 1.4.0's DefaultStrategy as DESIGN.md 4.0i states it (the rule
written there is the contract, not the library), on HIP kernels (csrc/densify.hip).

    state = DensifyState(n, device)
    ...  render with rasterization(means2d_grad=True), run the backward  ...
    state.update(meta)                                        # every step: one fused pass over meta["means2d"].grad
    splats, info = densify(splats, state, cfg, step, optimizer=opt, carry={"field": field})     # every refine_every steps
    reset_opacity(splats, opt, cfg)                           # every reset_every steps
    splats, history = train.train_scene(splats, viewmats, K, W, H, image_fn, steps=7000, cfg=DensifyConfig())   # the loop (train.py)
    splats = init_splats_from_points(points, rgb)             # the start: a COLMAP point cloud

A Gaussian whose screen-space gradient norm, averaged over the steps that saw it, is above grow_grad2d is duplicated when it is small
and split in two when it is not; one whose opacity is below prune_opa -- or, after the first opacity reset, whose size is above
prune_scale3d -- leaves.  One round is a plan (kind per Gaussian and the exclusive scan of the rows each leaves behind), an emit (the new
means, scales, rotations and opacities, children adjacent, in parent order) and a gather of every other per-Gaussian table, the Adam
moments among them.  One host read per round: the size of the new set.  Splat dicts carry the reference's key names, pre-activation
(polish.py).  There is no PyTorch fallback: CPU tensors raise GwbpError.

Not offered: absgrad, the radius criteria (grow_scale2d, prune_scale2d, refine_scale2d_stop_iter), revised_opacity, packed mode.
gsplat's other strategy, MCMCStrategy, is mcmc.py; train.train_scene(strategy=MCMCConfig(...)) runs it (without packed mode; the
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
        """After the backward of a rasterization(means2d_grad=True) call: one kernel adds the call's cameras into the statistics
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


class DensifyRounds:
    """train_scene's rounds under this strategy (mcmc.MCMCRounds has the same members): the colour render reports means2d.grad,
    after_backward adds it into the statistics, after_step -- behind the optimiser's step -- runs the round and then the opacity reset
    that cfg schedules at the step.  rounds and resets are the history's; generator draws the split noise."""
    means2d_grad = True

    def __init__(self, cfg: DensifyConfig, n: int, device, generator: Optional[torch.Generator]):
        self.cfg, self.generator, self.state, self.rounds, self.resets = cfg, generator, DensifyState(n, device), [], []

    def after_backward(self, meta, step: int) -> None:
        if step < self.cfg.refine_stop_iter:
            self.state.update(meta)

    def after_step(self, work: Dict[str, torch.Tensor], opt, carried: Dict[str, torch.Tensor], step: int):
        if self.cfg.refines_at(step):
            work, info = densify(work, self.state, self.cfg, step, optimizer=opt, carry=carried, generator=self.generator)
            carried = info["carry"]
            if info["n_after"] < 1:
                raise GwbpError(f"step {step}: the round pruned every Gaussian")
            self.rounds.append({k: info[k] for k in ("step", "n_before", "n_after", "pruned", "kept", "cloned", "split")})
            # the old set's workspace goes here: the step is a function that has returned, so no graph, meta or render holds it
            release_engines(self.state.device, keep_n=info["n_after"])
        if self.cfg.resets_at(step):
            reset_opacity(work, opt, self.cfg)
            self.resets.append(step)
        return work, carried


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
