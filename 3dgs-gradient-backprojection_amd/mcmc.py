"""Train a set of Gaussians under a fixed budget: gsplat 1.4.0's MCMCStrategy as DESIGN.md 4.0j states it (the rule written there is
the contract, not the library), on HIP kernels (csrc/mcmc.hip).

    cfg = MCMCConfig(cap_max=1_000_000)
    ...  render, loss + opacity_reg * sigmoid(opacity).mean() + scale_reg * exp(scaling).mean(), backward, optimizer.step()  ...
    if cfg.refines_at(step):
        splats, info = relocate(splats, cfg, optimizer=opt, carry={"field": field})          # dead Gaussians move onto alive ones
        splats, info = sample_add(splats, cfg, cfg.n_new(n), optimizer=opt, carry=info["carry"])   # the set grows by 5 % up to cap_max
    inject_noise(splats, lr_means, cfg)                                                        # every step
    splats, history = train.train_scene(splats, viewmats, K, W, H, image_fn, steps=30000, strategy=MCMCConfig(), opacity_reg=0.01, scale_reg=0.01)

A Gaussian whose opacity is at or below min_opacity is dead.  A relocate round gives every dead Gaussian a parent drawn among the alive
ones with probability proportional to opacity; a parent drawn c times shares itself with its c copies: ratio r = min(c + 1, 51),
opacity 1 - (1 - o)^(1/r), scale s o / D(o', r).  An add round draws parents among all Gaussians in the same way and appends their
copies.  The Adam moments of every parent become zero, those of appended rows are zero, and those of a relocated dead row stay as they
are (gsplat's behaviour, kept).  One host read per relocate round (the number of dead Gaussians, with the total weight riding along),
none per add round.  There is no PyTorch fallback: CPU tensors raise GwbpError.

What differs from gsplat: the sampling weights are the integers floor(opacity 2^24); the draws are sorted, so the
j-th dead Gaussian in index order gets the j-th parent in index order instead of multinomial order; o'^(k+1) is a running product.
Not offered: packed mode, sparse gradient tensors (train_scene(adam="visible") steps the visible rows of dense ones), the binomial
table beyond n_max = 51.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import GwbpError, ptr
from ._views import ld, run
from .densify import GEOMETRY_KEYS, as_rows, device_f32, f32, gather_rows, swap_adam_leaves
from .polish import means_group
from .rasterization import release_engines


@dataclass
class MCMCConfig:
    """gsplat's MCMCStrategy fields under its defaults."""
    cap_max: int = 1_000_000
    noise_lr: float = 5e5
    refine_start_iter: int = 500
    refine_stop_iter: int = 25_000
    refine_every: int = 100
    min_opacity: float = 0.005

    def __post_init__(self):
        if int(self.cap_max) < 1:
            raise GwbpError(f"cap_max must be at least 1 (got {self.cap_max})")
        if not (self.noise_lr >= 0.0 and math.isfinite(self.noise_lr)):
            raise GwbpError(f"noise_lr must be finite and >= 0 (got {self.noise_lr})")
        if not (0.0 < self.min_opacity < 1.0):
            raise GwbpError(f"min_opacity must be in (0, 1) (got {self.min_opacity})")
        if int(self.refine_every) < 1:
            raise GwbpError(f"refine_every must be at least 1 (got {self.refine_every})")
        for name in ("refine_start_iter", "refine_stop_iter"):
            if int(getattr(self, name)) < 0:
                raise GwbpError(f"{name} must be >= 0 (got {getattr(self, name)})")

    def refines_at(self, step: int) -> bool:
        return self.refine_start_iter < step < self.refine_stop_iter and step % self.refine_every == 0

    def n_new(self, n: int) -> int:
        """How many Gaussians an add round appends to a set of n."""
        return max(0, min(int(self.cap_max), int(1.05 * n)) - n)

    def t_opa(self) -> float:
        """logit(min_opacity): the dead test happens in pre-activation space -- float64 here, rounded to float32 once."""
        m = f32(self.min_opacity)
        return f32(math.log(m / (1.0 - m)))


# ---- the kernels, one call each ---------------------------------------------------------------------------------------------------
def plan(opacity: torch.Tensor, t_opa: float, mode: str = "relocate"):
    """(cdf int64 [n + 1], dead_offsets int64 [n + 1], dead_idx int32 [n]) of gwbp_mcmc_plan.  No host read."""
    if mode not in _lib.MCMC_MODES:
        raise GwbpError(f"mode must be one of {sorted(_lib.MCMC_MODES)}, got {mode!r}")
    opacity = device_f32(opacity, "opacity", ())
    n, dev = opacity.shape[0], opacity.device
    cdf = torch.empty(n + 1, dtype=torch.int64, device=dev)
    dead_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    dead_idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    need = C.c_size_t(0)
    _lib.check(_lib.lib().gwbp_mcmc_plan_workspace_size(C.c_int64(n), C.byref(need)), "gwbp_mcmc_plan_workspace_size")
    ws = torch.empty(max(1, int(need.value) // 8), dtype=torch.int64, device=dev)
    run("gwbp_mcmc_plan", dev, C.c_int64(n), ptr(opacity), C.c_float(float(t_opa)), _lib.MCMC_MODES[mode], ptr(cdf), ptr(dead_offsets),
        ptr(dead_idx), ptr(ws), C.c_size_t(ws.numel() * 8))
    return cdf, dead_offsets, dead_idx[:n]


def draw(cdf: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """parent int32 [m] of gwbp_mcmc_draw; u float64 [m], ascending."""
    if u.dtype != torch.float64 or u.dim() != 1 or not u.is_cuda or not u.is_contiguous():
        raise GwbpError("u must be a dense float64 HIP vector")
    n, m = cdf.shape[0] - 1, u.shape[0]
    parent = torch.full((m,), -1, dtype=torch.int32, device=u.device)
    run("gwbp_mcmc_draw", u.device, C.c_int64(n), C.c_int64(m), ptr(cdf), ptr(u), ptr(parent))
    return parent


def update(opacity: torch.Tensor, scaling: torch.Tensor, parent: torch.Tensor, min_opacity: float) -> torch.Tensor:
    """count int32 [n] of gwbp_mcmc_update; the drawn rows of opacity [n] and scaling [n, 3] change IN PLACE."""
    n, dev = opacity.shape[0], opacity.device
    if opacity.dtype != torch.float32 or scaling.dtype != torch.float32 or not opacity.is_contiguous() or not scaling.is_contiguous() \
            or tuple(scaling.shape) != (n, 3):
        raise GwbpError("update() writes dense float32 opacity [n] and scaling [n, 3] in place")
    count = torch.empty(n, dtype=torch.int32, device=dev)
    run("gwbp_mcmc_update", dev, C.c_int64(n), C.c_int64(parent.shape[0]), ptr(parent), C.c_float(f32(min_opacity)), ptr(opacity),
        ptr(scaling), C.c_int64(3), ptr(count))
    return count


def _table(t: torch.Tensor, n: int, name: str) -> torch.Tensor:
    """A float32 per-Gaussian tensor as the [n, w] view the in-place kernels write: it must BE a view."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() < 1 or t.shape[0] < n:
        raise GwbpError(f"{name} must be a float32 HIP tensor of at least {n} rows")
    rows = as_rows(t, t.shape[0])
    if rows.data_ptr() != t.data_ptr():
        raise GwbpError(f"{name} cannot be written in place: its rows are not dense")
    return rows


def move_rows(table: torch.Tensor, parent: torch.Tensor, dead_idx: torch.Tensor, n: int) -> None:
    """table[dead_idx[j]] = table[parent[j]] in place (gwbp_mcmc_move)."""
    if table.numel() == 0 or parent.shape[0] == 0:
        return
    rows = _table(table, n, "a moved table")
    w = int(rows.shape[1])
    run("gwbp_mcmc_move", table.device, C.c_int64(n), C.c_int64(parent.shape[0]), w, ptr(parent), ptr(dead_idx), ptr(rows),
        C.c_int64(ld(rows)))


def zero_rows(table: torch.Tensor, count: torch.Tensor) -> None:
    """table[i] = 0 where count[i] > 0, in place (gwbp_mcmc_zero_rows); the table may have more rows than count."""
    n = count.shape[0]
    if table.numel() == 0 or n == 0:
        return
    rows = _table(table, n, "a zeroed table")
    w = int(rows.shape[1])
    run("gwbp_mcmc_zero_rows", table.device, C.c_int64(n), w, ptr(count), ptr(rows), C.c_int64(ld(rows)))


def device_libm(op: str, a: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """expf(a), logf(a) or powf(a, b) as the kernels evaluate them (gwbp_mcmc_libm): for tests that hold the kernels' bits."""
    a = a.contiguous()
    out = torch.empty_like(a)
    run("gwbp_mcmc_libm", a.device, C.c_int64(a.numel()), _lib.MCMC_LIBM[op], ptr(a), ptr(b.contiguous() if b is not None else None),
        ptr(out))
    return out


# ---- the rounds ------------------------------------------------------------------------------------------------------------------------
def _uniforms(m: int, dev, generator) -> torch.Tensor:
    """m sorted float64 draws in [0, 1) (a CPU generator draws on the host)."""
    if generator is not None and generator.device.type == "cpu":
        u = torch.rand(m, dtype=torch.float64, generator=generator).to(dev)
    else:
        u = torch.rand(m, dtype=torch.float64, generator=generator, device=dev)
    return torch.sort(u).values


def _check(splats, carry, fn: str):
    for k in GEOMETRY_KEYS:
        if k not in splats:
            raise GwbpError(f"the splat dict has no {k!r}")
    if not splats["means"].is_cuda:
        raise GwbpError(f"{fn}() needs HIP tensors (there is no CPU path)")
    n = int(splats["means"].shape[0])
    rowwise = {k: t for k, t in splats.items() if torch.is_tensor(t) and t.dim() >= 1 and t.shape[0] == n}
    for k, t in list(rowwise.items()) + list((carry or {}).items()):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.shape[0] != n:
            raise GwbpError(f"{k!r} must be a float32 HIP tensor of {n} rows to follow the round")
    if tuple(splats["opacity"].shape) != (n,) or tuple(splats["scaling"].shape) != (n, 3):
        raise GwbpError(f"opacity must be [{n}] and scaling [{n}, 3]")
    return n, rowwise


def _adam_states(optimizer, splats):
    """The Adam state dicts of the optimiser's parameters, which must be tensors of the splat dict, one per group."""
    if optimizer is None:
        return []
    if not isinstance(optimizer, torch.optim.Adam):
        raise GwbpError(f"the rounds relocate the state of torch.optim.Adam, got {type(optimizer).__name__}")
    ids = {id(t) for t in splats.values() if torch.is_tensor(t)}
    out = []
    for group in optimizer.param_groups:
        if len(group["params"]) != 1 or id(group["params"][0]) not in ids:
            raise GwbpError("every group of the optimizer must hold exactly one tensor of the splat dict")
        st = optimizer.state.get(group["params"][0])
        if st:
            out.append(st)
    return out


MOMENTS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def relocate(splats: Dict[str, torch.Tensor], cfg: MCMCConfig, *, optimizer=None, carry: Optional[Dict[str, torch.Tensor]] = None,
             generator: Optional[torch.Generator] = None):
    """One relocate round, IN PLACE on the tensors of `splats` (under no_grad: leaves stay leaves, the optimiser keeps its parameter
    objects): (splats, info).  info: relocated (the number of dead Gaussians that moved), n_dead, total_weight, parent int32
    [relocated], dead_idx int32 [relocated], count int32 [n] (None where nothing moved), and "carry": the `carry` tables, moved in place
    as well.  Nothing happens when no Gaussian is dead or no alive one has weight."""
    n, rowwise = _check(splats, carry, "relocate")
    carried = dict(carry or {})
    states = _adam_states(optimizer, splats)
    info = dict(relocated=0, n_dead=0, total_weight=0, parent=None, dead_idx=None, count=None, carry=carried, n_before=n, n_after=n)
    if n == 0:
        return splats, info
    dev = splats["means"].device
    with torch.no_grad():
        opacity, scaling = splats["opacity"], splats["scaling"]
        if not (opacity.is_contiguous() and scaling.is_contiguous()):
            raise GwbpError("relocate() writes opacity and scaling in place: they must be dense")
        cdf, dead_offsets, dead_idx = plan(opacity, cfg.t_opa(), "relocate")
        # the one host read of a round: the number of dead Gaussians, with the total weight riding along
        n_dead, total = (int(v) for v in torch.stack([dead_offsets[n], cdf[n]]).cpu().tolist())
        info.update(n_dead=n_dead, total_weight=total)
        if n_dead == 0 or total == 0:
            return splats, info
        parent = draw(cdf, _uniforms(n_dead, dev, generator))
        count = update(opacity.detach(), scaling.detach(), parent, cfg.min_opacity)
        for k, t in list(rowwise.items()) + list(carried.items()):
            move_rows(t.detach(), parent, dead_idx, n)
        for st in states:
            for name in MOMENTS:
                if name in st:
                    zero_rows(st[name], count)
    info.update(relocated=n_dead, parent=parent, dead_idx=dead_idx[:n_dead], count=count)
    return splats, info


def sample_add(splats: Dict[str, torch.Tensor], cfg: MCMCConfig, n_new: int, *, optimizer=None,
               carry: Optional[Dict[str, torch.Tensor]] = None, generator: Optional[torch.Generator] = None):
    """One add round: (new_splats, info) with n_new rows appended to every float32 per-Gaussian tensor -- copies of parents drawn among
    all Gaussians by opacity, parents and copies holding the shared opacity and scale.  New tensors; the optimiser's parameters are
    swapped for the new leaves, exp_avg and exp_avg_sq follow with zeros on the appended rows and on the parents, `step` is kept.
    info: added, parent int32 [n_new], count int32 [n], n_before, n_after, "carry".  No host read."""
    n, rowwise = _check(splats, carry, "sample_add")
    n_new = int(n_new)
    carried = dict(carry or {})
    if n_new < 0 or n_new > n:
        raise GwbpError(f"n_new must be in [0, n = {n}] (got {n_new})")
    info = dict(added=0, parent=None, count=None, n_before=n, n_after=n, carry=carried)
    if n_new == 0:
        return splats, info
    _adam_states(optimizer, splats)
    dev = splats["means"].device
    with torch.no_grad():
        cdf, _, _ = plan(splats["opacity"], cfg.t_opa(), "add")
        parent = draw(cdf, _uniforms(n_new, dev, generator))
        opacity, scaling = splats["opacity"].detach().clone(), splats["scaling"].detach().clone()
        count = update(opacity, scaling, parent, cfg.min_opacity)
        rows = torch.cat([torch.arange(n, dtype=torch.int32, device=dev), parent])
        source = dict(rowwise, opacity=opacity, scaling=scaling)
        out = dict(splats)
        for k, t in source.items():
            out[k] = gather_rows(t, rows, n)
        moved = {k: gather_rows(t, rows, n) for k, t in carried.items()}
        if optimizer is not None:
            # moments: the old rows in place, the appended ones from outside [0, n), which the gather answers with zeros
            rows0 = torch.cat([rows[:n], torch.full((n_new,), -1, dtype=torch.int32, device=dev)])
            child = torch.zeros(n + n_new, dtype=torch.uint8, device=dev)
            kind = torch.full((n,), _lib.DENSIFY_KINDS["keep"], dtype=torch.uint8, device=dev)

            def moments(t):
                t = gather_rows(t, rows0, n, child, kind, "zero_new")
                zero_rows(t, count)
                return t
            swap_adam_leaves(optimizer, splats, out, moments)
    info.update(added=n_new, parent=parent, count=count, n_after=n + n_new, carry=moved)
    return out, info


def inject_noise(splats: Dict[str, torch.Tensor], lr: float, cfg: MCMCConfig, generator: Optional[torch.Generator] = None) -> None:
    """means += Sigma (randn g(1 - o) lr noise_lr), in place: one torch.randn [n, 3] and one kernel (gwbp_mcmc_noise).  lr: the means
    group's current learning rate."""
    for k in GEOMETRY_KEYS:
        if k not in splats:
            raise GwbpError(f"the splat dict has no {k!r}")
    means = splats["means"]
    if not means.is_cuda:
        raise GwbpError("inject_noise() needs HIP tensors (there is no CPU path)")
    n, dev = means.shape[0], means.device
    if means.dtype != torch.float32 or not means.is_contiguous() or tuple(means.shape) != (n, 3):
        raise GwbpError("inject_noise() writes a dense float32 means [n, 3] in place")
    if generator is not None and generator.device.type == "cpu":
        z = torch.randn(n, 3, generator=generator).to(dev)
    else:
        z = torch.randn(n, 3, generator=generator, device=dev)
    add_noise(means, splats["scaling"], splats["rotation"], splats["opacity"], z, float(lr) * float(cfg.noise_lr))


def add_noise(means, scaling, rotation, opacity, z, scaler: float) -> None:
    """The kernel of inject_noise with the normal draws z [n, 3] handed in: means changes in place."""
    n = means.shape[0]
    scaling, rotation = device_f32(scaling, "scaling", (3,)), device_f32(rotation, "rotation", (4,))
    opacity, z = device_f32(opacity, "opacity", ()), device_f32(z, "z", (3,))
    if not (scaling.shape[0] == rotation.shape[0] == opacity.shape[0] == z.shape[0] == n):
        raise GwbpError(f"add_noise: the tables of {n} Gaussians do not agree in their first dimension")
    with torch.no_grad():
        run("gwbp_mcmc_noise", means.device, C.c_int64(n), ptr(means.detach()), ptr(scaling), ptr(rotation), ptr(opacity), ptr(z),
            C.c_float(f32(scaler)))


class MCMCRounds:
    """train_scene's rounds under this strategy (densify.DensifyRounds has the same members): no means2d gradient, nothing behind the
    backward; after_step -- behind the optimiser's step -- runs a relocate and an add round when cfg.refines_at(step) and at EVERY step
    puts noise on the means at their group's current rate (none when the means are not trained).  generator draws, in this order, for
    relocate, sample_add and inject_noise."""
    means2d_grad = False

    def __init__(self, cfg: MCMCConfig, generator: Optional[torch.Generator]):
        self.cfg, self.generator, self.rounds, self.resets = cfg, generator, [], []

    def after_backward(self, meta, step: int) -> None:
        pass

    def after_step(self, work: Dict[str, torch.Tensor], opt, carried: Dict[str, torch.Tensor], step: int):
        cfg = self.cfg
        if cfg.refines_at(step):
            n_before = int(work["means"].shape[0])
            work, moved = relocate(work, cfg, optimizer=opt, carry=carried, generator=self.generator)
            work, added = sample_add(work, cfg, cfg.n_new(n_before), optimizer=opt, carry=moved["carry"], generator=self.generator)
            carried = added["carry"]
            self.rounds.append(dict(step=step, n_before=n_before, n_after=added["n_after"], relocated=moved["relocated"],
                                    added=added["added"]))
            if added["added"]:  # (the old set's workspace, as in DensifyRounds.after_step)
                release_engines(work["means"].device, keep_n=added["n_after"])
        group = means_group(opt, work)
        if group is not None:
            inject_noise(work, group["lr"], cfg, generator=self.generator)
        return work, carried
