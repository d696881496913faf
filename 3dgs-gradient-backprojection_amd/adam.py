"""The optimiser step of training as one HIP kernel per table, with a row mask (csrc/adam.hip).

    opt = SplatAdam([dict(params=[means], lr=1.6e-4), dict(params=[opacity], lr=5e-2)], eps=1e-15)
    loss.backward()
    opt.step()                                   # torch.optim.Adam's arithmetic, one fused pass per tensor
    opt.step(visible=meta["radii"])              # ... on the Gaussians the step's view saw; the others keep every bit

SplatAdam IS a torch.optim.Adam: param_groups, state (step, exp_avg, exp_avg_sq -- step a host scalar, as on torch's default route),
state_dict and add_param_group are torch's, so densify.swap_adam_leaves, reset_opacity and the MCMC rounds take it as they take torch's.
Only step() is ours.  With a mask it is gsplat's SelectiveAdam: a row no camera of the step saw is not read and not written -- its
parameters, its moments (which do not decay) and whatever gradient it has (a regulariser's) stay as they are -- while the step count,
and with it the bias correction, advances for every tensor on every call.
"""
from __future__ import annotations

from typing import Iterable, Optional

import torch

from ._lib import GwbpError
from .engine import adam_step_tables
from .sh import device_caller


def visible_rows(visible: torch.Tensor) -> torch.Tensor:
    """The mask of SplatAdam.step as the kernel reads it: uint8 or bool [N] as given, int32 radii [C, N] as (radii > 0).any(0)."""
    if not torch.is_tensor(visible) or not visible.is_cuda:
        raise GwbpError("SplatAdam.step(): visible must be a HIP tensor (there is no CPU path)")
    if visible.dtype == torch.int32 and visible.dim() == 2:
        return (visible > 0).any(0) if visible.shape[0] != 1 else visible[0] > 0
    if visible.dtype in (torch.uint8, torch.bool) and visible.dim() == 1:
        return visible.contiguous()
    raise GwbpError(f"SplatAdam.step(): visible must be bool or uint8 [N], or int32 radii [C, N]; got {visible.dtype} "
                    f"{tuple(visible.shape)}")


class SplatAdam(torch.optim.Adam):
    """torch.optim.Adam whose step() is gwbp_adam_step: float32 HIP parameters, weight_decay = 0, no amsgrad, no maximize."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, amsgrad: bool = False,
                 *, maximize: bool = False, **unsupported):
        if amsgrad or maximize or weight_decay != 0:
            raise GwbpError(f"SplatAdam offers no amsgrad, weight_decay or maximize (got amsgrad={amsgrad}, weight_decay={weight_decay}, "
                            f"maximize={maximize})")
        if any(unsupported.values()):
            raise GwbpError(f"SplatAdam takes none of torch.optim.Adam's {sorted(unsupported)}")
        if torch.is_tensor(lr) or any(torch.is_tensor(b) for b in betas):
            raise GwbpError("SplatAdam takes lr and betas as Python floats (the step's scalars are formed on the host)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=0.0, amsgrad=False, foreach=False, fused=False)

    @staticmethod
    def _check_param(p: torch.Tensor) -> None:
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise GwbpError(f"SplatAdam steps contiguous float32 parameters, got {p.dtype} {tuple(p.shape)} with strides {tuple(p.stride())}")
        if not p.is_cuda:
            raise GwbpError("SplatAdam needs HIP tensors (there is no CPU path)")

    def add_param_group(self, param_group) -> None:
        params = param_group["params"]
        for p in ([params] if torch.is_tensor(params) else list(params)):
            self._check_param(p)
        if param_group.get("amsgrad") or param_group.get("maximize") or param_group.get("weight_decay", 0) != 0:
            raise GwbpError("SplatAdam offers no amsgrad, weight_decay or maximize")
        super().add_param_group(param_group)

    @torch.no_grad()
    def step(self, closure=None, *, visible: Optional[torch.Tensor] = None, dense: Iterable[torch.Tensor] = ()):
        """One step of every group tensor that has a gradient (None: skipped, as torch does; not contiguous: made so).
        visible: None steps every row.  A bool or uint8 [N], or the int32 meta["radii"] [C, N] of the step's render (a row is visible
        where any camera's radius is positive): rows that are not visible keep the bits of the parameter and of both moments.
        The step count advances for every stepped tensor on every call, visible or not, and the bias correction uses that count.
        dense: tensors of the groups whose first dimension is not the mask's length and that are to be stepped whole (a decoder beside
        per-Gaussian tables); any other such tensor is an error."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        mask = None if visible is None else visible_rows(visible)
        whole = {id(t) for t in dense}
        todo = []  # every check first: a call that raises has stepped nothing
        for group in self.param_groups:
            if group["amsgrad"] or group["maximize"] or group["weight_decay"] != 0:
                raise GwbpError("SplatAdam offers no amsgrad, weight_decay or maximize")
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._check_param(p)
                if p.grad.is_sparse or p.grad.dtype != torch.float32:
                    raise GwbpError(f"SplatAdam steps dense float32 gradients, got {p.grad.dtype}")
                rows = mask
                if mask is not None and (p.dim() == 0 or p.shape[0] != mask.shape[0] or mask.device != p.device):
                    if id(p) not in whole:
                        raise GwbpError(f"SplatAdam.step(): the mask has {mask.shape[0]} rows on {mask.device}, a parameter is "
                                        f"{tuple(p.shape)} on {p.device}: list it in dense= to step it whole")
                    rows = None
                todo.append((group, p, rows))
        for group, p, rows in todo:
            state = self.state[p]
            if len(state) == 0:  # torch's lazy state, its default route: the count on the host
                state["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["step"] += 1
            b1, b2 = group["betas"]
            call, stream = device_caller(p.device)
            adam_step_tables(call, stream, p, p.grad.contiguous(), state["exp_avg"], state["exp_avg_sq"], rows,
                             int(state["step"].item()), float(group["lr"]), float(b1), float(b2), float(group["eps"]))
        return loss
