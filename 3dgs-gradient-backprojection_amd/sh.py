"""The SH colours of a training step: one HIP kernel forward, one backward (csrc/sh.hip).

    colors = sh_colors(degree, means, coeffs, campos)                  # [N,K,3] -> [N,3]
    colors = sh_colors(degree, means, features_dc, campos, rest=features_rest)   # the two tables as a splat dict stores them

What gsplat's spherical_harmonics followed by "+ 0.5, clamp at 0" gives, differentiable in the coefficients (both tables) and, through
the view direction, in means.  The forward has Engine.sh_colors' bits; the backward differentiates projection.sh_colors_torch, which stays
the yardstick.  Rows of the tables above (degree + 1)^2 are not read and receive exact zero gradients (not None: Adam sees zeros, as in
the reference trainer while its SH degree is still rising).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Union

import torch

from . import _lib
from ._lib import GwbpError, check
from .engine import sh_eval_tables, sh_eval_tables_backward, sh_eval_tables_backward_dev, sh_eval_tables_dev


def device_caller(device):
    def call(name: str, *args):
        fn = getattr(_lib.lib(), name)
        if device.index is None or torch.cuda.current_device() == device.index:
            check(fn(*args), name)
            return
        with torch.cuda.device(device):
            check(fn(*args), name)
    return call, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _ShColors(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, head, tail, degree, campos):
        call, stream = device_caller(means.device)
        out = sh_eval_tables(call, stream, degree, means, head, tail, campos)
        ctx.save_for_backward(means, head, tail)
        ctx.degree, ctx.campos = degree, campos
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v_colors):
        means, head, tail = ctx.saved_tensors
        want_means, want_head, want_tail = ctx.needs_input_grad[:3]
        empty_tail = tail is not None and tail.shape[1] == 0
        v_tail = torch.zeros_like(tail) if (want_tail and empty_tail) else None
        want_tail = want_tail and tail is not None and not empty_tail
        if ctx.degree == 0 and want_means and not (want_head or want_tail):
            return torch.zeros_like(means), None, v_tail, None, None  # (no dependence on the means at degree 0)
        v_head = v_means = None
        if want_head or want_tail or want_means:
            call, stream = device_caller(means.device)
            v_head, v_t, v_means = sh_eval_tables_backward(call, stream, ctx.degree, means, head, tail, ctx.campos, v_colors, want_head,
                                                           want_tail, want_means)
            v_tail = v_t if want_tail else v_tail
        return v_means, v_head, v_tail, None, None


class _ShColorsDev(torch.autograd.Function):
    """_ShColors with the centre a device tensor the kernels load, and a gradient to it (gwbp_sh_eval_dev and its backward)."""

    @staticmethod
    def forward(ctx, means, head, tail, degree, campos):
        call, stream = device_caller(means.device)
        out = sh_eval_tables_dev(call, stream, degree, means, head, tail, campos)
        ctx.save_for_backward(means, head, tail, campos)
        ctx.degree = degree
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v_colors):
        means, head, tail, campos = ctx.saved_tensors
        want_means, want_head, want_tail, _, want_campos = ctx.needs_input_grad
        empty_tail = tail is not None and tail.shape[1] == 0
        v_tail = torch.zeros_like(tail) if (want_tail and empty_tail) else None
        want_tail = want_tail and tail is not None and not empty_tail
        v_head = v_means = v_campos = None
        if want_head or want_tail or want_means or want_campos:
            call, stream = device_caller(means.device)
            v_head, v_t, v_means, v_campos = sh_eval_tables_backward_dev(call, stream, ctx.degree, means, head, tail, campos, v_colors,
                                                                         want_head, want_tail, want_means, want_campos)
            v_tail = v_t if want_tail else v_tail
            if v_campos is not None:
                v_campos = v_campos.to(torch.float32).reshape(campos.shape)
        return v_means, v_head, v_tail, None, v_campos


def sh_colors(degree: int, means: torch.Tensor, coeffs: torch.Tensor, campos: Union[torch.Tensor, Sequence[float]],
              rest: Optional[torch.Tensor] = None, campos_grad: bool = False) -> torch.Tensor:
    """[N,K,3] SH coefficients (K >= (degree + 1)^2, degree <= 3) -> [N,3] colours toward `campos`: + 0.5, clamped at 0; what
    sh_colors_torch computes, in one HIP kernel, and differentiable in coeffs, rest and means through one more.
    rest: the table's remaining rows [N,K',3] when it is stored in two parts (features_dc, features_rest): coefficient k is coeffs[:, k]
    for k < K and rest[:, k - K] behind; nothing is concatenated.  campos: three floats (a tensor is read on the host, detached).
    campos_grad=True: campos must be a float32 HIP tensor of three elements; the kernels load it on the device (no host read, the same
    bits for the same values), and where it requires grad it receives d loss / d campos = -sum_i v_means_i, summed in float64 in a
    fixed order and cast to float32.
    float32 HIP tensors only: anything else raises GwbpError (there is no CPU path)."""
    for name, t in (("means", means), ("coeffs", coeffs), ("rest", rest)):
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise GwbpError(f"sh_colors(): {name} must be a HIP tensor (there is no CPU path; sh_colors_torch is the torch form)")
        if t.dtype != torch.float32:
            raise GwbpError(f"sh_colors(): {name} must be float32, got {t.dtype}")
    if isinstance(degree, bool) or not isinstance(degree, int) or not 0 <= degree <= 3:
        raise GwbpError(f"sh_colors(): degree must be an int in [0, 3], got {degree!r}")
    if means.dim() != 2 or means.shape[1] != 3:
        raise GwbpError(f"sh_colors(): means must be [N,3], got {tuple(means.shape)}")
    for name, t in (("coeffs", coeffs), ("rest", rest)):
        if t is not None and (t.dim() != 3 or t.shape[2] != 3 or t.shape[0] != means.shape[0]):
            raise GwbpError(f"sh_colors(): {name} must be [N,K,3] with N = {means.shape[0]}, got {tuple(t.shape)}")
    k_head, k_rest = coeffs.shape[1], 0 if rest is None else rest.shape[1]
    if k_head < 1 or k_head + k_rest < (degree + 1) ** 2:
        raise GwbpError(f"sh_colors(): {k_head} + {k_rest} coefficients are fewer than the {(degree + 1) ** 2} of degree {degree}")
    # the kernels take rows of at most SH_MAX_K coefficients; wider tables are narrowed to what degree 3 can read, and autograd's
    # slice gives the columns behind their zeros
    if k_head > _lib.SH_MAX_K:
        coeffs, rest = coeffs[:, :_lib.SH_MAX_K], None if rest is None else rest[:, :0]
    elif k_head + k_rest > _lib.SH_MAX_K:
        rest = rest[:, :_lib.SH_MAX_K - k_head]
    if campos_grad:
        if not torch.is_tensor(campos) or not campos.is_cuda or campos.dtype != torch.float32 or campos.numel() != 3 \
                or campos.device != means.device:
            raise GwbpError("sh_colors(campos_grad=True): campos must be a float32 HIP tensor of three elements on the means' device")
        return _ShColorsDev.apply(means, coeffs, rest, degree, campos)
    cp = tuple(float(v) for v in (campos.detach().cpu().tolist() if torch.is_tensor(campos) else campos))
    if len(cp) != 3:
        raise GwbpError(f"sh_colors(): campos must hold three floats, got {len(cp)}")
    return _ShColors.apply(means, coeffs, rest, degree, cp)
