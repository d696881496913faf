"""What the modules that work on a finished lift share (transfer, pca, segment, label_render, fidelity, decoded_field): the checks of
their arguments, the C-ABI call on the caller's stream, and the two ways they reach a projected view -- front() for one view through
rasterization()'s engine and front cache, score_views() for a pass over many views with one capacity check behind it.
Nothing here is public API; pruning.gradient_mask and the lift drivers of backproject.py keep loops of their own.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable

import torch

from ._lib import GwbpError, check, lib
from .engine import MAP_TYPES as FIELD_TYPES  # dtype -> GWBP_MAP_*: a finished field has a feature map's element types
from .engine import Engine
from .engine import field_rows  # noqa: F401  (the Engine's own payload check; re-exported for the modules on a finished field)
from .engine import row_stride as ld  # noqa: F401
from .rasterization import get_engine, run_front

RASTER_KW = dict(near_plane=0.01, far_plane=1e10, eps2d=0.3, radius_clip=0.0, camera_model="pinhole", rasterize_mode="classic")


def raster_kw(fn: str, kw: dict) -> dict:
    """The projection keywords of fn()'s **raster_kw over their defaults; any other keyword is the caller's mistake."""
    unknown = set(kw) - set(RASTER_KW)
    if unknown:
        raise TypeError(f"{fn}() got unexpected keyword arguments {sorted(unknown)}")
    return dict(RASTER_KW, **kw)


def require_device(fn: str, means) -> None:
    if not means.is_cuda:
        raise GwbpError(f"{fn}() needs HIP tensors (there is no CPU path)")


def rows(t: torch.Tensor, name: str) -> torch.Tensor:
    """A [rows, D] float32 device tensor with unit stride inside a row and a non-negative row stride >= D, as the kernel reads it."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise GwbpError(f"{name} must be a HIP tensor (no CPU fallback exists for this path)")
    if t.dim() != 2 or t.shape[1] < 1:
        raise GwbpError(f"{name} must be [rows, D] with D >= 1, got {tuple(t.shape)}")
    if t.dtype in (torch.float16, torch.bfloat16):
        t = t.float()
    if t.dtype != torch.float32:
        raise GwbpError(f"{name} must be float32, float16 or bfloat16, got {t.dtype}")
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def out_type(fn: str, out_dtype):
    """(torch dtype, GWBP_MAP_* code) of an out_dtype keyword: None means float32."""
    dtype = torch.float32 if out_dtype is None else out_dtype
    if dtype not in FIELD_TYPES:
        raise GwbpError(f"{fn}: out_dtype must be None, float32, float16 or bfloat16, got {out_dtype!r}")
    return dtype, FIELD_TYPES[dtype]


def run(name: str, device, *args):
    fn = getattr(lib(), name)
    with torch.cuda.device(device):
        check(fn(*args, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), name)


def front(fn: str, means, quats, scales, opacities, viewmat, K, width, height, kw: dict, *, want_alphas: bool = False,
          want_store: bool = False):
    """(engine, view, alphas) with the view projected and sorted -- and blended with want_store -- on rasterization()'s engine,
    through its front cache: after a rendered frame of the same view and the same tensor objects nothing is launched.  kw: fn()'s
    **raster_kw as given.  alphas: the blend's [H, W] map with want_alphas (which needs the store), else None."""
    require_device(fn, means)
    kw = raster_kw(fn, kw)
    width, height = int(width), int(height)
    eng = get_engine(means.device, means.shape[0], width, height)
    view = eng.view(viewmat, K, width, height, **kw)
    alphas = run_front(eng, view, means, quats, scales, opacities, want_alphas, False, want_store=want_store)[2]
    return eng, view, alphas


def score_views(fn: str, means, quats, scales, opacities, viewmats, K, width, height, kw: dict, *, make_result: Callable,
                per_view: Callable, blend: bool):
    """One pass over the views of viewmats [V, 4, 4] (K: [3, 3] or [V, 3, 3]) on rasterization()'s engine with nothing inside that
    waits for the device: the workspace's capacity is checked once behind the loop, and an overflow grows the workspace and
    runs the views again into a fresh result.  make_result(): the zeroed result of one attempt.  per_view(eng, v, result) runs
    first for a view -- it is where the caller's callback is asked for the view's input -- and returns None to skip the view
    before anything is made or launched for it, else launch(view), which issues the view's kernel once the view is projected
    and sorted (and, with blend, its weight store written).  kw: fn()'s **raster_kw as given."""
    require_device(fn, means)
    kw = raster_kw(fn, kw)
    width, height = int(width), int(height)
    n_views = viewmats.shape[0]
    vm_host, K_host = viewmats.detach().cpu(), K.detach().cpu()
    eng = get_engine(means.device, means.shape[0], width, height)
    for _ in range(6):
        result = make_result()
        accum = torch.zeros(32, dtype=torch.uint8, device=means.device)
        eng.front_cache = None  # the workspace holds the last scored view from here on, and no stats of it
        for v in range(n_views):
            launch = per_view(eng, v, result)
            if launch is None:
                continue
            view = eng.view(vm_host[v], K_host if K_host.dim() == 2 else K_host[v], width, height, **kw)
            eng.project(view, means, quats, scales, opacities)
            eng.bin_sort(view)
            if blend:
                eng.blend_weights(view)
            eng.holds_new_view()
            launch(view)
            eng.accumulate_stats(accum)
        stats = Engine.decode_stats(accum)
        if not stats["overflow"]:
            return result
        eng.grow(stats, views=n_views)
    raise RuntimeError(f"{fn}: no pass over the views finished without a workspace overflow (flags {stats['overflow']})")
