"""Engine: a per-device workspace + thin methods over the C ABI stages (include/gwbp.h).

Everything is enqueued on torch's current HIP stream of the tensors' device; nothing synchronises except
`stats()` / `dump_pairs()` and the capacity auto-grow in `backproject_view(check=True)`.
"""
from __future__ import annotations

from ctypes import byref, c_double, c_float, c_int64, c_size_t, c_void_p
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import Caps, GwbpError, Stats, check, make_view, ptr

TILE = 16
# feature-map element types the scatter entry points take (GWBP_MAP_*); everything else the Engine computes in is float32
MAP_TYPES = {torch.float32: _lib.MAP_F32, torch.float16: _lib.MAP_F16, torch.bfloat16: _lib.MAP_BF16}
HALF_TYPES = (torch.float16, torch.bfloat16)
PIXEL_TOPK_MAX = 16      # GWBP_PIXEL_TOPK_MAX (gwbp_pixel_gaussians' list length)
PROBE_MAX_PIXELS = 4096  # GWBP_PROBE_MAX_PIXELS


def nearest_index(n_in: int, n_out: int) -> torch.Tensor:
    """Source index of every output index under torch.nn.functional.interpolate(mode="nearest"):
    min(floor(dst * scale), n_in - 1) with scale = n_in / n_out, all in fp32 (ATen UpSample.h
    nearest_neighbor_compute_source_index; the op the reference applies at backproject.py:244-248)."""
    if n_in < 1 or n_out < 1:
        raise ValueError("sizes must be positive")
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    idx = torch.floor(torch.arange(n_out, dtype=torch.float32) * scale).to(torch.int64).clamp_(max=n_in - 1)
    return idx.to(torch.int32)


def bilinear_index(n_in: int, n_out: int):
    """(lower source index int32[n_out], weight of the upper neighbour float32[n_out]) of
    torch.nn.functional.interpolate(mode="bilinear", align_corners=False), computed like ATen's
    area_pixel_compute_source_index in fp32: src = max(scale * (dst + 0.5) - 0.5, 0), scale = n_in / n_out
    (the op the reference applies at backproject.py:110-112)."""
    if n_in < 1 or n_out < 1:
        raise ValueError("sizes must be positive")
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    src = (scale * (torch.arange(n_out, dtype=torch.float32) + 0.5) - 0.5).clamp_(min=0.0)
    i0 = src.to(torch.int64).clamp_(max=n_in - 1)
    lam = (src - i0.to(torch.float32)).clamp_(0.0, 1.0)
    return i0.to(torch.int32), lam


# label-map element types gwbp_scatter_labels reads natively (GWBP_LABEL_*); a bool mask is read as its uint8 bytes
LABEL_TYPES = {torch.uint8: _lib.LABEL_U8, torch.bool: _lib.LABEL_U8, torch.int16: _lib.LABEL_I16, torch.int32: _lib.LABEL_I32}


# per-pixel weight-map element types the _ex blends read natively (GWBP_PIXW_*); a bool mask is read as its uint8 bytes, and
# GWBP_PIXW_U8 counts any non-zero byte as 1
PIXEL_WEIGHT_TYPES = {torch.float32: _lib.PIXW_F32, torch.float16: _lib.PIXW_F16, torch.bfloat16: _lib.PIXW_BF16,
                      torch.uint8: _lib.PIXW_U8, torch.bool: _lib.PIXW_U8}


def narrow_labels(labels: torch.Tensor, num_classes: int) -> torch.Tensor:
    """An int64 label map as the int32 map gwbp_scatter_labels reads: every id outside [0, num_classes) becomes -1 (ignored)
    BEFORE the narrowing, so that no wide id can wrap into range."""
    return torch.where((labels < 0) | (labels >= num_classes), -1, labels).to(torch.int32)


def _req(t: torch.Tensor, name: str, shape_tail=None) -> torch.Tensor:
    if not t.is_cuda:
        raise GwbpError(f"{name} must be a CUDA/HIP tensor (no CPU fallback exists for this path)")
    if t.dtype != torch.float32:
        raise GwbpError(f"{name} must be float32, got {t.dtype}")
    if shape_tail is not None and tuple(t.shape[1:]) != tuple(shape_tail):
        raise GwbpError(f"{name} has shape {tuple(t.shape)}, expected [N,{','.join(map(str, shape_tail))}]")
    return t.contiguous()


def _sh_tables(degree, means, head, tail):
    """(means, head, tail) as gwbp_sh_eval reads them: float32 HIP tensors, contiguous, [N,3], [N,K_head,3] and None or [N,K_tail,3]."""
    means = _req(means, "means", (3,))
    head = _req(head, "sh coefficients")
    tail = None if tail is None else _req(tail, "sh coefficients (tail)")
    for t in (head, tail):
        if t is not None and (t.dim() != 3 or t.shape[2] != 3 or t.shape[0] != means.shape[0] or t.device != means.device):
            raise GwbpError(f"SH coefficients must be [N,K,3] beside means [{means.shape[0]},3], got {tuple(t.shape)}")
    if tail is not None and tail.shape[1] == 0:
        tail = None
    if isinstance(degree, bool) or int(degree) != degree:
        raise GwbpError(f"the SH degree must be an int, got {degree!r}")
    return means, head, tail


def sh_eval_tables(call, stream, degree, means, head, tail, campos) -> torch.Tensor:
    """Engine.sh_eval for whoever brings the caller of the C ABI (call(name, *args)) and the stream handle."""
    means, head, tail = _sh_tables(degree, means, head, tail)
    out = torch.empty(means.shape[0], 3, device=means.device)
    cp = (c_float * 3)(*[float(v) for v in campos])
    call("gwbp_sh_eval", c_int64(means.shape[0]), int(degree), head.shape[1], 0 if tail is None else tail.shape[1], ptr(means), ptr(head),
         ptr(tail), cp, ptr(out), stream)
    return out


def sh_eval_tables_backward(call, stream, degree, means, head, tail, campos, v_colors, want_head, want_tail, want_means):
    """Engine.sh_eval_backward, likewise."""
    means, head, tail = _sh_tables(degree, means, head, tail)
    v_colors = _req(v_colors, "v_colors", (3,))
    if v_colors.shape[0] != means.shape[0]:
        raise GwbpError(f"v_colors must be [{means.shape[0]},3], got {tuple(v_colors.shape)}")
    v_head = torch.empty_like(head) if want_head else None
    v_tail = torch.empty_like(tail) if want_tail and tail is not None else None
    v_means = torch.empty_like(means) if want_means else None
    if v_head is None and v_tail is None and v_means is None:
        raise GwbpError("sh_eval_backward: no output asked for")
    cp = (c_float * 3)(*[float(v) for v in campos])
    call("gwbp_sh_eval_backward", c_int64(means.shape[0]), int(degree), head.shape[1], 0 if tail is None else tail.shape[1], ptr(means),
         ptr(head), ptr(tail), cp, ptr(v_colors), ptr(v_head), ptr(v_tail), ptr(v_means), stream)
    return v_head, v_tail, v_means


def _sh_campos_dev(campos, means) -> torch.Tensor:
    """The camera centre as gwbp_sh_eval_dev reads it: three float32 values on means' device, never read on the host."""
    if not torch.is_tensor(campos) or not campos.is_cuda or campos.dtype != torch.float32 or campos.numel() != 3 \
            or campos.device != means.device:
        raise GwbpError("the device camera centre must be a float32 HIP tensor of three elements on the means' device")
    return campos.detach().reshape(3).contiguous()


def sh_eval_tables_dev(call, stream, degree, means, head, tail, campos) -> torch.Tensor:
    """sh_eval_tables with the centre a device tensor (gwbp_sh_eval_dev): the same bits for the same three values."""
    means, head, tail = _sh_tables(degree, means, head, tail)
    cp = _sh_campos_dev(campos, means)
    out = torch.empty(means.shape[0], 3, device=means.device)
    call("gwbp_sh_eval_dev", c_int64(means.shape[0]), int(degree), head.shape[1], 0 if tail is None else tail.shape[1], ptr(means),
         ptr(head), ptr(tail), ptr(cp), ptr(out), stream)
    return out


def sh_eval_tables_backward_dev(call, stream, degree, means, head, tail, campos, v_colors, want_head, want_tail, want_means,
                                want_campos):
    """sh_eval_tables_backward with the centre a device tensor (gwbp_sh_eval_backward_dev): (v_head, v_tail, v_means, v_campos), the
    last float64 [3] = minus the fixed-order sum of the rows' v_means values."""
    means, head, tail = _sh_tables(degree, means, head, tail)
    cp = _sh_campos_dev(campos, means)
    v_colors = _req(v_colors, "v_colors", (3,))
    if v_colors.shape[0] != means.shape[0]:
        raise GwbpError(f"v_colors must be [{means.shape[0]},3], got {tuple(v_colors.shape)}")
    v_head = torch.empty_like(head) if want_head else None
    v_tail = torch.empty_like(tail) if want_tail and tail is not None else None
    v_means = torch.empty_like(means) if want_means else None
    v_campos = scratch = None
    if want_campos:
        blocks = int(_lib.lib().gwbp_sh_eval_backward_blocks(c_int64(means.shape[0])))
        if blocks < 0:
            check(blocks, "gwbp_sh_eval_backward_blocks")
        v_campos = torch.empty(3, dtype=torch.float64, device=means.device)
        scratch = torch.empty(max(blocks, 1), 3, dtype=torch.float64, device=means.device)
    if v_head is None and v_tail is None and v_means is None and v_campos is None:
        raise GwbpError("sh_eval_backward: no output asked for")
    call("gwbp_sh_eval_backward_dev", c_int64(means.shape[0]), int(degree), head.shape[1], 0 if tail is None else tail.shape[1],
         ptr(means), ptr(head), ptr(tail), ptr(cp), ptr(v_colors), ptr(v_head), ptr(v_tail), ptr(v_means), ptr(v_campos), ptr(scratch),
         stream)
    return v_head, v_tail, v_means, v_campos


def adam_scalars(step: int, lr: float, b1: float, b2: float):
    """(lr / (1 - b1^step), sqrt(1 - b2^step)) in float64, as torch's single-tensor Adam forms them on the host; the C ABI takes each
    rounded to float32 once."""
    return float(lr) / (1.0 - float(b1) ** int(step)), (1.0 - float(b2) ** int(step)) ** 0.5


def adam_step_tables(call, stream, p, g, m, v, visible, step: int, lr: float, b1: float, b2: float, eps: float) -> None:
    """Engine.adam_step for whoever brings the caller of the C ABI (call(name, *args)) and the stream handle."""
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise GwbpError(f"adam_step: {name} must be a HIP tensor (there is no CPU path)")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise GwbpError(f"adam_step: {name} must be a contiguous float32 tensor, got {t.dtype}, strides {tuple(t.stride())}")
        if t.shape != p.shape or t.device != p.device:
            raise GwbpError(f"adam_step: {name} is {tuple(t.shape)} on {t.device} beside p {tuple(p.shape)} on {p.device}")
    if isinstance(step, bool) or int(step) != step or step < 1:
        raise GwbpError(f"adam_step: the step count must be a positive int, got {step!r}")
    n = int(p.shape[0]) if p.dim() else 1
    w = p.numel() // n if n else 1
    if n == 0 or w == 0:
        return
    if visible is not None:
        if (not torch.is_tensor(visible) or visible.dtype not in (torch.uint8, torch.bool) or visible.device != p.device
                or tuple(visible.shape) != (n,) or not visible.is_contiguous()):
            raise GwbpError(f"adam_step: visible must be a contiguous uint8 or bool tensor [{n}] on {p.device}")
        visible = visible.view(torch.uint8)
    step_size, sqrt_bc2 = adam_scalars(step, lr, b1, b2)
    call("gwbp_adam_step", c_int64(n), int(w), ptr(p), ptr(g), ptr(m), ptr(v), ptr(visible), c_float(step_size), c_float(sqrt_bc2),
         c_double(float(b1)), c_double(float(b2)), c_float(float(eps)), stream)


def depth_image_args(fn: str, render, alpha, channel: int):
    """(render, alpha [H, W], H, W, Dp, ch) of a depth loss: render a float32 HIP tensor [H, W, Dp], alpha [H, W] or [H, W, 1] on the same
    device, channel an index into Dp (negative: from the end).  Both are read in place; another layout than a dense one is copied."""
    for name, t in (("render", render), ("alpha", alpha)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise GwbpError(f"{fn}: {name} must be a HIP tensor (there is no CPU path)")
        if t.dtype != torch.float32:
            raise GwbpError(f"{fn}: {name} must be float32, got {t.dtype}")
    if render.dim() != 3 or render.shape[0] < 1 or render.shape[1] < 1 or render.shape[2] < 1:
        raise GwbpError(f"{fn}: render must be [H, W, D'] with H, W, D' >= 1, got {tuple(render.shape)}")
    H, W, Dp = (int(v) for v in render.shape)
    if tuple(alpha.shape) not in ((H, W), (H, W, 1)) or alpha.device != render.device:
        raise GwbpError(f"{fn}: alpha must be [{H}, {W}] or [{H}, {W}, 1] on {render.device}, got {tuple(alpha.shape)} on {alpha.device}")
    if isinstance(channel, bool) or not isinstance(channel, int) or not -Dp <= channel < Dp:
        raise GwbpError(f"{fn}: channel must be an int in [{-Dp}, {Dp}), got {channel!r}")
    return render.contiguous(), alpha.reshape(H, W).contiguous(), H, W, Dp, channel % Dp


def depth_point_args(fn: str, render, points, depths):
    """(points [M, 2], depths [M], M) of the point term: float32 tensors on the render's device."""
    for name, t in (("points", points), ("depths", depths)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise GwbpError(f"{fn}: {name} must be a HIP tensor (there is no CPU path)")
        if t.dtype != torch.float32 or t.device != render.device:
            raise GwbpError(f"{fn}: {name} must be float32 on {render.device}, got {t.dtype} on {t.device}")
    if points.dim() != 2 or points.shape[1] != 2 or tuple(depths.shape) != (points.shape[0],):
        raise GwbpError(f"{fn}: points must be [M, 2] and depths [M], got {tuple(points.shape)} and {tuple(depths.shape)}")
    return points.contiguous(), depths.contiguous(), int(points.shape[0])


def depth_map_args(fn: str, render, depth, weights, kind: str):
    """(depth [H, W], weights [H, W] or None, GWBP_DEPTH_KIND_*) of the map term: float32 tensors on the render's device."""
    if kind not in _lib.DEPTH_KINDS:
        raise GwbpError(f"{fn}: kind must be one of {list(_lib.DEPTH_KINDS)}, got {kind!r}")
    H, W = int(render.shape[0]), int(render.shape[1])
    for name, t in (("depth", depth), ("weights", weights)):
        if t is None and name == "weights":
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise GwbpError(f"{fn}: {name} must be a HIP tensor (there is no CPU path)")
        if t.dtype != torch.float32 or t.device != render.device or tuple(t.shape) != (H, W):
            raise GwbpError(f"{fn}: {name} must be float32 [{H}, {W}] on {render.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return depth.contiguous(), (None if weights is None else weights.contiguous()), _lib.DEPTH_KINDS[kind]


def field_rows(t: torch.Tensor, name: str):
    """(tensor, GWBP_MAP_* code) of a finished [rows, D] FIELD as it is stored: float32, float16 or bfloat16, read by the *_typed entry
    points without a float32 copy.  Unit stride inside a row and a non-negative row stride >= D, in elements; a layout the kernels
    cannot read is made contiguous in the tensor's own dtype."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise GwbpError(f"{name} must be a HIP tensor (no CPU fallback exists for this path)")
    if t.dim() != 2 or t.shape[1] < 1:
        raise GwbpError(f"{name} must be [rows, D] with D >= 1, got {tuple(t.shape)}")
    if t.dtype not in MAP_TYPES:
        raise GwbpError(f"{name} must be float32, float16 or bfloat16, got {t.dtype}")
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, MAP_TYPES[t.dtype]


def row_stride(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])  # (the stride of a single row means nothing)


class Engine:
    """Workspace sized for (N Gaussians, max WxH, isect_cap, pair_cap) on one device."""

    def __init__(self, n_gaussians: int, max_width: int, max_height: int, device=None,
                 isect_cap: Optional[int] = None, pair_cap: Optional[int] = None, scatter_workgroups: int = 0,
                 tight_binning: bool = False):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise GwbpError("Engine needs a HIP device (there is no CPU path)")
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.lib = _lib.lib()
        self._maps: Dict[Tuple[int, int, int, int], Tuple[torch.Tensor, torch.Tensor]] = {}
        self.n = int(n_gaussians)
        self.max_w, self.max_h = int(max_width), int(max_height)
        # Defaults: ~16 tiles per Gaussian and ~128 weights per pixel; both auto-grow on overflow.
        self.isect_cap = int(isect_cap or max(1 << 18, 16 * self.n))
        self.pair_cap = int(pair_cap or max(1 << 20, 128 * self.max_w * self.max_h))
        self.scatter_workgroups = int(scatter_workgroups)  # 0 = one persistent scatter workgroup per CU
        # tight_binning: GWBP_FLAG_TIGHT_BINNING -- same F, d, weights and renders, shorter tile lists; off by default
        # because meta["isect_ids"] of the drop-in operator must show gsplat's 3-sigma binning
        self.tight_binning = bool(tight_binning)
        self._halves = False  # the workspace holds the half-tile lists + weight sums of the view blended last
        self._tokens = None   # (h, w) of the map whose token-quadrant weight sums the workspace holds (blend_tokens)
        self.stream, self._stream_handle = None, None
        self.generation, self.front_cache = 0, None  # see holds_new_view
        self._alloc()

    def holds_new_view(self, front_cache: Optional[dict] = None) -> None:
        """The workspace holds another view now; whoever projects one into it says so.  rasterization()'s backwards compare `generation`
        with their forward's (a missed count is a silently wrong gradient); `front_cache` is run_front's record of its view, or None."""
        self.generation, self.front_cache = self.generation + 1, front_cache

    def _set_flag(self, bit: int, on: bool) -> None:
        if on:
            self.caps.flags |= bit
        else:
            self.caps.flags &= ~bit

    def set_front_priority(self, on: bool) -> None:
        """GWBP_FLAG_FRONT_PRIORITY for this engine's project / bin_sort / blend_weights launches: raised wave priority.
        Only useful when they run on a second stream beside a D % 256 == 0 scatter (ViewPipeline sets it)."""
        self._set_flag(_lib.FLAG_FRONT_PRIORITY, on)

    def set_split_encoder(self, on: bool) -> None:
        """GWBP_FLAG_SPLIT_ENCODER: blend_scatter_encoded as ONE persistent launch of encoder (producer) waves and blend (consumer)
        waves around an LDS ring of encoded tiles (the compressed variant on large images, see gwbp.h)."""
        self._set_flag(_lib.FLAG_SPLIT_ENCODER, on)

    def set_narrow_scatter(self, on: bool) -> None:
        """GWBP_FLAG_NARROW_SCATTER: the 128-channel scatter kernel even when D % 256 == 0 (short records, see gwbp.h).
        An Engine starts narrow (k_blend then skips the half-tile lists only the 256-channel kernel reads); whoever
        knows that a D % 256 == 0 scatter follows switches it off BEFORE blend_weights of that view (ViewPipeline,
        the drop-in operator)."""
        self._set_flag(_lib.FLAG_NARROW_SCATTER, on)

    def _alloc(self):
        # run-time flags survive a re-allocation (grow); a new engine starts narrow
        run = (self.caps.flags & (_lib.FLAG_FRONT_PRIORITY | _lib.FLAG_NARROW_SCATTER | _lib.FLAG_SPLIT_ENCODER)
               if hasattr(self, "caps") else _lib.FLAG_NARROW_SCATTER)
        base = _lib.FLAG_TIGHT_BINNING if self.tight_binning else 0
        self.caps = Caps(self.n, self.isect_cap, self.pair_cap, self.max_w, self.max_h, self.scatter_workgroups, base | run)
        nbytes = c_size_t(0)
        self._call("gwbp_workspace_size", byref(self.caps), byref(nbytes))
        self.ws_bytes = int(nbytes.value)
        self.ws = torch.empty(self.ws_bytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self.ws.data_ptr()) % 256
        self._ws_ptr = c_void_p(self.ws.data_ptr() + off)

    def grow(self, stats: Dict[str, int], views: int = 1):
        """Enlarge whichever capacity overflowed (bit0 = isect, bit1 = pairs) and reallocate.  The pair counter keeps
        counting after the pool is exhausted, so the weight store can be sized for what the views really needed
        (`stats` summed over `views` views)."""
        if stats["overflow"] & 1:
            self.isect_cap *= 2
        if stats["overflow"] & 2:
            self.pair_cap = max(2 * self.pair_cap, int(2.5 * stats["n_pairs"] / max(1, views)) + (1 << 16))
        del self.ws
        self._alloc()

    # ---- helpers -----------------------------------------------------------------------------------------
    def _stream(self):
        if self.stream is not None:  # bound by a driver that keeps this engine on one stream (no context switch per call)
            return self._stream_handle
        return c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def bind_stream(self, stream: Optional[torch.cuda.Stream]):
        """Launch this engine's kernels on `stream` whatever torch's current stream is (None: follow the current stream).
        Methods that allocate outputs (want_alphas, render, ...) still allocate on the current stream."""
        self.stream = stream
        self._stream_handle = c_void_p(stream.cuda_stream) if stream is not None else None

    def _call(self, name: str, *args):
        """One C-ABI call with this engine's device current: libgwbp launches on the CURRENT HIP device, while the
        workspace, the tensors and the stream handle belong to self.device (a process may hold engines on several)."""
        fn = getattr(self.lib, name)
        if torch.cuda.current_device() == self._dev_index:  # the usual case: no device switch (a context manager costs
            check(fn(*args), name)                           # ~10 us per call, and small scenes are host-bound)
            return
        with torch.cuda.device(self.device):
            check(fn(*args), name)

    def _args(self):
        return byref(self.caps), self._ws_ptr, c_size_t(self.ws_bytes)

    def _on_stream(self):
        """Context in which torch allocates and computes on the stream this engine's kernels run on: the bound stream, or, with none
        bound (torch.cuda.stream(None) changes nothing), torch's current one."""
        return torch.cuda.stream(self.stream)

    def _alphas(self, view, want: bool) -> Optional[torch.Tensor]:
        """The [H, W] alpha map a blend writes when asked for it."""
        return torch.empty(view.height, view.width, device=self.device) if want else None

    def _widen(self, feats: torch.Tensor) -> torch.Tensor:
        """A half map for a kernel that reads float32 only: feats.float() (exact), made on the stream the kernel runs on.
        What it costs is that of the copy: one read of the map, one write and one read of twice its size."""
        if feats.dtype not in HALF_TYPES:
            return feats
        with self._on_stream():
            return feats.float()

    def half_native(self, feats: torch.Tensor) -> bool:
        """Does scatter() read this fp16 / bf16 map as it is (gwbp_scatter_typed and its upsampled / bilinear forms)?  The
        256-channel kernel takes D % 256 == 0 with unit channel stride; the 128-channel kernel (D % 128 == 0, and D % 256 == 0
        with set_narrow_scatter(True)) also needs pixel strides that are multiples of 8 elements and a 16-B aligned map.
        Other half maps are widened with .float() at the call."""
        if feats.dim() != 3 or feats.dtype not in HALF_TYPES:
            return False
        sy, sx, sc = feats.stride()
        D = feats.shape[2]
        if sc != 1 or D % 128 != 0 or min(sy, sx) < 0:
            return False
        if D % 256 == 0 and not (self.caps.flags & _lib.FLAG_NARROW_SCATTER):
            return True
        return sy % 8 == 0 and sx % 8 == 0 and feats.data_ptr() % 16 == 0

    def view(self, viewmat, K, width, height, **kw):
        """make_view: near_plane, far_plane, eps2d, radius_clip, camera_model ("pinhole" | "ortho" | "fisheye") and
        rasterize_mode ("classic" | "antialiased") as keywords."""
        return make_view(viewmat, K, int(width), int(height), **kw)

    # ---- stages ------------------------------------------------------------------------------------------
    def project(self, view, means, quats, scales, opacities, want_outputs=False):
        """Projection of `view` under the camera model and rasterize mode it carries (Engine.view / make_view): the default
        pinhole / classic view issues gwbp_project, any other gwbp_project_camera; every later stage of the view reads the
        projected table either writes.  want_outputs: radii, means2d, depths, conics -- and, under antialiased, compensations."""
        means, quats = _req(means, "means", (3,)), _req(quats, "quats", (4,))
        scales, opacities = _req(scales, "scales", (3,)), _req(opacities, "opacities")
        if means.shape[0] != self.n:
            raise GwbpError(f"engine was sized for {self.n} Gaussians, got {means.shape[0]}")
        model, mode = _lib.camera_of(view)
        out = {}
        if want_outputs:
            out = dict(radii=torch.empty(self.n, dtype=torch.int32, device=self.device),
                       means2d=torch.empty(self.n, 2, device=self.device),
                       depths=torch.empty(self.n, device=self.device),
                       conics=torch.empty(self.n, 3, device=self.device))
            if mode == "antialiased":
                out["compensations"] = torch.empty(self.n, device=self.device)
        if model == "pinhole" and mode == "classic":
            self._call("gwbp_project", *self._args(), byref(view), ptr(means), ptr(quats), ptr(scales),
                                        ptr(opacities), ptr(out.get("radii")), ptr(out.get("means2d")),
                                        ptr(out.get("depths")), ptr(out.get("conics")), self._stream())
            return out
        self._call("gwbp_project_camera", *self._args(), byref(view), _lib.CAMERA_MODELS[model],
                   _lib.RASTERIZE_MODES[mode], ptr(means), ptr(quats), ptr(scales), ptr(opacities), ptr(out.get("radii")),
                   ptr(out.get("means2d")), ptr(out.get("depths")), ptr(out.get("conics")), ptr(out.get("compensations")),
                   self._stream())
        return out

    def bin_sort(self, view, want_outputs=False):
        out = {}
        if want_outputs:
            nt = -(-view.width // TILE) * -(-view.height // TILE)
            out = dict(isect_ids=torch.empty(self.isect_cap, dtype=torch.int64, device=self.device),
                       flatten_ids=torch.empty(self.isect_cap, dtype=torch.int32, device=self.device),
                       tile_offsets=torch.empty(nt + 1, dtype=torch.int32, device=self.device))
        self._call("gwbp_bin_sort", *self._args(), byref(view), ptr(out.get("isect_ids")),
                                     ptr(out.get("flatten_ids")), ptr(out.get("tile_offsets")), self._stream())
        return out

    def _wide_requested(self) -> bool:
        return not (self.caps.flags & _lib.FLAG_NARROW_SCATTER)

    def blend_weights(self, view, want_alphas=False, d=None, scale_d=1.0):
        """d (optional, float32[N]): also add this view's denominators d[g] += scale_d * sum_p w_g(p) from inside the blend
        (gwbp_blend_weights_d; needs the 256-channel scatter kernel enabled, like accumulate_d)."""
        alphas = self._alphas(view, want_alphas)
        self._tokens = None
        self._halves = self._wide_requested()  # k_blend<HALVES> writes the lists only without NARROW_SCATTER
        if d is not None:
            self._check_denominator(d)
            self._need_weight_sums("blend_weights", blend=True)
            self._call("gwbp_blend_weights_d", *self._args(), byref(view), ptr(alphas), c_float(scale_d), ptr(d),
                       self._stream())
            return alphas
        self._call("gwbp_blend_weights", *self._args(), byref(view), ptr(alphas), self._stream())
        return alphas

    # ---- per-pixel weight maps (masks, confidences): the _ex blends ---------------------------------------------------
    def pixel_weights(self, c: torch.Tensor, view) -> _lib.PixelWeights:
        """The gwbp_pixel_weights of a [view.height, view.width] weight map on this engine's device: bool, uint8 (non-zero = 1),
        float16, bfloat16 or float32, any non-negative strides (a channel of an [H, W, C] tensor works).  Raises GwbpError on
        anything else.  The returned struct points into `c`: keep `c` alive until the blend that reads it has run."""
        if not torch.is_tensor(c):
            raise GwbpError(f"pixel weights must be a tensor, got {type(c).__name__}")
        if c.dtype not in PIXEL_WEIGHT_TYPES:
            raise GwbpError(f"pixel weights must be bool, uint8, float16, bfloat16 or float32, got {c.dtype}")
        if not c.is_cuda or c.device.index != self._dev_index:
            raise GwbpError(f"pixel weights must be on the engine's device cuda:{self._dev_index}, got {c.device}")
        if tuple(c.shape) != (view.height, view.width):
            raise GwbpError(f"pixel weights must be [H,W] = [{view.height},{view.width}], got {tuple(c.shape)}")
        if min(c.stride()) < 0:
            raise GwbpError("negative pixel-weight strides are not supported")
        pw = _lib.PixelWeights()
        pw.data = c.data_ptr() or None
        pw.ws_y, pw.ws_x = c.stride()
        pw.dtype = PIXEL_WEIGHT_TYPES[c.dtype]
        pw.reserved = 0
        return pw

    def blend_weighted(self, view, pixel_weights: torch.Tensor, want_alphas=False, d=None, scale_d=1.0):
        """blend_weights with a per-pixel weight map c (gwbp_blend_weights_ex / _d_ex): the store holds w c(p) for the pixels with
        c(p) != 0 only, so every scatter of the view (scatter, scatter_labels, accumulate_d, ...) adds
        F[g] += scale_f sum_p w_g(p) c(p) f(p), d[g] += scale_d sum_p w_g(p) c(p).  The alpha map is the unweighted one."""
        pw = self.pixel_weights(pixel_weights, view)
        alphas = self._alphas(view, want_alphas)
        self._tokens = None
        self._halves = self._wide_requested()
        if d is not None:
            self._check_denominator(d)
            self._need_weight_sums("blend_weighted", blend=True)
            self._call("gwbp_blend_weights_d_ex", *self._args(), byref(view), ptr(alphas), c_float(scale_d), ptr(d),
                       byref(pw), self._stream())
            return alphas
        self._call("gwbp_blend_weights_ex", *self._args(), byref(view), ptr(alphas), byref(pw), self._stream())
        return alphas

    def blend_tokens_weighted(self, view, lr_h: int, lr_w: int, pixel_weights: torch.Tensor, want_alphas=False):
        """blend_tokens with a per-pixel weight map (gwbp_blend_tokens_ex): the token-quadrant sums are sums of w c(p)."""
        pw = self.pixel_weights(pixel_weights, view)
        if not self.token_geometry_ok(lr_h, lr_w, view.height, view.width):
            raise GwbpError(f"blend_tokens_weighted: a {lr_h}x{lr_w} map has texels narrower than a tile at "
                            f"{view.height}x{view.width}; use blend_weighted + scatter(upsample='nearest')")
        ymap, xmap = self.nearest_maps(lr_h, lr_w, view.height, view.width)
        alphas = self._alphas(view, want_alphas)
        self._halves = False
        self._tokens = (int(lr_h), int(lr_w))
        self._call("gwbp_blend_tokens_ex", *self._args(), byref(view), ptr(ymap), ptr(xmap), ptr(alphas), byref(pw),
                   self._stream())
        return alphas

    def blend_scatter_weighted(self, view, feats, pixel_weights: torch.Tensor, F, d, scale_f=1.0, scale_d=1.0, want_alphas=False):
        """blend_scatter with a per-pixel weight map (gwbp_blend_scatter_ex)."""
        pw = self.pixel_weights(pixel_weights, view)
        if not self.can_blend_scatter(feats):
            raise GwbpError(f"blend_scatter_weighted: [H,W,D] map with unit channel stride and D <= "
                            f"{self.fused_max_dim(view.width, view.height)} required, got {tuple(feats.shape)}")
        feats = self._widen(feats)
        sy, sx, _, D = self._feat_strides(feats, view)
        self._check_acc(F, d, D)
        alphas = self._alphas(view, want_alphas)
        self._halves, self._tokens = False, None
        self._call("gwbp_blend_scatter_ex", *self._args(), byref(view), ptr(feats), sy, sx, D, c_float(scale_f),
                   c_float(scale_d), ptr(F), ptr(d), ptr(alphas), byref(pw), self._stream())
        return alphas

    def blend_scatter_encoded_weighted(self, view, feats, encoder, pixel_weights: torch.Tensor, F, d, scale_f=1.0, scale_d=1.0,
                                       want_alphas=False):
        """blend_scatter_encoded with a per-pixel weight map (gwbp_blend_scatter_encoded_ex)."""
        pw = self.pixel_weights(pixel_weights, view)
        if not self.can_blend_scatter_encoded(feats, encoder):
            raise GwbpError("blend_scatter_encoded_weighted: [H,W,K] channel-contiguous 16-B aligned map, K % 16 == 0, "
                            f"16 <= K <= 512, <= 16 outputs required, got {tuple(feats.shape)} @ {tuple(encoder.shape)}")
        if feats.shape[0] != view.height or feats.shape[1] != view.width:
            raise GwbpError(f"feature map must be [{view.height},{view.width},K], got {tuple(feats.shape)}")
        feats = self._widen(feats)
        sy, sx, _ = feats.stride()
        K, n = encoder.shape
        self._check_acc(F, d, n)
        enc = encoder.contiguous()
        alphas = self._alphas(view, want_alphas)
        self._halves, self._tokens = False, None
        self._call("gwbp_blend_scatter_encoded_ex", *self._args(), byref(view), ptr(feats), sy, sx, K, ptr(enc), n,
                   c_float(scale_f), c_float(scale_d), ptr(F), ptr(d), ptr(alphas), byref(pw), self._stream())
        return alphas

    FUSED_MAX_DIM = 16         # gwbp_blend_scatter holds 4 pixels x 16 channels per lane in registers ...
    FUSED_MAX_DIM_SMALL = 32   # ... or, on images of at most FUSED_SMALL_TILES tiles, one pixel x 32 channels (a wave per
    FUSED_SMALL_TILES = 4096   # quarter tile: four short blend chains per tile instead of one long one)

    @classmethod
    def fused_max_dim(cls, width: int, height: int) -> int:
        tiles = (-(-int(width) // 16)) * (-(-int(height) // 16))
        return cls.FUSED_MAX_DIM_SMALL if tiles <= cls.FUSED_SMALL_TILES else cls.FUSED_MAX_DIM

    @classmethod
    def can_blend_scatter(cls, feats: torch.Tensor) -> bool:
        """Maps gwbp_blend_scatter takes: [H,W,D] float32 at full resolution, D <= 16 (<= 32 on small images), unit channel
        stride, non-negative strides.  (fp16 / bf16 maps of that shape too: blend_scatter widens them with .float().)"""
        return (feats.dim() == 3 and feats.is_cuda and feats.dtype in MAP_TYPES
                and 1 <= feats.shape[2] <= cls.fused_max_dim(feats.shape[1], feats.shape[0])
                and feats.stride(2) == 1 and min(feats.stride()) >= 0)

    def blend_scatter(self, view, feats, F, d, scale_f=1.0, scale_d=1.0, want_alphas=False):
        """blend_weights + scatter of one view in ONE kernel for narrow maps (D <= 16: the compressed variant after its
        encoder, backproject_compressed.py:127-165): the tile's pixels sit in registers while it is blended, each
        contributing record is reduced across the wave and added to F / d at once.  No weight store is written: the
        view cannot be scattered or rendered again without a new blend_weights().  A half map is widened with .float()
        first (the kernel reads float32)."""
        if not self.can_blend_scatter(feats):
            raise GwbpError(f"blend_scatter: [H,W,D] float32 map with unit channel stride and D <= {self.FUSED_MAX_DIM} "
                            f"(<= {self.FUSED_MAX_DIM_SMALL} on images of at most {self.FUSED_SMALL_TILES} tiles) required, "
                            f"got {tuple(feats.shape)} strides {tuple(feats.stride())}")
        feats = self._widen(feats)
        sy, sx, _, D = self._feat_strides(feats, view)
        self._check_acc(F, d, D)
        alphas = self._alphas(view, want_alphas)
        self._halves, self._tokens = False, None  # the store is empty: no scatter kernel has anything to read
        self._call("gwbp_blend_scatter", *self._args(), byref(view), ptr(feats), sy, sx, D, c_float(scale_f),
                   c_float(scale_d), ptr(F), ptr(d), ptr(alphas), self._stream())
        return alphas

    @staticmethod
    def can_blend_scatter_encoded(feats: torch.Tensor, encoder: torch.Tensor) -> bool:
        """Shapes gwbp_blend_scatter_encoded takes: [H,W,K] float32 with channel-contiguous 16-B aligned pixels, K % 16 == 0,
        16 <= K <= 512, at most 16 outputs (the reference's encoder is 512 -> 16, backproject_compressed.py:26,127).  fp16 / bf16
        maps of that shape and layout too: blend_scatter_encoded widens them with .float()."""
        if not Engine._encoder_layout(feats, encoder, 512):
            return False
        K, n = encoder.shape
        sx = feats.stride(1)
        # (a row must span less than 4 GB: the kernel's per-lane column offsets are 32-bit -- a channel slice of a much wider
        # tensor falls back to encode_map, like any other layout the kernel does not take)
        return n >= 1 and K >= 16 and sx >= K and ((feats.shape[1] - 1) * sx + K) * 4 < (1 << 32)

    def blend_scatter_encoded(self, view, feats, encoder, F, d, scale_f=1.0, scale_d=1.0, want_alphas=False):
        """blend_scatter(view, feats @ encoder, ...) of the compressed variant (backproject_compressed.py:127-165) in ONE
        kernel: every tile's wave streams its 256 pixels x K channels once through the matrix cores (exact fp32, the same
        chain as encode_map) into the registers the fused blend + scatter works from -- no [H,W,n] map, no encoder kernel, no
        weight store."""
        if not self.can_blend_scatter_encoded(feats, encoder):
            raise GwbpError("blend_scatter_encoded: [H,W,K] float32 channel-contiguous 16-B aligned map, K % 16 == 0, "
                            f"16 <= K <= 512, <= 16 outputs required, got {tuple(feats.shape)} strides {tuple(feats.stride())} "
                            f"@ {tuple(encoder.shape)}")
        if feats.shape[0] != view.height or feats.shape[1] != view.width:
            raise GwbpError(f"feature map must be [{view.height},{view.width},K], got {tuple(feats.shape)}")
        feats = self._widen(feats)
        sy, sx, _ = feats.stride()
        K, n = encoder.shape
        self._check_acc(F, d, n)
        enc = encoder.contiguous()
        alphas = self._alphas(view, want_alphas)
        self._halves, self._tokens = False, None  # the store is empty: no scatter kernel has anything to read
        self._call("gwbp_blend_scatter_encoded", *self._args(), byref(view), ptr(feats), sy, sx, K, ptr(enc), n,
                   c_float(scale_f), c_float(scale_d), ptr(F), ptr(d), ptr(alphas), self._stream())
        return alphas

    @staticmethod
    def _feat_strides(feats: torch.Tensor, view, lowres: bool = False) -> Tuple[int, int, int, int]:
        if feats.dim() != 3 or (not lowres and (feats.shape[0] != view.height or feats.shape[1] != view.width)):
            raise GwbpError(f"feature map must be [H,W,D] = [{view.height},{view.width},D], got {tuple(feats.shape)}")
        if feats.dtype not in MAP_TYPES or not feats.is_cuda:
            raise GwbpError(f"feature map must be a float32, float16 or bfloat16 HIP tensor, got {feats.dtype}")
        sy, sx, sc = feats.stride()
        if min(sy, sx, sc) < 0:
            raise GwbpError("negative feature-map strides are not supported")
        return sy, sx, sc, feats.shape[2]

    # ---- token space: the dino variant's nearest-upsampled patch-token map (backproject.py:242-249) ------------------
    TOKEN_MIN_DIM = 64  # gwbp_scatter_tokens: one float4 per lane and 256-channel chunk; narrower maps leave 3/4 of a wave idle
    TOKEN_MAX_VIEW = 4096  # ... and keeps per-tile-column / -row tables of 256 entries in LDS (token.hip kTokMaxTiles)

    _TOKEN_GEOMETRY: Dict[Tuple[int, int, int, int], bool] = {}

    @classmethod
    def token_geometry_ok(cls, lr_h: int, lr_w: int, height: int, width: int) -> bool:
        """Does every 16 x 16 tile of a height x width view see at most 2 x 2 texels of an lr_h x lr_w map under
        F.interpolate(mode="nearest")?  Checked on the exact index maps (PyTorch's fp32 rule), tile by tile: the precondition
        of gwbp_blend_tokens.  True whenever a texel is at least a tile wide and high (the 64 x 64 dino tokens at 1600 x 1060)."""
        key = (int(lr_h), int(lr_w), int(height), int(width))
        ok = cls._TOKEN_GEOMETRY.get(key)
        if ok is None:
            ok = True
            for n_in, n_out in ((key[0], key[2]), (key[1], key[3])):
                m = nearest_index(n_in, n_out).to(torch.int64)
                first = m[0::TILE]
                last = m[torch.clamp(torch.arange(0, n_out, TILE) + TILE - 1, max=n_out - 1)]
                ok = ok and int((last - first).max()) <= 1
            cls._TOKEN_GEOMETRY[key] = ok
        return ok

    @classmethod
    def can_scatter_tokens(cls, tokens: torch.Tensor, height: int, width: int) -> bool:
        """Low-resolution maps the token-space path takes: [h, w, D] float32, float16 or bfloat16 on the device, D % 4 == 0 and
        D >= 64 (the 384 / 768 / 1024 / 1536 channels of the DINOv2 backbones), channel-contiguous rows whose strides are multiples
        of 4 elements, a 16-B aligned map, texels at least a tile wide and high (token_geometry_ok), views of at most 4096 x 4096
        pixels.  Anything else goes through blend_weights + scatter(upsample="nearest")."""
        if tokens.dim() != 3 or not tokens.is_cuda or tokens.dtype not in MAP_TYPES:
            return False
        if max(int(height), int(width)) > cls.TOKEN_MAX_VIEW:
            return False
        sy, sx, sc = tokens.stride()
        D = tokens.shape[2]
        return (D >= cls.TOKEN_MIN_DIM and D % 4 == 0 and sc == 1 and sy % 4 == 0 and sx % 4 == 0 and sy >= 0
                and sx >= D and tokens.data_ptr() % 16 == 0
                and cls.token_geometry_ok(tokens.shape[0], tokens.shape[1], int(height), int(width)))

    def blend_tokens(self, view, lr_h: int, lr_w: int, want_alphas=False):
        """blend_weights for a view whose feature map is an lr_h x lr_w map upsampled with mode="nearest" (the dino variant):
        instead of a weight store the blend leaves, per contributing (Gaussian, tile) record, the weight sums of the tile's
        2 x 2 tokens (gwbp_blend_tokens); scatter_tokens() consumes them.  Same weights, same alpha map."""
        if not self.token_geometry_ok(lr_h, lr_w, view.height, view.width):
            raise GwbpError(f"blend_tokens: a {lr_h}x{lr_w} map has texels narrower than a tile at {view.height}x{view.width}; "
                            "use blend_weights + scatter(upsample='nearest')")
        ymap, xmap = self.nearest_maps(lr_h, lr_w, view.height, view.width)
        alphas = self._alphas(view, want_alphas)
        self._halves = False  # no weight store: only scatter_tokens can consume this view
        self._tokens = (int(lr_h), int(lr_w))
        self._call("gwbp_blend_tokens", *self._args(), byref(view), ptr(ymap), ptr(xmap), ptr(alphas), self._stream())
        return alphas

    def scatter_tokens(self, view, tokens, F, d, scale_f=1.0, scale_d=1.0):
        """F[g,:] += scale_f * sum_t omega_{g,t} tokens[t,:], d[g] += scale_d * sum_t omega_{g,t} from the sums blend_tokens left:
        equals scatter(view, tokens, F, d, upsample="nearest") up to summation order, with one plain read-modify-write of every
        row that receives weight (no atomics: deterministic) and the token map read from L2 / Infinity Cache.  fp16 / bf16 tokens
        are read as they are and widened in the kernel: F and d equal those of tokens.float() bit for bit."""
        if getattr(self, "_tokens", None) != (int(tokens.shape[0]), int(tokens.shape[1])):
            raise GwbpError("scatter_tokens needs blend_tokens(view, h, w) of the same view and map size first")
        if not self.can_scatter_tokens(tokens, view.height, view.width):
            raise GwbpError(f"scatter_tokens: [h,w,D] float32 / float16 / bfloat16 map with D % 4 == 0, D >= 64, channel-contiguous 16-B aligned rows and texels "
                            f"of at least a tile at a view of at most {self.TOKEN_MAX_VIEW} x {self.TOKEN_MAX_VIEW} pixels required, got "
                            f"{tuple(tokens.shape)} strides {tuple(tokens.stride())} at {view.width} x {view.height}")
        D = tokens.shape[2]
        self._check_acc(F, d, D)
        ymap, xmap = self.nearest_maps(tokens.shape[0], tokens.shape[1], view.height, view.width)
        sy, sx, _ = tokens.stride()
        if tokens.dtype in HALF_TYPES:
            self._call("gwbp_scatter_tokens_typed", *self._args(), byref(view), ptr(tokens), MAP_TYPES[tokens.dtype],
                       c_int64(sy), c_int64(sx), D, ptr(ymap), ptr(xmap), c_float(scale_f), c_float(scale_d), ptr(F),
                       ptr(d), self._stream())
            return
        self._call("gwbp_scatter_tokens", *self._args(), byref(view), ptr(tokens), c_int64(sy), c_int64(sx), D, ptr(ymap),
                   ptr(xmap), c_float(scale_f), c_float(scale_d), ptr(F), ptr(d), self._stream())

    def accumulate_d(self, view, d, scale_d=1.0):
        """d += scale_d * sum_p w from the blend's per-record weight sums (needs a blend with the wide scatter enabled)."""
        self._check_denominator(d)
        self._need_weight_sums("accumulate_d")
        self._call("gwbp_accumulate_d", *self._args(), byref(view), c_float(scale_d), ptr(d), self._stream())

    def has_weight_sums(self) -> bool:
        """The view in the workspace was blended with the 256-channel scatter kernel enabled: its records carry their weight
        sums (accumulate_d, scatter_uniform)."""
        return bool(self._halves)

    def scatter_uniform(self, view, value: torch.Tensor, F: torch.Tensor) -> None:
        """F[g, :] += value * sum_p w_g(p): the scatter of a map whose every entry is `value` (a 0-d float32 HIP tensor, read
        on the device), from the per-record weight sums -- the backward of `render.sum()`, which is what the reference's
        denominator pass asks for (backproject.py:145-147).  Needs has_weight_sums()."""
        self._need_weight_sums("scatter_uniform")
        if F.dtype != torch.float32 or not F.is_cuda or F.dim() != 2 or F.shape[0] != self.n:
            raise GwbpError(f"F must be a float32 HIP tensor [{self.n},D]")
        sums = torch.zeros(self.n, device=self.device, dtype=torch.float32)
        saved = self.caps.flags  # (the flag says which kernel the NEXT blend serves; the sums of THIS view are there)
        self.caps.flags = saved & ~_lib.FLAG_NARROW_SCATTER
        try:
            self.accumulate_d(view, sums)
        finally:
            self.caps.flags = saved
        F.add_(sums[:, None] * value.to(torch.float32))

    def scatter(self, view, feats, F, d, scale_f=1.0, scale_d=1.0, upsample: Optional[str] = None):
        """F += scale_f * sum_p w feats[p], d += scale_d * sum_p w from the view's weight store.

        upsample="nearest" / "bilinear": feats is a LOW-RESOLUTION map [h,w,D]; the result equals scattering
        F.interpolate(feats, size=(H,W), mode=...) (dino: backproject.py:244-248; lseg: backproject.py:110-112,
        align_corners=False) without building that map -- the interpolation happens while the tile slabs are staged.

        feats may be float32, float16 or bfloat16.  A half map that half_native() admits is read as it is and widened to fp32
        while the slabs are staged: F and d equal those of feats.float() up to the order of the atomic sums.  Any other half map
        (D <= 64 or not a multiple of 128, fs_c != 1, misaligned for the 128-channel kernel) is widened with .float() here."""
        if self._tokens is not None:
            raise GwbpError("this view was blended with blend_tokens (no weight store): scatter_tokens() is its consumer; "
                            "blend_weights() first for scatter()")
        if self._wide_requested() and not self._halves:
            # This view was blended WITH GWBP_FLAG_NARROW_SCATTER (no half-tile lists): the 256-channel kernel would read
            # another view's tables.  Scatter it with the 128-channel kernel, which needs only the headers every blend writes.
            saved = self.caps.flags
            self.caps.flags = saved | _lib.FLAG_NARROW_SCATTER
            try:
                return self.scatter(view, feats, F, d, scale_f, scale_d, upsample)
            finally:
                self.caps.flags = saved
        if feats.dtype in HALF_TYPES:
            if not self.half_native(feats):
                return self.scatter(view, self._widen(feats), F, d, scale_f, scale_d, upsample)
            return self._scatter_half(view, feats, F, d, scale_f, scale_d, upsample)
        if upsample is None:
            sy, sx, sc, D = self._feat_strides(feats, view)
            self._check_acc(F, d, D)
            self._call("gwbp_scatter", *self._args(), byref(view), ptr(feats), c_int64(sy), c_int64(sx),
                                        c_int64(sc), D, c_float(scale_f), c_float(scale_d), ptr(F), ptr(d),
                                        self._stream())
            return
        if upsample not in ("nearest", "bilinear"):
            raise GwbpError(f"upsample must be None, 'nearest' or 'bilinear', got {upsample!r}")
        sy, sx, sc, D = self._feat_strides(feats, view, lowres=True)
        self._check_acc(F, d, D)
        if upsample == "bilinear":
            y0, ly, x0, lx = self.bilinear_maps(feats.shape[0], feats.shape[1], view.height, view.width)
            self._call("gwbp_scatter_bilinear", *self._args(), byref(view), ptr(feats), c_int64(sy),
                                                 c_int64(sx), c_int64(sc), D, int(feats.shape[0]),
                                                 int(feats.shape[1]), ptr(y0), ptr(ly), ptr(x0), ptr(lx),
                                                 c_float(scale_f), c_float(scale_d), ptr(F), ptr(d),
                                                 self._stream())
            return
        ymap, xmap = self.nearest_maps(feats.shape[0], feats.shape[1], view.height, view.width)
        self._call("gwbp_scatter_upsampled", *self._args(), byref(view), ptr(feats), c_int64(sy), c_int64(sx),
                                              c_int64(sc), D, ptr(ymap), ptr(xmap), c_float(scale_f),
                                              c_float(scale_d), ptr(F), ptr(d), self._stream())

    def scatter_labels(self, view, labels, F, d, num_classes: int, scale_f=1.0, scale_d=1.0, upsample: Optional[str] = None):
        """F[g, k] += scale_f * sum_p w_g(p) [labels[p] == k], d[g] += scale_d * sum_p w_g(p) from the view's weight store: scatter()
        of one_hot(labels, num_classes) without the one-hot map (gwbp_scatter_labels: one atomic per record and distinct label).
        A label outside [0, num_classes) adds to no column of F; its weight still counts in d.

        labels: [H, W] uint8 / bool / int16 / int32 read as stored, any non-negative strides; int64 is narrowed first
        (narrow_labels).  upsample="nearest": a LOW-RESOLUTION [h, w] map read through F.interpolate(mode="nearest")'s index maps.
        F: float32 [N, num_classes] with unit column stride (its row stride may be wider); d: float32 [N] or None."""
        if self._tokens is not None:
            raise GwbpError("this view was blended with blend_tokens (no weight store): blend_weights() first for scatter_labels()")
        labels, ymap, xmap, K = self._class_args(view, labels, F, "F", d, "d", num_classes, upsample)
        sy, sx = labels.stride()
        self._call("gwbp_scatter_labels", *self._args(), byref(view), ptr(labels), LABEL_TYPES[labels.dtype], c_int64(sy),
                   c_int64(sx), K, ptr(ymap), ptr(xmap), c_float(scale_f), c_float(scale_d), ptr(F), c_int64(F.stride(0)),
                   ptr(d), self._stream())

    def _label_map(self, view, labels, num_ids: int, upsample: Optional[str]):
        """(label map as the kernels read it, ymap, xmap) of scatter_labels, the votes and scatter_mask_features: an [H, W] map --
        with upsample="nearest" an [h, w] map and F.interpolate(mode="nearest")'s index maps -- of uint8 / int16 / int32 with
        non-negative strides on the device; bool is read as its bytes, int64 narrowed to the ids in [0, num_ids) (narrow_labels).
        The map may be a narrowed copy: the caller holds it until its kernel is enqueued."""
        if not torch.is_tensor(labels) or not labels.is_cuda:
            raise GwbpError("labels must be a HIP tensor (no CPU fallback exists for this path)")
        if labels.dtype == torch.int64:
            labels = narrow_labels(labels, num_ids)
        if labels.dtype not in LABEL_TYPES:
            raise GwbpError(f"labels must be an integer map (uint8, bool, int16, int32 or int64), got {labels.dtype}")
        if labels.dtype == torch.bool:
            labels = labels.view(torch.uint8)
        if upsample not in (None, "nearest"):
            raise GwbpError(f"upsample must be None or 'nearest' for a label map, got {upsample!r}")
        if labels.dim() != 2 or (upsample is None and tuple(labels.shape) != (view.height, view.width)):
            want = f"[H,W] = [{view.height},{view.width}]" if upsample is None else "[h,w]"
            raise GwbpError(f"label map must be {want}, got {tuple(labels.shape)}")
        if min(labels.stride()) < 0:
            raise GwbpError("negative label-map strides are not supported")
        ymap = xmap = None
        if upsample == "nearest":
            ymap, xmap = self.nearest_maps(labels.shape[0], labels.shape[1], view.height, view.width)
        return labels, ymap, xmap

    def _class_args(self, view, labels, acc, acc_name: str, den, den_name: str, num_classes: int, upsample: Optional[str]):
        """(label map as read, ymap, xmap, K) of scatter_labels (acc = F, den = d) and of the two votes (C, n), validated alike; the
        names go into the messages."""
        K = int(num_classes)
        if K < 1:
            raise GwbpError(f"num_classes must be positive, got {K}")
        labels, ymap, xmap = self._label_map(view, labels, K, upsample)
        self._check_class_acc(acc, acc_name, K)
        if den is not None:
            self._check_denominator(den, den_name)
        return labels, ymap, xmap, K

    # ---- per-view votes of label maps (gwbp_vote_labels, gwbp_vote_projected) -----------------------------------------------
    @staticmethod
    def vote_words(num_classes: int) -> int:
        """uint32 words per Gaussian of gwbp_vote_labels' bitset: bit 0 = "seen", label k = bit k + 1."""
        return (int(num_classes) + 1 + 31) // 32

    def _vote_seen(self, num_classes: int) -> torch.Tensor:
        """The bitset of gwbp_vote_labels, [N * vote_words(K)] int32: allocated zeroed on first use (grown with K) on the stream
        this engine's kernels run on, and kept all zero by the commit kernel after every call."""
        need = self.n * self.vote_words(num_classes)
        if getattr(self, "_seen", None) is None or self._seen.numel() < need:
            with self._on_stream():
                self._seen = torch.zeros(max(need, 1), dtype=torch.int32, device=self.device)
        return self._seen

    def vote_labels(self, view, labels, C, n, num_classes: int, upsample: Optional[str] = None):
        """Binary vote of one view from its weight store (gwbp_vote_labels): C[g, k] += 1 if Gaussian g has at least one
        contributing pixel (w > 0) of label k, n[g] += 1 if it has any contributing pixel.  A label outside [0, num_classes)
        counts in n and in no column.  labels, upsample: as scatter_labels.  C: float32 [N, num_classes] with unit column stride;
        n: float32 [N] or None.  Needs blend_weights / blend_weighted / blend_weights_rgb of the view (a pixel of weight 0 then
        casts no vote)."""
        if self._tokens is not None:
            raise GwbpError("this view was blended with blend_tokens (no weight store): blend_weights() first for vote_labels()")
        labels, ymap, xmap, K = self._class_args(view, labels, C, "C", n, "n", num_classes, upsample)
        seen = self._vote_seen(K)
        sy, sx = labels.stride()
        self._call("gwbp_vote_labels", *self._args(), byref(view), ptr(labels), LABEL_TYPES[labels.dtype],
                   c_int64(sy), c_int64(sx), ptr(ymap), ptr(xmap), K, ptr(seen), ptr(C),
                   c_int64(C.stride(0)), ptr(n), self._stream())

    def vote_projected(self, view, labels, C, n, num_classes: int, upsample: Optional[str] = None,
                       pixel_weights: Optional[torch.Tensor] = None):
        """Projection vote of one view from its projected table (gwbp_vote_projected; needs project() of the view only): a
        Gaussian with radius > 0 whose centre, rounded half to even, lies in the image adds 1 to C[g, label there] (if that label
        is in [0, num_classes)) and to n[g].  pixel_weights (optional, [H, W] at full resolution, as blend_weighted): a Gaussian
        whose pixel has a weight that is not > 0 casts no vote.  labels, upsample, C, n: as vote_labels."""
        labels, ymap, xmap, K = self._class_args(view, labels, C, "C", n, "n", num_classes, upsample)
        pw = byref(self.pixel_weights(pixel_weights, view)) if pixel_weights is not None else None
        sy, sx = labels.stride()
        self._call("gwbp_vote_projected", *self._args(), byref(view), ptr(labels), LABEL_TYPES[labels.dtype],
                   c_int64(sy), c_int64(sx), ptr(ymap), ptr(xmap), pw, K, ptr(C), c_int64(C.stride(0)),
                   ptr(n), self._stream())

    # ---- the integer walks of the mask association (gwbp_label_overlap, gwbp_label_votes; associate.py) ----------------------
    def _assoc_args(self, what: str, view, labels, num_labels: int, upsample, aux, aux_name: str, aux_len: int, acc, acc_name: str,
                    acc_rows: int):
        """(label map as read, ymap, xmap, K, n_cols) of label_overlap (aux = group [N], acc = O [K + 1, n_cols]) and label_votes
        (aux = remap [K], acc = V [N, n_cols]): the map through _label_map, the int32 table and the int64 accumulator checked."""
        if self._tokens is not None:
            raise GwbpError(f"this view was blended with blend_tokens (no weight store): blend_weights() first for {what}()")
        K = int(num_labels)
        if K < 1:
            raise GwbpError(f"num_labels must be positive, got {K}")
        labels, ymap, xmap = self._label_map(view, labels, K, upsample)
        rows, n = int(acc_rows), int(aux_len)
        if (not torch.is_tensor(acc) or acc.dtype != torch.int64 or not acc.is_cuda or acc.dim() != 2 or acc.shape[0] != rows
                or acc.shape[1] < 1 or (acc.shape[1] > 1 and acc.stride(1) != 1) or acc.stride(0) < acc.shape[1]):
            raise GwbpError(f"{acc_name} must be an int64 HIP tensor [{rows}, n_cols] with unit column stride")
        if (not torch.is_tensor(aux) or aux.dtype != torch.int32 or not aux.is_cuda or not aux.is_contiguous()
                or tuple(aux.shape) != (n,)):
            raise GwbpError(f"{aux_name} must be a contiguous int32 HIP tensor [{n}]")
        return labels, ymap, xmap, K, int(acc.shape[1])

    def label_overlap(self, view, labels, group, O, num_labels: int, upsample: Optional[str] = None):
        """O[row, group[g] + 1] += q(w) over the view's weight store (gwbp_label_overlap), q the fixed-point weight of
        associate.quantize_weights: row = labels[p] if it lies in [0, num_labels), else num_labels (the ignored pixels' row);
        group: int32 [N], -1 (or anything outside [-1, n_cols - 2]) = column 0, "not yet assigned".  O: int64
        [num_labels + 1, n_cols] with unit column stride, ADDED to.  Integer sums: the same bits on every run.  labels, upsample: as
        scatter_labels."""
        labels, ymap, xmap, K, n_cols = self._assoc_args("label_overlap", view, labels, num_labels, upsample, group, "group", self.n,
                                                         O, "O", int(num_labels) + 1)
        sy, sx = labels.stride()
        self._call("gwbp_label_overlap", *self._args(), byref(view), ptr(labels), LABEL_TYPES[labels.dtype], c_int64(sy),
                   c_int64(sx), K, ptr(ymap), ptr(xmap), ptr(group), n_cols, ptr(O), c_int64(O.stride(0)), self._stream())

    def label_votes(self, view, labels, remap, V, num_labels: int, upsample: Optional[str] = None):
        """V[g, remap[labels[p]]] += q(w) over the view's weight store (gwbp_label_votes).  remap: int32 [num_labels] with values in
        [-1, n_cols); a label outside [0, num_labels) or a negative entry adds nothing.  V: int64 [N, n_cols] with unit column
        stride, ADDED to.  Integer sums, as label_overlap."""
        labels, ymap, xmap, K, n_cols = self._assoc_args("label_votes", view, labels, num_labels, upsample, remap, "remap", int(num_labels),
                                                         V, "V", self.n)
        sy, sx = labels.stride()
        self._call("gwbp_label_votes", *self._args(), byref(view), ptr(labels), LABEL_TYPES[labels.dtype], c_int64(sy),
                   c_int64(sx), K, ptr(ymap), ptr(xmap), ptr(remap), n_cols, ptr(V), c_int64(V.stride(0)), self._stream())

    def label_votes_sparse(self, view, labels, remap, sv, num_labels: int, upsample: Optional[str] = None):
        """label_votes into per-Gaussian slot lists (gwbp_label_votes_sparse; sparse_votes.py): q(w) goes to the slot of row g whose
        key is remap[labels[p]] -- the first empty slot takes the key for good -- or to sv.spill[g] when the row's S slots hold
        other keys; with sv.total every non-zero q also counts in total[g], whatever its label.  Any remap entry >= 0 is a key:
        there is no column count.  sv: a SparseVotes (new_sparse_votes) -- keys int32 [N, S] (-1 empty) and vals int64 [N, S] with
        unit column stride and 1 <= S <= 32, spill int64 [N], total int64 [N] or None, none sharing memory; ADDED to.  Integer
        sums: without spill a row holds exactly the dense row's non-zero entries on every run, in a slot order that may differ."""
        keys, vals, spill, total = sv
        if not torch.is_tensor(vals) or vals.dim() != 2 or not 1 <= vals.shape[1] <= _lib.SPARSE_MAX_SLOTS:
            raise GwbpError(f"vals must be an int64 HIP tensor [{self.n}, S] with 1 <= S <= {_lib.SPARSE_MAX_SLOTS} slots")
        labels, ymap, xmap, K, S = self._assoc_args("label_votes_sparse", view, labels, num_labels, upsample, remap, "remap",
                                                    int(num_labels), vals, "vals", self.n)
        if (not torch.is_tensor(keys) or keys.dtype != torch.int32 or not keys.is_cuda or tuple(keys.shape) != (self.n, S)
                or (S > 1 and keys.stride(1) != 1) or keys.stride(0) < S):
            raise GwbpError(f"keys must be an int32 HIP tensor [{self.n}, {S}] (the shape of vals) with unit column stride")
        for t, name in ((spill, "spill"), (total, "total")):
            if t is None and name == "total":
                continue
            if (not torch.is_tensor(t) or t.dtype != torch.int64 or not t.is_cuda or tuple(t.shape) != (self.n,)
                    or not t.is_contiguous()):
                raise GwbpError(f"{name} must be a contiguous int64 HIP tensor [{self.n}]" + (" or None" if name == "total" else ""))
        sy, sx = labels.stride()
        self._call("gwbp_label_votes_sparse", *self._args(), byref(view), ptr(labels), LABEL_TYPES[labels.dtype], c_int64(sy),
                   c_int64(sx), K, ptr(ymap), ptr(xmap), ptr(remap), S, ptr(keys), c_int64(keys.stride(0)), ptr(vals),
                   c_int64(vals.stride(0)), ptr(spill), ptr(total), self._stream())

    @staticmethod
    def mask_fast_path(dim: int) -> bool:
        """Table widths gwbp_scatter_mask_features takes (every other width materialises table[labels], see
        scatter_mask_features)."""
        return dim >= 4 and dim % 4 == 0

    def _mask_buffers(self):
        """(slot store, spill counter) of gwbp_scatter_mask_features: allocated on first use, again after grow(); made on the stream
        this engine's kernels run on (one buffer serves every view of this engine: its views are scattered in stream order)."""
        need = self.isect_cap * _lib.MASK_SLOT_BYTES
        if getattr(self, "_mask_slots", None) is None or self._mask_slots.numel() < need:
            with self._on_stream():
                self._mask_slots = torch.empty(need, dtype=torch.uint8, device=self.device)
                if getattr(self, "mask_spilled", None) is None:
                    self.mask_spilled = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._mask_slots, self.mask_spilled

    def scatter_mask_features(self, view, labels, table, F, d, scale_f=1.0, scale_d=1.0, upsample: Optional[str] = None):
        """F[g, :] += scale_f * sum_p w_g(p) table[labels[p], :], d[g] += scale_d * sum_p w_g(p) from the view's weight store: scatter()
        of the materialised map table[labels] (a zero row where a label is outside [0, M)) without building it
        (gwbp_scatter_mask_features: per-record label sums filed at the emit positions, then ONE read-modify-write of every F row
        that receives weight).  Records with more than four distinct labels add the rest with atomics and count in
        `mask_spilled` (a device int32 counter of this engine, never reset here).

        labels: [H, W] (with upsample="nearest": [h, w]) uint8 / bool / int16 / int32 read as stored, any non-negative strides;
        int64 is narrowed first (narrow_labels).  table: [M, D] float32, float16 or bfloat16 with unit channel stride; a half
        table is widened as it is read (F equals that of table.float()).  F: float32 [N, D] contiguous; d: float32 [N] or None.
        A D that is no multiple of 4 (mask_fast_path) builds table[labels] and calls scatter(): same F and d."""
        if self._tokens is not None:
            raise GwbpError("this view was blended with blend_tokens (no weight store): blend_weights() first for "
                            "scatter_mask_features()")
        if not torch.is_tensor(labels) or not labels.is_cuda or not torch.is_tensor(table) or not table.is_cuda:
            raise GwbpError("labels and table must be HIP tensors (no CPU fallback exists for this path)")
        if table.dim() != 2 or table.dtype not in MAP_TYPES or table.shape[0] < 1 or table.shape[1] < 1:
            raise GwbpError(f"table must be a float32 / float16 / bfloat16 [M, D] tensor with M, D >= 1, got "
                            f"{table.dtype} {tuple(table.shape)}")
        if table.shape[1] > 1 and table.stride(1) != 1:
            raise GwbpError("table must have unit channel stride")
        M, D = int(table.shape[0]), int(table.shape[1])
        labels, ymap, xmap = self._label_map(view, labels, M, upsample)
        if F.dtype != torch.float32 or not F.is_cuda or F.dim() != 2 or tuple(F.shape) != (self.n, D) or not F.is_contiguous():
            raise GwbpError(f"F must be a contiguous float32 HIP tensor [{self.n},{D}]")
        if d is not None:
            self._check_denominator(d)
        if not self.mask_fast_path(D) or F.data_ptr() % 16:
            # the map the fast path avoids: a zero row wherever a label is outside [0, M)
            idx = labels.to(torch.int64)
            ok = ((idx >= 0) & (idx < M)).unsqueeze(-1)
            feats = torch.where(ok, table[idx.clamp(0, M - 1)], torch.zeros((), dtype=table.dtype, device=table.device))
            return self.scatter(view, feats, F, d, scale_f, scale_d, upsample=upsample)
        align = 16 if table.dtype == torch.float32 else 8
        if table.stride(0) % 4 or table.data_ptr() % align:
            table = table.contiguous() if not table.is_contiguous() else table.clone()  # (a fresh allocation is 256-B aligned)
        slots, spilled = self._mask_buffers()
        sy, sx = labels.stride()
        self._call("gwbp_scatter_mask_features", *self._args(), byref(view), ptr(labels), LABEL_TYPES[labels.dtype],
                   c_int64(sy), c_int64(sx), ptr(ymap), ptr(xmap), ptr(table), MAP_TYPES[table.dtype],
                   c_int64(table.stride(0) if M > 1 else D), M, D, c_float(scale_f), c_float(scale_d), ptr(F), ptr(d),
                   ptr(slots), c_size_t(slots.numel()), ptr(spilled), self._stream())

    def _scatter_half(self, view, feats, F, d, scale_f, scale_d, upsample):
        """scatter() of a half map that half_native() admits: the typed entry points."""
        if upsample not in (None, "nearest", "bilinear"):
            raise GwbpError(f"upsample must be None, 'nearest' or 'bilinear', got {upsample!r}")
        sy, sx, sc, D = self._feat_strides(feats, view, lowres=upsample is not None)
        self._check_acc(F, d, D)
        head = (*self._args(), byref(view), ptr(feats), MAP_TYPES[feats.dtype], c_int64(sy), c_int64(sx), c_int64(sc), D)
        tail = (c_float(scale_f), c_float(scale_d), ptr(F), ptr(d), self._stream())
        if upsample is None:
            self._call("gwbp_scatter_typed", *head, *tail)
        elif upsample == "bilinear":
            y0, ly, x0, lx = self.bilinear_maps(feats.shape[0], feats.shape[1], view.height, view.width)
            self._call("gwbp_scatter_bilinear_typed", *head, int(feats.shape[0]), int(feats.shape[1]), ptr(y0), ptr(ly), ptr(x0),
                       ptr(lx), *tail)
        else:
            ymap, xmap = self.nearest_maps(feats.shape[0], feats.shape[1], view.height, view.width)
            self._call("gwbp_scatter_upsampled_typed", *head, ptr(ymap), ptr(xmap), *tail)

    @staticmethod
    def _encoder_layout(feats: torch.Tensor, encoder: torch.Tensor, max_k: int) -> bool:
        """What the three encoder kernels (gwbp_encode_map, gwbp_scatter_encoded, gwbp_blend_scatter_encoded) ask alike of
        feats [H,W,K] @ encoder [K,n]: a float32 / float16 / bfloat16 map on the device with channel-contiguous 16-B aligned pixels
        (non-negative pixel strides that are multiples of 4 elements), a float32 encoder, K % 16 == 0, K <= max_k, n <= 16.  Each
        can_* predicate adds what only its kernel asks."""
        if feats.dim() != 3 or encoder.dim() != 2 or feats.shape[2] != encoder.shape[0]:
            return False
        sy, sx, sc = feats.stride()
        K, n = encoder.shape
        return (feats.is_cuda and feats.dtype in MAP_TYPES and encoder.dtype == torch.float32 and n <= 16
                and K % 16 == 0 and K <= max_k and sc == 1 and sy % 4 == 0 and sx % 4 == 0 and sy >= 0 and sx >= 0
                and feats.data_ptr() % 16 == 0)

    @staticmethod
    def can_fuse_encoder(feats: torch.Tensor, encoder: torch.Tensor) -> bool:
        """Shapes gwbp_scatter_encoded takes: [H,W,K] float32 with channel-contiguous 16-B aligned pixels, K % 16 == 0,
        K <= 1024, at most 16 outputs.  (fp16 / bf16 maps of that shape and layout too: scatter_encoded widens them.)"""
        return Engine._encoder_layout(feats, encoder, 1024) and encoder.shape[0] >= 16

    def scatter_encoded(self, view, feats, encoder, F, d, scale_f=1.0, scale_d=1.0):
        """scatter(view, feats @ encoder, ...) of the compressed variant (backproject_compressed.py:127-165) in ONE kernel:
        the [H,W,K] map is read once, tile by tile, and multiplied by the encoder while the slabs are staged.  A half map is
        widened with .float() first (the fused encoder reads float32)."""
        if not self.can_fuse_encoder(feats, encoder):
            raise GwbpError("scatter_encoded: [H,W,K] float32 channel-contiguous map, K % 16 == 0, K <= 1024, <= 16 outputs")
        if feats.shape[0] != view.height or feats.shape[1] != view.width:
            raise GwbpError(f"feature map must be [{view.height},{view.width},K], got {tuple(feats.shape)}")
        feats = self._widen(feats)
        sy, sx, _ = feats.stride()
        K, n = encoder.shape
        self._check_acc(F, d, n)
        enc = encoder.contiguous()
        self._call("gwbp_scatter_encoded", *self._args(), byref(view), ptr(feats), sy, sx, K, ptr(enc), n,
                   c_float(scale_f), c_float(scale_d), ptr(F), ptr(d), self._stream())

    def bilinear_maps(self, h: int, w: int, H: int, W: int):
        """device maps of F.interpolate(mode="bilinear", align_corners=False): (y0[H], ly[H], x0[W], lx[W]); cached."""
        key = ("bilinear", h, w, H, W)
        m = self._maps.get(key)
        if m is None:
            (y0, ly), (x0, lx) = bilinear_index(h, H), bilinear_index(w, W)
            m = tuple(t.to(self.device) for t in (y0, ly, x0, lx))
            self._maps[key] = m
        return m

    def nearest_maps(self, h: int, w: int, H: int, W: int):
        """int32 device index maps of F.interpolate(mode="nearest"): (ymap[H], xmap[W]); cached per geometry."""
        key = (h, w, H, W)
        m = self._maps.get(key)
        if m is None:
            m = tuple(nearest_index(i, o).to(self.device) for i, o in ((h, H), (w, W)))
            self._maps[key] = m
        return m

    def render(self, view, colors, out_dtype=None):
        """out [H, W, D] = the render of the table `colors` [N, D] from the view's weight store (gwbp_render_typed).  colors: float32,
        float16 or bfloat16, read as stored at any row stride >= D -- a half table gives the bits of colors.float(), without that copy.
        out_dtype (None = float32, float16, bfloat16): a half out is the float32 render rounded once to nearest even, out32.to(dtype)
        bit for bit."""
        colors, ct = field_rows(colors, "colors")
        if (out_dtype or torch.float32) not in MAP_TYPES:
            raise GwbpError(f"render: out_dtype must be float32, float16 or bfloat16, got {out_dtype}")
        D = colors.shape[1]
        out = torch.empty(view.height, view.width, D, dtype=out_dtype or torch.float32, device=self.device)
        self._call("gwbp_render_typed", *self._args(), byref(view), ptr(colors), ct, c_int64(row_stride(colors)), D, ptr(out),
                   MAP_TYPES[out.dtype], self._stream())
        return out

    def field_compare(self, view, features, fmap, index=None, want_planes=True, table=None):
        """The field `features` [N, D] (float32, float16 or bfloat16, any row stride >= D, read as stored: a half field gives the bits of
        features.float() without that copy) rendered from the view's weight store and
        compared with the view's map inside the kernel (gwbp_field_compare): needs project + bin_sort + blend_weights of `view`,
        like render().  Returns (planes, table): planes float32 [6, H, W] = dot, rr, mm, l1, l2, cosine of the rendered row r and
        the map row m per pixel (None with want_planes=False: no plane is written), table float64 [8] on the device = sum cosine,
        sum l1, sum l2, sum mm (over the valid pixels), n_valid, n_bad, n_pixels, D.
        fmap: [H, W, D] float32 / float16 / bfloat16 with unit channel stride and non-negative pixel strides, read as stored; with
        index = (ymap int32 [H], xmap int32 [W]) (nearest_maps) a low-resolution [h, w, D] map read through them.
        table: a float64 [8] device tensor to fill (a row of a [V, 8] table) instead of a new one."""
        if self._tokens is not None:
            raise GwbpError("this view was blended with blend_tokens (no weight store): blend_weights() first for field_compare()")
        features, ft = field_rows(features, "features")
        if features.shape[0] != self.n:
            raise GwbpError(f"engine was sized for {self.n} Gaussians, the field has {features.shape[0]} rows")
        D = features.shape[1]
        if not 1 <= D <= 2048:
            raise GwbpError(f"D must be in [1, 2048], got {D}")
        ld = row_stride(features)
        sy, sx, sc, Dm = self._feat_strides(fmap, view, lowres=index is not None)
        if Dm != D:
            raise GwbpError(f"the field has D = {D}, the map D = {Dm}")
        if D > 1 and sc != 1:
            raise GwbpError("the map's channels must be contiguous (unit last stride)")
        if fmap.device.index != self._dev_index:
            raise GwbpError(f"the map must be on the engine's device cuda:{self._dev_index}, got {fmap.device}")
        ymap = xmap = None
        lr_h = lr_w = 0
        if index is not None:
            ymap, xmap = index
            for t, n, name in ((ymap, view.height, "ymap [H]"), (xmap, view.width, "xmap [W]")):
                if (not torch.is_tensor(t) or t.dtype != torch.int32 or not t.is_cuda or tuple(t.shape) != (n,)
                        or not t.is_contiguous()):
                    raise GwbpError(f"index must be (ymap [H], xmap [W]) contiguous int32 HIP tensors; bad {name}")
            lr_h, lr_w = int(fmap.shape[0]), int(fmap.shape[1])
        if table is None:
            table = torch.empty(8, dtype=torch.float64, device=self.device)
        elif (not torch.is_tensor(table) or table.dtype != torch.float64 or not table.is_cuda or tuple(table.shape) != (8,)
              or not table.is_contiguous()):
            raise GwbpError("table must be a contiguous float64 [8] HIP tensor")
        planes = torch.empty(6, view.height, view.width, device=self.device) if want_planes else None
        self._call("gwbp_field_compare_typed", *self._args(), byref(view), ptr(features), ft, c_int64(ld), D, ptr(fmap),
                   MAP_TYPES[fmap.dtype], c_int64(sy), c_int64(sx), lr_h, lr_w, ptr(ymap), ptr(xmap), ptr(planes), ptr(table),
                   self._stream())
        return planes, table

    def _decode_workspace(self, d: int, D: int):
        """The slice partials of gwbp_decode_loss: a function of (d, D) alone, kept between calls (one buffer serves every call of
        this engine: they run in stream order), made on the stream this engine's kernels run on."""
        need = c_size_t(0)
        self._call("gwbp_decode_loss_workspace_size", d, D, byref(need))
        ws = getattr(self, "_decode_ws", None)
        if ws is None or ws.numel() < need.value:
            with self._on_stream():
                ws = self._decode_ws = torch.empty(int(need.value), dtype=torch.uint8, device=self.device)
        return ws

    def decode_loss(self, rendered, decoder, fmap, loss: str = "l1", scale: Optional[float] = None,
                    pixel_weights: Optional[torch.Tensor] = None, grad_rendered: Optional[torch.Tensor] = None):
        """Decode, compare and both gradients of one view of a latent field in one call (gwbp_decode_loss; no [H, W, D] tensor):
        with y = rendered @ decoder, e = y - fmap and w_p = scale * pixel_weights[p],
            loss = sum w_p |e| ("l1") or sum w_p e^2 ("l2"), grad_rendered = d loss / d rendered [H, W, d],
            grad_decoder = d loss / d decoder [d, D].
        Returns (loss, grad_rendered, grad_decoder, table): loss a float64 0-d device tensor (= table[0]), table float64 [8] =
        loss, n_pixels, n_bad, P, d, D, 0, 0.  A pixel whose map row holds a non-finite value adds nothing anywhere, has a zero
        gradient row and counts in n_bad.
        rendered: float32 [H, W, d], d % 16 == 0, 16 <= d <= 128 (rows of another layout are copied once).  decoder: float32
        [d, D], D % 16 == 0, 16 <= D <= 2048.  fmap: [H, W, D] float32 / float16 / bfloat16 read as stored, unit channel stride,
        any non-negative pixel strides.  pixel_weights: [H, W] as blend_weighted takes it.  grad_rendered: the float32 [H, W, d]
        tensor to fill; it may be `rendered` itself."""
        if loss not in _lib.LOSS_KINDS:
            raise GwbpError(f"loss must be 'l1' or 'l2', got {loss!r}")
        for t, name in ((rendered, "rendered"), (decoder, "decoder")):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.device.index != self._dev_index:
                raise GwbpError(f"{name} must be a float32 HIP tensor on cuda:{self._dev_index} (there is no CPU path)")
        if rendered.dim() != 3 or decoder.dim() != 2 or rendered.shape[2] != decoder.shape[0]:
            raise GwbpError(f"rendered must be [H, W, d] and decoder [d, D], got {tuple(rendered.shape)} and {tuple(decoder.shape)}")
        H, W, d = (int(v) for v in rendered.shape)
        D = int(decoder.shape[1])
        if not torch.is_tensor(fmap) or fmap.dim() != 3 or tuple(fmap.shape) != (H, W, D):
            raise GwbpError(f"the feature map must be [H, W, D] = [{H}, {W}, {D}], got "
                            f"{tuple(fmap.shape) if torch.is_tensor(fmap) else type(fmap).__name__}")
        if fmap.dtype not in MAP_TYPES or not fmap.is_cuda or fmap.device.index != self._dev_index:
            raise GwbpError(f"the feature map must be float32, float16 or bfloat16 on cuda:{self._dev_index}, got {fmap.dtype} "
                            f"on {fmap.device}")
        sy, sx, sc = fmap.stride()
        if sc != 1 or sy < 0 or sx < 0:
            raise GwbpError("the map's channels must be contiguous (unit last stride) and its pixel strides non-negative")

        def flat_rows(t):  # [H, W, d] whose pixel p = y W + x lies at p * row stride
            return t.stride(2) == 1 and t.stride(1) >= d and (H <= 1 or t.stride(0) == W * t.stride(1))
        with self._on_stream():
            if not flat_rows(rendered):
                rendered = rendered.contiguous()
            if decoder.stride(1) != 1 or decoder.stride(0) < D:
                decoder = decoder.contiguous()
            if grad_rendered is None:
                grad_rendered = torch.empty(H, W, d, device=self.device)
            elif (not torch.is_tensor(grad_rendered) or grad_rendered.dtype != torch.float32 or not grad_rendered.is_cuda
                  or tuple(grad_rendered.shape) != (H, W, d) or not flat_rows(grad_rendered)):
                raise GwbpError(f"grad_rendered must be a float32 HIP tensor [{H}, {W}, {d}] with flat pixel rows")
            grad_decoder = torch.empty(d, D, device=self.device)
            table = torch.empty(8, dtype=torch.float64, device=self.device)
        pw = None
        if pixel_weights is not None:
            class _Shape:
                height, width = H, W
            pw = byref(self.pixel_weights(pixel_weights, _Shape))
        ws = self._decode_workspace(d, D)
        self._call("gwbp_decode_loss", H, W, d, D, ptr(rendered), c_int64(rendered.stride(1)), ptr(decoder),
                   c_int64(decoder.stride(0)), ptr(fmap), MAP_TYPES[fmap.dtype], c_int64(sy), c_int64(sx), pw,
                   _lib.LOSS_KINDS[loss], c_float(1.0 if scale is None else float(scale)), ptr(grad_rendered),
                   c_int64(grad_rendered.stride(1)), ptr(grad_decoder), c_int64(D), ptr(table), ptr(ws), c_size_t(ws.numel()),
                   self._stream())
        return table[0], grad_rendered, grad_decoder, table

    def image_loss(self, x, y, ssim_lambda: float = 0.2, padding: str = "valid", pixel_weights: Optional[torch.Tensor] = None,
                   want_map: bool = False, want_grad: bool = False, grad_out: Optional[torch.Tensor] = None):
        """The photometric loss (1 - ssim_lambda) L1 + ssim_lambda (1 - SSIM) of a render x against a target y in one call
        (gwbp_image_loss: forward, reduce and -- want_grad -- backward, no host read in between).  Returns (table, map, grad):
        table float64 [8] = sum w ssim, sum w |x - y|, sum w (x - y)^2, Wv, Wa, windows, H W, D; map float32 [H', W', D] or None;
        grad = d loss / d x, float32 [H, W, D], or None.  x, y: float32 [H, W, D], 1 <= D <= 32, unit channel stride and flat pixel
        rows (stride(1) >= D, stride(0) == W stride(1)), each with its own pixel stride: `out[..., :3]` of an RGB+D render goes in
        without a copy; another layout is copied once.  padding "valid": the windows wholly inside the image (H, W >= 11),
        "same": all H W windows, zeros outside.  pixel_weights: [H, W] as blend_weighted takes it.  grad_out: the tensor to fill.
        Non-finite inputs are not masked: they propagate."""
        if padding not in _lib.SSIM_PADDINGS:
            raise GwbpError(f"padding must be 'valid' or 'same', got {padding!r}")
        for t, name in ((x, "x"), (y, "y")):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.device.index != self._dev_index:
                raise GwbpError(f"{name} must be a float32 HIP tensor on cuda:{self._dev_index} (there is no CPU path)")
        if x.dim() != 3 or x.shape != y.shape:
            raise GwbpError(f"x and y must be [H, W, D] of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
        H, W, D = (int(v) for v in x.shape)

        def pixel_stride(t):  # (the stride of a dimension of size 1 means nothing)
            return int(t.stride(1)) if W > 1 else int(t.stride(0)) if H > 1 else D

        def flat_rows(t):
            return ((D <= 1 or t.stride(2) == 1) and pixel_stride(t) >= D
                    and (H <= 1 or W <= 1 or t.stride(0) == W * t.stride(1)))
        off = 0 if padding == "same" else 5
        with self._on_stream():
            if not flat_rows(x):
                x = x.contiguous()
            if not flat_rows(y):
                y = y.contiguous()
            grad = None
            if want_grad or grad_out is not None:
                grad = grad_out if grad_out is not None else torch.empty(H, W, D, device=self.device)
                if (not torch.is_tensor(grad) or grad.dtype != torch.float32 or not grad.is_cuda or tuple(grad.shape) != (H, W, D)
                        or not flat_rows(grad)):
                    raise GwbpError(f"grad_out must be a float32 HIP tensor [{H}, {W}, {D}] with flat pixel rows")
            ssim = torch.empty(max(0, H - 2 * off), max(0, W - 2 * off), D, device=self.device) if want_map else None
            table = torch.empty(8, dtype=torch.float64, device=self.device)
        pw = None
        if pixel_weights is not None:
            class _Shape:
                height, width = H, W
            pw = byref(self.pixel_weights(pixel_weights, _Shape))
        need = c_size_t(0)
        self._call("gwbp_image_loss_workspace_size", H, W, D, int(grad is not None), byref(need))
        ws = getattr(self, "_image_loss_ws", None)
        if ws is None or ws.numel() < need.value:
            with self._on_stream():
                ws = self._image_loss_ws = torch.empty(int(need.value), dtype=torch.uint8, device=self.device)
        self._call("gwbp_image_loss", H, W, D, ptr(x), c_int64(pixel_stride(x)), ptr(y), c_int64(pixel_stride(y)), pw,
                   _lib.SSIM_PADDINGS[padding], c_float(float(ssim_lambda)), ptr(ssim), ptr(grad),
                   c_int64(pixel_stride(grad) if grad is not None else D), ptr(table), ptr(ws), c_size_t(ws.numel()), self._stream())
        return table, ssim, grad

    def render_pixels(self, view, colors, want_alphas=True):
        """Pixel-parallel forward render for 1..32 channels; needs project + bin_sort of `view` (not the weight store).  colors: float32,
        float16 or bfloat16 [N, D] at any row stride >= D, read as stored (a half table: the bits of colors.float(), no copy)."""
        colors, ct = field_rows(colors, "colors")
        D = colors.shape[1]
        out = torch.empty(view.height, view.width, D, device=self.device)
        alphas = self._alphas(view, want_alphas)
        self._call("gwbp_render_pixels_typed", *self._args(), byref(view), ptr(colors), ct, c_int64(row_stride(colors)), D, ptr(out),
                   ptr(alphas), self._stream())
        return out, alphas

    def render_pixels_backward(self, view, colors, v_out, v_alpha=None, want_colors=True):
        """Backward of render_pixels (gwbp_render_pixels_backward; needs project + bin_sort of `view`, not the weight store): from the
        gradient v_out [H, W, D] (and v_alpha [H, W]) that reaches the render of the float32 table colors [N, D], D <= 32, the pair
        (v_colors [N, D] or None, v_g2d [N, 6]); v_g2d = d / d(mx, my, ca, cb, cc, o) of the projected records, o the opacity the blend
        read (under the antialiased mode: opacity x compensation).  Float atomics in an order that is not fixed: not bit-reproducible
        from run to run."""
        colors, ct = field_rows(colors, "colors")
        if ct != _lib.MAP_F32:
            raise GwbpError(f"render_pixels_backward reads a float32 colour table, got {colors.dtype}")
        if colors.shape[0] != self.n:
            raise GwbpError(f"engine was sized for {self.n} Gaussians, got a table of {colors.shape[0]} rows")
        D = colors.shape[1]
        v_out = _req(v_out, "v_out")
        if tuple(v_out.shape) != (view.height, view.width, D):
            raise GwbpError(f"v_out has shape {tuple(v_out.shape)}, expected {(view.height, view.width, D)}")
        if v_alpha is not None:
            v_alpha = _req(v_alpha, "v_alpha")
            if v_alpha.numel() != view.height * view.width:
                raise GwbpError(f"v_alpha has shape {tuple(v_alpha.shape)}, expected {(view.height, view.width)}")
        v_g2d = torch.zeros(self.n, 6, device=self.device)
        v_colors = torch.zeros(self.n, D, device=self.device) if want_colors else None
        self._call("gwbp_render_pixels_backward", *self._args(), byref(view), ptr(colors), c_int64(row_stride(colors)), D, ptr(v_out),
                   ptr(v_alpha), ptr(v_colors), ptr(v_g2d), self._stream())
        return v_colors, v_g2d

    def render_dots_backward(self, view, colors, v_out, v_alpha=None):
        """The geometry half of the blend backward for a float32 table colors [N, D], D <= 128 (gwbp_render_dots_backward; needs
        project + bin_sort of `view`, not the weight store): v_g2d [N, 6] as render_pixels_backward returns it, from v_out [H, W, D]
        (and v_alpha [H, W]).  The channels enter only through <colors_j, v_out_p>; the table's own gradient is scatter(view, v_out)
        over the weight store of the forward render and is not computed here.  Float atomics: not bit-reproducible from run to run."""
        colors, ct = field_rows(colors, "colors")
        if ct != _lib.MAP_F32:
            raise GwbpError(f"render_dots_backward reads a float32 colour table, got {colors.dtype}")
        if colors.shape[0] != self.n:
            raise GwbpError(f"engine was sized for {self.n} Gaussians, got a table of {colors.shape[0]} rows")
        D = colors.shape[1]
        v_out = _req(v_out, "v_out")
        if tuple(v_out.shape) != (view.height, view.width, D):
            raise GwbpError(f"v_out has shape {tuple(v_out.shape)}, expected {(view.height, view.width, D)}")
        if v_alpha is not None:
            v_alpha = _req(v_alpha, "v_alpha")
            if v_alpha.numel() != view.height * view.width:
                raise GwbpError(f"v_alpha has shape {tuple(v_alpha.shape)}, expected {(view.height, view.width)}")
        v_g2d = torch.zeros(self.n, 6, device=self.device)
        self._call("gwbp_render_dots_backward", *self._args(), byref(view), ptr(colors), c_int64(row_stride(colors)), D, ptr(v_out),
                   ptr(v_alpha), ptr(v_g2d), self._stream())
        return v_g2d

    def project_backward(self, view, means, quats, scales, opacities, v_g2d, needs=(True,) * 4, want_viewmat=False):
        """Backward of project (gwbp_project_backward; needs the projection of `view` and of these Gaussians in the workspace, which
        says which rows are visible): from v_g2d [N, 6] = d / d(mx, my, ca, cb, cc, o) of the projected records, as
        render_pixels_backward returns it, the tuple (v_means [N, 3], v_quats [N, 4], v_scales [N, 3], v_opacities [N], v_viewmat).
        needs: which of the four float32 per-Gaussian gradients to compute (the others are None); want_viewmat: also the gradient of
        the view matrix, float64 [4, 4] with a zero bottom row (None otherwise).  The chain is evaluated in float64 per Gaussian and
        rounded once; culled rows get exact zeros; the view sums take no atomics: the same inputs give the same bits."""
        means, quats = _req(means, "means", (3,)), _req(quats, "quats", (4,))
        scales, opacities = _req(scales, "scales", (3,)), _req(opacities, "opacities")
        v_g2d = _req(v_g2d, "v_g2d", (6,))
        if not (means.shape[0] == quats.shape[0] == scales.shape[0] == opacities.shape[0] == v_g2d.shape[0] == self.n):
            raise GwbpError(f"engine was sized for {self.n} Gaussians, got {means.shape[0]} means and {v_g2d.shape[0]} v_g2d rows")
        needs = tuple(bool(x) for x in needs)
        if len(needs) != 4 or not (any(needs) or want_viewmat):
            raise GwbpError("project_backward: needs must have four entries, and at least one gradient must be asked for")
        model, mode = _lib.camera_of(view)
        with self._on_stream():
            outs = [torch.empty((self.n,) + tail, device=self.device) if need else None
                    for need, tail in zip(needs, ((3,), (4,), (3,), ()))]
            flat = scratch = None
            if want_viewmat:
                blocks = int(self.lib.gwbp_project_backward_blocks(c_int64(self.n)))
                if blocks < 0:
                    check(blocks, "gwbp_project_backward_blocks")
                flat = torch.empty(12, dtype=torch.float64, device=self.device)
                scratch = torch.empty(max(1, blocks) * 12, dtype=torch.float64, device=self.device)
            self._call("gwbp_project_backward", *self._args(), byref(view), _lib.CAMERA_MODELS[model], _lib.RASTERIZE_MODES[mode],
                       ptr(means), ptr(quats), ptr(scales), ptr(opacities), ptr(v_g2d), *(ptr(t) for t in outs), ptr(flat),
                       ptr(scratch), self._stream())
            v_viewmat = None
            if want_viewmat:
                v_viewmat = torch.zeros(4, 4, dtype=torch.float64, device=self.device)
                v_viewmat[:3, :3] = flat[:9].view(3, 3)
                v_viewmat[:3, 3] = flat[9:]
        return (*outs, v_viewmat)

    def probe_pixels(self, view, xy, table, want_depth=True, want_alpha=True):
        """The render of `table` [N, D] (float32, float16 or bfloat16, any row stride >= D, read as stored: a half table gives the bits of
        table.float() without that copy) at the pixels xy [M, 2] (int32, (x, y)) only:
        (out [M, D], depth [M] or None, alpha [M] or None); needs project + bin_sort of `view` (not the weight store).  depth
        accumulates the PROJECTION's camera depths; rasterization()'s "+D" channel computes its depths in torch -- render that
        column as a one-channel table to get its bits."""
        table, ft = field_rows(table, "the probed table")
        if table.shape[0] != self.n:
            raise GwbpError(f"engine was sized for {self.n} Gaussians, the table has {table.shape[0]} rows")
        if xy.dtype != torch.int32 or xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_cuda:
            raise GwbpError("xy must be an int32 [M, 2] HIP tensor of (x, y) pixels")
        xy = xy.contiguous()
        M, D = xy.shape[0], table.shape[1]
        ld = row_stride(table)
        out = torch.empty(M, D, device=self.device)
        depth = torch.empty(M, device=self.device) if want_depth else None
        alpha = torch.empty(M, device=self.device) if want_alpha else None
        self._call("gwbp_probe_pixels_typed", *self._args(), byref(view), M, ptr(xy), ptr(table), ft, c_int64(ld), D, ptr(out), ptr(depth),
                   ptr(alpha), self._stream())
        return out, depth, alpha

    def pixel_gaussians(self, view, k: int, xy=None, want_median=True):
        """The Gaussians each pixel is made of (gwbp_pixel_gaussians; needs project + bin_sort of `view`, not the weight store, and leaves
        the workspace as it was): (ids int32 [P.., k], weights [P.., k], n_contrib int32 [P..], alpha [P..], median_id int32 [P..] or None,
        median_depth [P..] or None) with P.. = [H, W], or [M] at the pixels xy [M, 2] (int32, (x, y)) only.  ids / weights: the k
        contributing records of largest weight alpha T, heaviest first, equal weights by id; empty slots -1 / 0.  n_contrib > k: the
        list was cut.  median: the record after which T <= 0.5 and its projected camera depth, -1 / 0 where T stays above one half."""
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= PIXEL_TOPK_MAX:
            raise GwbpError(f"k must be an int in [1, {PIXEL_TOPK_MAX}], got {k!r}")
        if xy is None:
            M, shape = 0, (view.height, view.width)
        else:
            if not torch.is_tensor(xy) or xy.dtype != torch.int32 or xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_cuda:
                raise GwbpError("xy must be an int32 [M, 2] HIP tensor of (x, y) pixels")
            xy = xy.contiguous()
            M, shape = xy.shape[0], (xy.shape[0],)
            if not 1 <= M <= PROBE_MAX_PIXELS:
                raise GwbpError(f"the number of pixels must be in [1, {PROBE_MAX_PIXELS}], got {M}")
        ids = torch.empty(*shape, k, dtype=torch.int32, device=self.device)
        weights = torch.empty(*shape, k, device=self.device)
        n_contrib = torch.empty(shape, dtype=torch.int32, device=self.device)
        alpha = torch.empty(shape, device=self.device)
        median_id = torch.empty(shape, dtype=torch.int32, device=self.device) if want_median else None
        median_depth = torch.empty(shape, device=self.device) if want_median else None
        self._call("gwbp_pixel_gaussians", *self._args(), byref(view), k, M, ptr(xy), ptr(ids), ptr(weights), ptr(n_contrib), ptr(alpha),
                   ptr(median_id), ptr(median_depth), self._stream())
        return ids, weights, n_contrib, alpha, median_id, median_depth

    def render_labels(self, view, labels, num_classes: int, want_maps=True, want_alphas=True, want_argmax=False, gt=None,
                      counts=None, cut: int = 64, min_opacity: float = 0.0):
        """Per-Gaussian labels [N] (any integer type; int64 narrowed by narrow_labels; a label outside [0, num_classes) adds to
        alpha and to no class) rendered in one blend pass (gwbp_render_labels; needs project + bin_sort of `view`, not the weight
        store).  Returns (maps float32 [H, W, K] or None, alphas [H, W] or None, argmax int32 [H, W] or None, counts or None).
        maps equal the render of the one-hot [N, K] table bit for bit; argmax is the class of the largest sum (lowest index among
        equals), -1 where nothing contributed or that sum lies below min_opacity.  gt: an integer [H, W] label map; the call then
        ADDS the {intersection, predicted, ground truth} pixel counts of every class into counts (int64 [K, 3] on the device;
        made, zeroed, when None), predicted being uint8(clamp(maps, 0, 1) * 255) > cut."""
        K = int(num_classes)
        if isinstance(num_classes, bool) or K < 1:
            raise GwbpError(f"num_classes must be a positive int, got {num_classes!r}")
        if (not torch.is_tensor(labels) or labels.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
                or labels.dim() != 1):
            raise GwbpError("labels must be an integer [N] tensor")
        if not labels.is_cuda or labels.device.index != self._dev_index:
            raise GwbpError(f"labels must be on the engine's device cuda:{self._dev_index}, got {labels.device}")
        if labels.shape[0] != self.n:
            raise GwbpError(f"engine was sized for {self.n} Gaussians, got {labels.shape[0]} labels")
        with self._on_stream():
            # (only an int64 id can wrap into range when narrowed; the kernel ignores what lies outside [0, K) itself)
            labels = (narrow_labels(labels, K) if labels.dtype == torch.int64 else labels.to(torch.int32)).contiguous()
            if counts is not None and gt is None:
                raise GwbpError("counts without a ground-truth map gt")
            if gt is not None:
                if not torch.is_tensor(gt) or gt.is_floating_point() or gt.is_complex() or gt.dtype == torch.bool:
                    raise GwbpError("gt must be an integer [H,W] label map")
                if tuple(gt.shape) != (view.height, view.width):
                    raise GwbpError(f"gt must be [H,W] = [{view.height},{view.width}], got {tuple(gt.shape)}")
                gt = gt.to(self.device)
                gt = (narrow_labels(gt, K) if gt.dtype == torch.int64 else gt.to(torch.int32)).contiguous()
                if counts is None:
                    counts = torch.zeros(K, 3, dtype=torch.int64, device=self.device)
                elif (not torch.is_tensor(counts) or counts.dtype != torch.int64 or not counts.is_cuda
                      or counts.device.index != self._dev_index or not counts.is_contiguous() or tuple(counts.shape) != (K, 3)):
                    raise GwbpError(f"counts must be a contiguous int64 HIP tensor [{K},3]")
            if not (want_maps or want_alphas or want_argmax or gt is not None):
                raise GwbpError("render_labels: no output asked for")
            maps = torch.empty(view.height, view.width, K, device=self.device) if want_maps else None
            alphas = self._alphas(view, want_alphas)
            argmax = torch.empty(view.height, view.width, dtype=torch.int32, device=self.device) if want_argmax else None
            sums = torch.empty(view.height, view.width, device=self.device) if want_argmax and K > 64 else None
        self._call("gwbp_render_labels", *self._args(), byref(view), ptr(labels), K, ptr(maps), ptr(alphas), ptr(argmax), ptr(sums),
                   c_float(min_opacity), ptr(gt), int(cut), ptr(counts), self._stream())
        return maps, alphas, argmax, counts

    def sh_colors(self, degree: int, means, coeffs, campos):
        """[N,K,3] SH coefficients -> [N,3] view-dependent colours (+0.5, clamped at 0) on the device."""
        means = _req(means, "means", (3,))
        coeffs = _req(coeffs, "sh coefficients")
        if coeffs.dim() != 3 or coeffs.shape[2] != 3 or coeffs.shape[0] != means.shape[0]:
            raise GwbpError(f"SH coefficients must be [N,K,3], got {tuple(coeffs.shape)}")
        out = torch.empty(means.shape[0], 3, device=self.device)
        cp = (c_float * 3)(*[float(v) for v in campos])
        self._call("gwbp_sh_colors", c_int64(means.shape[0]), int(degree), coeffs.shape[1], ptr(means), ptr(coeffs),
                                      cp, ptr(out), self._stream())
        return out

    def sh_eval(self, degree: int, means, head, tail, campos):
        """sh_colors over a coefficient row stored in two tables: head [N,K_head,3] and tail [N,K_tail,3] (None: one table), e.g. a
        splat dict's features_dc and features_rest as they are stored.  [N,3], the bits of sh_colors on the concatenated table."""
        return sh_eval_tables(self._call, self._stream(), degree, means, head, tail, campos)

    def sh_eval_backward(self, degree: int, means, head, tail, campos, v_colors, want_head: bool = True, want_tail: bool = True,
                         want_means: bool = True):
        """The backward of sh_eval (gwbp_sh_eval_backward): (v_head, v_tail, v_means) from v_colors [N,3], None where not asked for
        (v_tail also without a tail).  Rows of the tables above the degree's (degree + 1)^2 get exact zeros; v_means is all zero at
        degree 0.  No atomics: the same bits every run."""
        return sh_eval_tables_backward(self._call, self._stream(), degree, means, head, tail, campos, v_colors, want_head, want_tail,
                                       want_means)

    def sh_eval_dev(self, degree: int, means, head, tail, campos):
        """sh_eval with campos a float32 HIP tensor of three elements that the kernel loads (gwbp_sh_eval_dev): no host read, and
        sh_eval's bits for the same three values."""
        return sh_eval_tables_dev(self._call, self._stream(), degree, means, head, tail, campos)

    def sh_eval_backward_dev(self, degree: int, means, head, tail, campos, v_colors, want_head: bool = True, want_tail: bool = True,
                             want_means: bool = True, want_campos: bool = True):
        """The backward of sh_eval_dev (gwbp_sh_eval_backward_dev): (v_head, v_tail, v_means, v_campos).  The first three have
        sh_eval_backward's bits; v_campos is float64 [3], minus the sum of the rows' v_means values taken without atomics in a fixed
        order (exact +0 at degree 0)."""
        return sh_eval_tables_backward_dev(self._call, self._stream(), degree, means, head, tail, campos, v_colors, want_head,
                                           want_tail, want_means, want_campos)

    def adam_step(self, p, g, m, v, step: int, lr: float, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, visible=None) -> None:
        """One Adam step of the float32 table p [n, ...] IN PLACE from its gradient g, with the moments m and v (gwbp_adam_step;
        torch.optim.Adam's arithmetic with weight_decay = 0, amsgrad = False, maximize = False), on this engine's stream.  step: the
        count t >= 1 of this step; the bias corrections are formed on the host in float64, nothing is read back.  visible: None, or a
        uint8 / bool [n]: rows whose entry is zero keep the bits of p, m and v.  SplatAdam is the optimiser built on it."""
        adam_step_tables(self._call, self._stream(), p, g, m, v, visible, step, lr, b1, b2, eps)

    # ---- depth supervision (csrc/depth_loss.hip) --------------------------------------------------------------
    def _depth_workspace(self, n: int):
        need = max(_lib.depth_workspace_bytes(n), 16)
        ws = getattr(self, "_depth_ws", None)
        if ws is None or ws.numel() < need:
            with self._on_stream():
                ws = self._depth_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def _depth_upstream(self, fn: str, upstream) -> torch.Tensor:
        if not torch.is_tensor(upstream) or upstream.device != self.device or upstream.numel() != 1:
            raise GwbpError(f"{fn}: upstream must be a one-element tensor on {self.device} (it is read on the device)")
        with self._on_stream():
            return upstream.detach().to(torch.float32).reshape(1).contiguous()

    def depth_points_loss(self, render, alpha, points, depths, channel: int = -1, scale: float = 1.0, want_per_point: bool = False):
        """The reference trainer's depth term (gwbp_depth_points_loss): scale * mean |1 / d - 1 / depths| with d the bilinear sample of
        the expected depth render[..., channel] / max(alpha, 1e-10) at the points (column index x, row index y: grid_sample's
        align_corners=True coordinates, zero padding).  Returns (loss, per_point): a float32 0-dim device tensor, nothing read back,
        the same bits every call; per_point [M, 2] = (d, t) per point with want_per_point, else None.  A sample with d <= 0
        contributes 1 / depths; M = 0 gives 0."""
        fn = "depth_points_loss"
        render, alpha, H, W, Dp, ch = depth_image_args(fn, render, alpha, channel)
        points, depths, M = depth_point_args(fn, render, points, depths)
        with self._on_stream():
            loss = torch.empty((), device=self.device)
            per_point = torch.empty(M, 2, device=self.device) if want_per_point else None
        ws = self._depth_workspace(M)
        self._call("gwbp_" + fn, H, W, Dp, ch, ptr(render), ptr(alpha), c_int64(M), ptr(points), ptr(depths), c_float(float(scale)),
                   ptr(loss), ptr(per_point), ptr(ws), c_size_t(ws.numel()), self._stream())
        return loss, per_point

    def depth_points_backward(self, render, alpha, points, depths, upstream, channel: int = -1, scale: float = 1.0):
        """(v_render [H, W, D'], v_alpha [H, W]) = upstream * the gradient of depth_points_loss (gwbp_depth_points_backward); upstream
        is a one-element DEVICE tensor, read by the kernel.  v_render is zero outside `channel`.  Float atomics where points share a
        corner: not bit-reproducible.  A sample with d <= 0 adds exact zeros."""
        fn = "depth_points_backward"
        render, alpha, H, W, Dp, ch = depth_image_args(fn, render, alpha, channel)
        points, depths, M = depth_point_args(fn, render, points, depths)
        upstream = self._depth_upstream(fn, upstream)
        with self._on_stream():
            v_render, v_alpha = torch.zeros(H, W, Dp, device=self.device), torch.zeros(H, W, device=self.device)
        self._call("gwbp_" + fn, H, W, Dp, ch, ptr(render), ptr(alpha), c_int64(M), ptr(points), ptr(depths), c_float(float(scale)),
                   ptr(upstream), ptr(v_render), ptr(v_alpha), self._stream())
        return v_render, v_alpha

    def depth_map_loss(self, render, alpha, depth, weights=None, kind: str = "disparity", channel: int = -1, scale: float = 1.0):
        """The depth term against a depth map (gwbp_depth_map_loss): scale * sum w t / sum w over the pixels with depth > 0 (and
        weights > 0), t = |1 / e - 1 / depth| ("disparity") or |e - depth| ("depth") of the expected depth e.  Returns (loss, sums):
        a float32 0-dim device tensor and the float64 [2] device tensor (sum w t, sum w) the backward reads."""
        fn = "depth_map_loss"
        render, alpha, H, W, Dp, ch = depth_image_args(fn, render, alpha, channel)
        depth, weights, code = depth_map_args(fn, render, depth, weights, kind)
        with self._on_stream():
            loss, sums = torch.empty((), device=self.device), torch.empty(2, dtype=torch.float64, device=self.device)
        ws = self._depth_workspace(H * W)
        self._call("gwbp_" + fn, H, W, Dp, ch, ptr(render), ptr(alpha), ptr(depth), ptr(weights), code, c_float(float(scale)),
                   ptr(loss), ptr(sums), ptr(ws), c_size_t(ws.numel()), self._stream())
        return loss, sums

    def depth_map_backward(self, render, alpha, depth, sums, upstream, weights=None, kind: str = "disparity", channel: int = -1,
                           scale: float = 1.0):
        """(v_render [H, W, D'], v_alpha [H, W]) = upstream * the gradient of depth_map_loss (gwbp_depth_map_backward), every element
        stored once: no atomics, the same bits every call.  sums: what depth_map_loss returned."""
        fn = "depth_map_backward"
        render, alpha, H, W, Dp, ch = depth_image_args(fn, render, alpha, channel)
        depth, weights, code = depth_map_args(fn, render, depth, weights, kind)
        if not torch.is_tensor(sums) or sums.dtype != torch.float64 or sums.device != self.device or tuple(sums.shape) != (2,):
            raise GwbpError(f"{fn}: sums must be the float64 [2] tensor depth_map_loss returned")
        upstream = self._depth_upstream(fn, upstream)
        with self._on_stream():
            v_render, v_alpha = torch.empty(H, W, Dp, device=self.device), torch.empty(H, W, device=self.device)
        self._call("gwbp_" + fn, H, W, Dp, ch, ptr(render), ptr(alpha), ptr(depth), ptr(weights), code, c_float(float(scale)),
                   ptr(sums.contiguous()), ptr(upstream), ptr(v_render), ptr(v_alpha), self._stream())
        return v_render, v_alpha

    # ---- the view's RGB render for the 2-D network (create_feature_field(render_colors=...)) ----------------------------------
    @staticmethod
    def campos(view) -> Tuple[float, float, float]:
        """Camera centre of a view in world space, computed as rasterization() computes it for sh_degree (float32 on the host:
        -R^T t of the view matrix), so that the SH colours below are those of its render bit for bit."""
        vm = torch.tensor(list(view.viewmat), dtype=torch.float32).reshape(4, 4)
        return tuple((-(vm[:3, :3].T @ vm[:3, 3])).tolist())

    def view_colors(self, view, means, colors, sh_degree: Optional[int] = None) -> torch.Tensor:
        """The [N,3] colours of `view` that rasterization(..., colors, sh_degree=sh_degree) renders: `colors` itself without
        sh_degree, the SH evaluation (sh_colors: +0.5, clamped at 0) toward the view's camera centre with it."""
        if sh_degree is None:
            return _req(colors, "render colors", (3,))
        return self.sh_colors(int(sh_degree), means, colors, self.campos(view))

    def _image(self, view, image: Optional[torch.Tensor]) -> torch.Tensor:
        if image is None:
            return torch.empty(view.height, view.width, 3, device=self.device)
        if (image.dtype != torch.float32 or not image.is_cuda or not image.is_contiguous()
                or tuple(image.shape) != (view.height, view.width, 3)):
            raise GwbpError(f"image must be a contiguous float32 HIP tensor [{view.height},{view.width},3]")
        return image

    def blend_weights_rgb(self, view, colors, image: Optional[torch.Tensor] = None, pixel_weights: Optional[torch.Tensor] = None,
                          d=None, scale_d=1.0, want_alphas=False):
        """blend_weights / blend_weighted (`pixel_weights`) that also composites the view's RGB render with [N,3] `colors` while it
        blends (gwbp_blend_weights_rgb / _d_rgb): returns (image [H,W,3], alphas or None) -- the image written into `image` when
        given, equal to render_pixels(view, colors) bit for bit and unweighted whatever `pixel_weights` is.  The weight store, d
        and the alpha map are those of the blend without it."""
        colors = _req(colors, "colors", (3,))
        image = self._image(view, image)
        pw = self.pixel_weights(pixel_weights, view) if pixel_weights is not None else None
        alphas = self._alphas(view, want_alphas)
        self._tokens = None
        self._halves = self._wide_requested()
        pwp = byref(pw) if pw is not None else None
        if d is not None:
            self._check_denominator(d)
            self._need_weight_sums("blend_weights_rgb", blend=True)
            self._call("gwbp_blend_weights_d_rgb", *self._args(), byref(view), ptr(alphas), c_float(scale_d), ptr(d), pwp,
                       ptr(colors), ptr(image), self._stream())
        else:
            self._call("gwbp_blend_weights_rgb", *self._args(), byref(view), ptr(alphas), pwp, ptr(colors), ptr(image),
                       self._stream())
        return image, alphas

    def blend_tokens_rgb(self, view, lr_h: int, lr_w: int, colors, image: Optional[torch.Tensor] = None,
                         pixel_weights: Optional[torch.Tensor] = None, want_alphas=False):
        """blend_tokens / blend_tokens_weighted that also composites the view's RGB render (gwbp_blend_tokens_rgb); returns
        (image, alphas or None) as blend_weights_rgb."""
        colors = _req(colors, "colors", (3,))
        image = self._image(view, image)
        pw = self.pixel_weights(pixel_weights, view) if pixel_weights is not None else None
        if not self.token_geometry_ok(lr_h, lr_w, view.height, view.width):
            raise GwbpError(f"blend_tokens_rgb: a {lr_h}x{lr_w} map has texels narrower than a tile at "
                            f"{view.height}x{view.width}; use blend_weights_rgb + scatter(upsample='nearest')")
        ymap, xmap = self.nearest_maps(lr_h, lr_w, view.height, view.width)
        alphas = self._alphas(view, want_alphas)
        self._halves = False
        self._tokens = (int(lr_h), int(lr_w))
        self._call("gwbp_blend_tokens_rgb", *self._args(), byref(view), ptr(ymap), ptr(xmap), ptr(alphas),
                   byref(pw) if pw is not None else None, ptr(colors), ptr(image), self._stream())
        return image, alphas

    def render_rgb(self, view, colors, image: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The [H,W,3] render of a projected and sorted view into `image` (gwbp_render_pixels, no alpha map): the render of the
        schedules whose blend needs the feature map, which the network makes from this image."""
        colors = _req(colors, "colors", (3,))
        image = self._image(view, image)
        self._call("gwbp_render_pixels", *self._args(), byref(view), ptr(colors), 3, ptr(image), None, self._stream())
        return image

    def _check_acc(self, F, d, D):
        if F.dtype != torch.float32 or not F.is_cuda or not F.is_contiguous() or tuple(F.shape) != (self.n, D):
            raise GwbpError(f"F must be a contiguous float32 HIP tensor [{self.n},{D}]")
        if d is not None:
            self._check_denominator(d)

    def _check_denominator(self, t, name: str = "d") -> None:
        """d of the scatters and blends, n of the votes: one float32 per Gaussian, contiguous, on the device."""
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
                or tuple(t.shape) != (self.n,)):
            raise GwbpError(f"{name} must be a contiguous float32 HIP tensor [{self.n}]")

    def _check_class_acc(self, t, name: str, K: int) -> None:
        """F of scatter_labels, C of the votes: float32 [N, K] on the device whose rows may be wider than K."""
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or tuple(t.shape) != (self.n, K)
                or (K > 1 and t.stride(1) != 1) or t.stride(0) < K):
            raise GwbpError(f"{name} must be a float32 HIP tensor [{self.n},{K}] with unit column stride")

    def _need_weight_sums(self, what: str, blend: bool = False) -> None:
        """`what` reads per-record weight sums, which only a blend with the 256-channel scatter kernel enabled leaves: the view in
        the workspace must have been blended so, or (blend=True) the blend that `what` is about to issue must be."""
        if self._halves:
            return
        if blend:
            raise GwbpError(f"{what}(d=...) needs the 256-channel scatter kernel enabled "
                            "(set_narrow_scatter(False)): a narrow blend takes no weight sums")
        raise GwbpError(f"{what} needs a view blended with the 256-channel scatter kernel enabled "
                        "(set_narrow_scatter(False) BEFORE blend_weights): this view's headers hold no weight sums")

    def backproject_view(self, view, means, quats, scales, opacities, feats, F, d, scale_f=1.0, scale_d=1.0):
        """Per-view body of create_feature_field_* (backproject.py:115-151), one fused call (pinhole / classic views only:
        gwbp_backproject_view has no camera settings).  An fp16 / bf16 map: project + bin_sort + blend_weights + scatter
        (the fused call reads float32 only), which scatter() reads natively where it can."""
        if not _lib.is_default_camera(view):
            raise GwbpError("backproject_view is pinhole / classic only; use project + bin_sort + blend_weights + scatter "
                            f"for {_lib.camera_of(view)}")
        if feats.dtype in HALF_TYPES:
            self._feat_strides(feats, view)
            self.project(view, means, quats, scales, opacities)
            self.bin_sort(view)
            self.blend_weights(view)
            return self.scatter(view, feats, F, d, scale_f, scale_d)
        sy, sx, sc, D = self._feat_strides(feats, view)
        self._check_acc(F, d, D)
        means, quats = _req(means, "means", (3,)), _req(quats, "quats", (4,))
        scales, opacities = _req(scales, "scales", (3,)), _req(opacities, "opacities")
        self._halves, self._tokens = self._wide_requested(), None
        self._call("gwbp_backproject_view", *self._args(), byref(view), ptr(means), ptr(quats), ptr(scales),
                                             ptr(opacities), ptr(feats), c_int64(sy), c_int64(sx),
                                             c_int64(sc), D, c_float(scale_f), c_float(scale_d), ptr(F),
                                             ptr(d), self._stream())

    @staticmethod
    def can_encode_map(feats: torch.Tensor, encoder: torch.Tensor) -> bool:
        """Shapes gwbp_encode_map takes: [H,W,K] float32 with channel-contiguous 16-B aligned pixels, K % 16 == 0, K <= 2048,
        at most 16 outputs (the reference's encoder is 512 -> 16, backproject_compressed.py:26,127)."""
        return Engine._encoder_layout(feats, encoder, 2048)

    def encode_map(self, feats: torch.Tensor, encoder: torch.Tensor, workgroups: int = 0,
                   stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
        """feats[H,W,K] @ encoder[K,n] (backproject_compressed.py:127) -> [H,W,n] with the hand-written skinny GEMM
        (gwbp_encode_map: the map is read once at HBM rate, exact fp32 MFMA).  Shapes it does not take (can_encode_map)
        RAISE: the hot stage never falls back to a library GEMM silently -- callers that want one write `feats @ encoder`.
        workgroups: 0 = fastest alone; one per CU when the call overlaps latency-bound kernels on other streams
        (ViewPipeline.encode_ahead).  stream: launch there instead of on this engine's stream (an engine bound to a view's
        stream by bind_stream must not run another view's encoder on it); the output is allocated under that stream.  A half
        map (fp16 / bf16) is widened with .float() on that stream first: the encoder reads float32."""
        if feats.dim() != 3 or encoder.dim() != 2 or feats.shape[2] != encoder.shape[0]:
            raise GwbpError(f"encode_map: [H,W,K] @ [K,n] expected, got {tuple(feats.shape)} @ {tuple(encoder.shape)}")
        if not self.can_encode_map(feats, encoder):
            raise GwbpError("encode_map: [H,W,K] float32 channel-contiguous 16-B aligned map, K % 16 == 0, K <= 2048, "
                            f"<= 16 outputs required, got {tuple(feats.shape)} strides {tuple(feats.stride())} @ "
                            f"{tuple(encoder.shape)} (use feats @ encoder for other shapes)")
        if feats.dtype in HALF_TYPES:
            if stream is None:
                feats = self._widen(feats)
            else:
                with torch.cuda.stream(stream):
                    feats = feats.float()
        H, W, K = feats.shape
        n = encoder.shape[1]
        sy, sx, _ = feats.stride()
        enc = encoder.contiguous()
        handle = self._stream() if stream is None else c_void_p(stream.cuda_stream)
        if stream is None:
            out = torch.empty(H, W, n, device=feats.device, dtype=torch.float32)
        else:
            with torch.cuda.stream(stream):
                out = torch.empty(H, W, n, device=feats.device, dtype=torch.float32)
        self._call("gwbp_encode_map", ptr(feats), sy, sx, H, W, K, ptr(enc), n, ptr(out), int(workgroups), handle)
        return out

    def finalize(self, F, d, out=None):
        out = torch.empty_like(F) if out is None else out
        self._call("gwbp_finalize", c_int64(F.shape[0]), F.shape[1], ptr(F), ptr(d), ptr(out), self._stream())
        return out

    def finalize_typed(self, F, d, dtype, out=None):
        """finalize() with the field written in dtype (torch.float32, torch.float16 or torch.bfloat16; gwbp_finalize_typed): the fp32
        value of finalize() -- normalize(F / (1e-12 + d)), NaN -> 0 -- rounded once, to nearest even: bit for bit
        finalize(F, d).to(dtype), without the fp32 field.  out (optional): a contiguous tensor of F's shape and that dtype; a half out
        cannot be F.  (A method of its own: finalize()'s signature is part of the driver's recorded call schedule.)"""
        if dtype not in MAP_TYPES:
            raise GwbpError(f"finalize_typed: dtype must be float32, float16 or bfloat16, got {dtype}")
        if out is None:
            out = torch.empty(F.shape, dtype=dtype, device=F.device)
        elif out.dtype != dtype or out.shape != F.shape or not out.is_contiguous():
            raise GwbpError(f"finalize_typed: out must be a contiguous {dtype} tensor of shape {tuple(F.shape)}")
        self._call("gwbp_finalize_typed", c_int64(F.shape[0]), F.shape[1], ptr(F), ptr(d), ptr(out), MAP_TYPES[dtype], self._stream())
        return out

    # ---- counters ----------------------------------------------------------------------------------------
    def accumulate_stats(self, accum: torch.Tensor):
        """accum: uint8[32] device tensor holding a gwbp_stats struct (zero-initialised by the caller)."""
        self._call("gwbp_accumulate_stats", *self._args(), ptr(accum), self._stream())

    def stats(self) -> Dict[str, int]:
        st = Stats()
        self._call("gwbp_read_stats", *self._args(), byref(st), self._stream())
        return st.as_dict()

    @staticmethod
    def decode_stats(accum: torch.Tensor) -> Dict[str, int]:
        raw = bytes(accum.cpu().numpy().tobytes())
        return Stats.from_buffer_copy(raw).as_dict()

    def dump_pairs(self, view):
        st = self.stats()
        cap = max(int(st["n_pairs"]), 1)
        gid = torch.empty(cap, dtype=torch.int32, device=self.device)
        pix = torch.empty(cap, dtype=torch.int32, device=self.device)
        w = torch.empty(cap, device=self.device)
        n = c_int64(0)
        self._call("gwbp_dump_pairs", *self._args(), byref(view), c_int64(cap), ptr(gid), ptr(pix), ptr(w),
                                       byref(n), self._stream())
        k = int(n.value)
        return gid[:k], pix[:k], w[:k]
