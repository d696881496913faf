"""Feature-field builder: counterpart of create_feature_field_lseg / _dino (backproject.py:25-172, :175-298)
and of the compressed variant (backproject_compressed.py:39-186) on top of the fused HIP path.

Per view the reference does: rasterise(zeros [N,D]) -> (render*feats).sum().backward() -> grad.clone();
rasterise(zeros [N,3]) -> render.sum().backward() -> grad[:,0]; F += ..; d += .. (backproject.py:115-151).
Here one call (`Engine.backproject_view`) projects, sorts, blends ONCE and scatter-accumulates straight into
F[N,D] and d[N].  Views shard across ranks (`synthetic.view_shard`); the partial F/d are summed in ONE exchange
step (a reduce-scatter of F + an all-reduce of the N-float d; RCCL over xGMI when the process group backend is
"nccl"), the 1e-12 of backproject.py:63 is added once after the reduction, normalisation is row-local
(backproject.py:166-169) so every rank finalises its own row block, and one all-gather of the finalised blocks
follows if the whole field is wanted on every rank.
"""
from __future__ import annotations

import time
import warnings
from collections import namedtuple
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from .engine import Engine
from .synthetic import view_shard


def _dist():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


def reduce_partials(F: torch.Tensor, d: torch.Tensor) -> None:
    """The path's single exchange step: sum the per-rank partial accumulators."""
    dist, _, world = _dist()
    if world > 1:
        dist.all_reduce(F, op=dist.ReduceOp.SUM)
        dist.all_reduce(d, op=dist.ReduceOp.SUM)


def rows_per_rank(n: int, world: int) -> int:
    """Rows of F every rank owns after the reduce-scatter: ceil(n / world); the last rank's block may be short."""
    return -(-n // world)


def alloc_accumulators(n: int, dim: int, device, world: Optional[int] = None):
    """F[n, dim], d[n] zero accumulators whose STORAGE is padded to a multiple of the world size, so that the
    reduce-scatter of reduce_partials_sharded runs in place on it (no 2 GB pad copy).  Returns (F, d, F_storage)."""
    if world is None:
        world = _dist()[2]
    n_pad = rows_per_rank(n, world) * world
    F_store = torch.zeros(n_pad, dim, device=device, dtype=torch.float32)
    return F_store[:n], torch.zeros(n, device=device, dtype=torch.float32), F_store


def reduce_partials_sharded(F: torch.Tensor, d: torch.Tensor, F_storage: Optional[torch.Tensor] = None):
    """The path's single exchange step as a reduce-scatter: rank r receives rows [row0, row0 + n_r) of the summed F (and
    the whole summed d, 4 B per Gaussian), which is all the row-local finalise needs (backproject.py:166-169) -- half
    the xGMI traffic of an all-reduce; an all-gather of the finalised rows follows only if one rank must hold the whole
    field.  Returns (F_rows, d_rows, row0).

    N need not divide by the world size: the reduce-scatter runs on ceil(N / world) * world rows -- on `F_storage` when
    the caller allocated F with alloc_accumulators (no copy), else on a zero-padded copy."""
    dist, rank, world = _dist()
    n = F.shape[0]
    if dist is None:  # no process group: nothing to exchange
        return F, d, 0
    # (a one-rank process group still goes through the collectives: `bench.py --force-dist` exercises the RCCL calls)
    per = rows_per_rank(n, world)
    row0, row1 = min(rank * per, n), min((rank + 1) * per, n)
    dist.all_reduce(d, op=dist.ReduceOp.SUM)
    src = F
    if per * world != n:
        if F_storage is not None and F_storage.shape[0] == per * world and F_storage.data_ptr() == F.data_ptr():
            src = F_storage
        else:
            src = torch.cat([F, F.new_zeros(per * world - n, F.shape[1])])
    out = torch.empty(per, F.shape[1], device=F.device, dtype=F.dtype)
    dist.reduce_scatter_tensor(out, src, op=dist.ReduceOp.SUM)
    return out[:row1 - row0], d[row0:row1], row0


def gather_rows(rows: torch.Tensor, n: int) -> torch.Tensor:
    """All ranks' finalised row blocks -> the whole [n, D] field on every rank (one all-gather; the reference writes one
    features file, backproject.py:330)."""
    dist, _, world = _dist()
    if dist is None:
        return rows
    per = rows_per_rank(n, world)
    if rows.shape[0] != per:  # the last rank's short block: pad to the common block size
        rows = torch.cat([rows, rows.new_zeros(per - rows.shape[0], rows.shape[1])])
    full = torch.empty(per * world, rows.shape[1], device=rows.device, dtype=rows.dtype)
    dist.all_gather_into_tensor(full, rows.contiguous())
    return full[:n]


def finalize_reference(F: torch.Tensor, d: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """backproject.py:63,166-169 in plain torch (host logic used by the CPU/gloo tests; the GPU path calls
    Engine.finalize / Engine.finalize_typed -> gwbp_finalize_typed).  dtype (float32, float16 or bfloat16): the fp32 result rounded once, to nearest even."""
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"dtype must be float32, float16 or bfloat16, got {dtype}")
    den = 1e-12 + d
    x = F / den[:, None]
    x = x / x.norm(dim=-1, keepdim=True)
    x[torch.isnan(x)] = 0
    return x if dtype == torch.float32 else x.to(dtype)


# verdict of wide_kernel_selfcheck per (library path, device index): the check runs once per process and device
_WIDE_OK: Dict[tuple, bool] = {}
WIDE_SELFCHECK_TOL = 1e-6


def wide_kernel_selfcheck(device) -> bool:
    """Does the 256-channel scatter kernel of THIS build agree with the 128-channel one on THIS device?

    k_scatter_wide keeps asm-issued loads and two fixed SGPR tuples live across inline-asm statements; the build is gated by an
    assembly scan (tools/check_asm_hazards.py, run by the Makefile for every variant), and this is the run-time half of the same
    safety net: one small seeded view (T1: 4000 Gaussians, 200x136, D = 256 -- records in one half, in both halves, padded
    lists, carry rows) is blended once and scattered through both kernels; they must agree to 1e-6 of the largest row (the
    kernels differ only in summation order: 1.4e-7 measured over every build variant of round 5).  On disagreement
    ViewPipeline.choose_scatter_kernel warns and stays on the 128-channel kernel -- 5 % slower at BASELINE size, never wrong.
    A few milliseconds, once per process and device, before the first D % 256 == 0 job."""
    from . import synthetic as syn
    dev = torch.device(device)
    key = (_lib._lib_path, dev.index if dev.index is not None else torch.cuda.current_device())
    if key in _WIDE_OK:
        return _WIDE_OK[key]
    cfg = syn.CONFIGS["T1"]
    means, quats, scales, opac = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    K, vm = syn.intrinsics(cfg), syn.make_cameras(cfg)[0]
    feats = syn.make_feature_map(cfg, 0, device=dev, dim=256)
    res = []
    for wide in (True, False):
        eng = Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, tight_binning=True)
        eng.set_narrow_scatter(not wide)
        view = eng.view(vm, K, cfg.width, cfg.height)
        eng.project(view, means, quats, scales, opac)
        eng.bin_sort(view)
        eng.blend_weights(view)
        F = torch.zeros(cfg.n_gaussians, 256, device=dev)
        eng.scatter(view, feats, F, None)
        res.append(F)
    scale = res[1].norm(dim=1).max().clamp_min(1e-30)
    diff = (res[0] - res[1]).norm(dim=1).max() / scale
    ok = bool(torch.isfinite(res[0]).all()) and bool(res[1].abs().sum() > 0) and float(diff) <= WIDE_SELFCHECK_TOL
    _WIDE_OK[key] = ok
    return ok


def _scatter_weighted(e: Engine, view, feats, F, d, scale_f, scale_d, upsample=None, encoder=None) -> None:
    """Scatter a view whose weight store has been blended (feats @ encoder with the encoder fused into the slab staging)."""
    if encoder is not None:
        e.scatter_encoded(view, feats, encoder, F, d, scale_f, scale_d)
    else:
        e.scatter(view, feats, F, d, scale_f, scale_d, upsample=upsample)


def _blend_and_scatter(e: Engine, view, feats, F, d, scale_f, scale_d, upsample=None, encoder=None, fuse: bool = True,
                       tokens: bool = False, pw: Optional[torch.Tensor] = None) -> None:
    """Blend and scatter a projected and sorted view by the first form that suits its map: the fused blend + scatter kernel
    (`fuse`; with `encoder` the encoder runs in its tile prologue), token space (`tokens`), or a weight store + scatter.
    pw: the view's per-pixel weight map -- every form then runs its weighted blend (Engine.*_weighted)."""
    if pw is not None:
        if fuse and upsample is None and encoder is None and Engine.can_blend_scatter(feats):
            e.blend_scatter_weighted(view, feats, pw, F, d, scale_f, scale_d)
        elif fuse and upsample is None and encoder is not None and Engine.can_blend_scatter_encoded(feats, encoder):
            e.blend_scatter_encoded_weighted(view, feats, encoder, pw, F, d, scale_f, scale_d)
        elif tokens and upsample == "nearest" and encoder is None and Engine.can_scatter_tokens(feats, view.height, view.width):
            e.blend_tokens_weighted(view, feats.shape[0], feats.shape[1], pw)
            e.scatter_tokens(view, feats, F, d, scale_f, scale_d)
        else:
            e.blend_weighted(view, pw)
            _scatter_weighted(e, view, feats, F, d, scale_f, scale_d, upsample, encoder)
        return
    if fuse and upsample is None and encoder is None and Engine.can_blend_scatter(feats):
        e.blend_scatter(view, feats, F, d, scale_f, scale_d)
    elif fuse and upsample is None and encoder is not None and Engine.can_blend_scatter_encoded(feats, encoder):
        e.blend_scatter_encoded(view, feats, encoder, F, d, scale_f, scale_d)
    elif tokens and upsample == "nearest" and encoder is None and Engine.can_scatter_tokens(feats, view.height, view.width):
        e.blend_tokens(view, feats.shape[0], feats.shape[1])
        e.scatter_tokens(view, feats, F, d, scale_f, scale_d)
    else:
        e.blend_weights(view)
        _scatter_weighted(e, view, feats, F, d, scale_f, scale_d, upsample, encoder)


# a view whose front stage has been enqueued (ViewPipeline.front): were its denominators added by the blend on the side
# stream, its weight store blended, its token-quadrant weight sums blended (Engine.blend_tokens)?
# pw: the view's per-pixel weight map (create_feature_field(pixel_weight_fn=...)), held until the view's blend has been enqueued
_Pending = namedtuple("_Pending", "view d_done blended tokens pw", defaults=(None,))


class ViewPipeline:
    """Software pipeline over views on the caller's stream + side streams, one workspace per view in flight (two by default).

    front(v)   = project -> bin/sort -> blend_weights   (small latency-bound kernels + the 20 KB-LDS blend)
    scatter(v) = the weighted scatter-accumulate         (one 139 KB-LDS workgroup per CU: 16 of 32 wave slots)
    front(v+1) runs on a side stream while scatter(v) runs on the caller's stream, so the front kernels fill
    the wave slots the scatter kernel cannot use.  Events order  front(v) -> scatter(v) -> front(v+K)
    (workspace reuse, K = number of engines).  Nothing synchronises the host.

    With K > 2 engines the fronts of views v+1 .. v+K-1 run concurrently on K-1 side streams (`lookahead` = K - 1): on small
    scenes the front stage is a chain of ~30 dependent launches that does not fill the chip, and several chains in flight
    multiply its throughput (pipeline_depth()).
    """

    def __init__(self, n_gaussians, width, height, device, engines=None, scatter_dim: Optional[int] = None,
                 allow_wide: bool = True, scatter_workgroups: Optional[int] = None, side_priority: int = -1,
                 front_priority: Optional[bool] = None, fuse_small: bool = True, side_streams: Optional[int] = None,
                 view_per_stream: Optional[bool] = None, token_grid=None, split_encoder: bool = False):
        self.dev = torch.device(device)
        # token_grid = (h, w): the views' feature maps are h x w maps upsampled with mode="nearest" whose texels are at least a
        # tile wide and high (the dino variant's 64 x 64 patch tokens): the front stage ends with Engine.blend_tokens (per-record
        # token-quadrant weight sums instead of a weight store) and scatter() runs Engine.scatter_tokens -- one plain
        # read-modify-write of every F row that receives weight, no atomics (csrc/token.hip)
        self.token_grid = tuple(int(x) for x in token_grid) if token_grid is not None else None
        if _lib.hw_queues_late():
            # the schedule below is built on streams that run CONCURRENTLY; with the HIP runtime's default of 4 hardware queues
            # (fewer once RCCL has taken its own) the side streams share a queue with the caller's and the step becomes front +
            # scatter.  The package asks for _lib.HW_QUEUES_WANTED when it is imported, which only works before the first HIP
            # call.
            raise _lib.GwbpError(
                "ViewPipeline needs GPU_MAX_HW_QUEUES >= %d, read by the HIP runtime when it starts: import gsbp_amd (or set "
                "the variable) before the first CUDA/HIP call of the process, or run the views with pipeline=False"
                % _lib.HW_QUEUES_WANTED)
        if not _lib.hw_queues_ok():  # somebody CHOSE fewer queues (the variable was set before the package was imported)
            warnings.warn("GPU_MAX_HW_QUEUES=%s < %d: the view pipeline's streams may share hardware queues and run back to back"
                          % (__import__("os").environ.get("GPU_MAX_HW_QUEUES"), _lib.HW_QUEUES_WANTED), RuntimeWarning)
        self.eng = list(engines) if engines else [Engine(n_gaussians, width, height, device=self.dev, tight_binning=True)
                                                  for _ in range(2)]
        # Scatter grid under overlap: one persistent workgroup per CU is the measured optimum once the front stage is
        # light (C2: 4.24 ms/view at 256 vs 4.40 at 240); `scatter_workgroups` overrides.
        if scatter_workgroups is not None:  # tuning on other workloads
            for e in self.eng:
                e.scatter_workgroups = int(scatter_workgroups)
                e.caps.scatter_workgroups = e.scatter_workgroups
        # High priority = a hardware queue of its own.  With default priority the side stream can land on the main
        # stream's hardware queue (it does once RCCL has created its streams), the two streams then run strictly one after
        # the other and the step is front + scatter (5.06 instead of 4.27 ms/view at C2).
        self.scatter_dim = scatter_dim
        self.allow_wide = bool(allow_wide)
        # Narrow maps (D <= 16): the front stage stops after the sort, and blend + scatter run as ONE kernel on the caller's
        # stream (gwbp_blend_scatter: no weight store, no scatter kernel); the side stream keeps project + sort of view v+1.
        # On small images the kernel runs a wave per QUARTER tile (four short blend chains per tile instead of one long
        # one) and takes up to 32 channels; on large ones it needs two workspaces' worth of schedule (len(eng) == 2).
        small_image = Engine.fused_max_dim(width, height) == Engine.FUSED_MAX_DIM_SMALL
        # view_per_stream=True: large images too run every view entirely on a stream of its own (K > 2 workspaces): the fused
        # kernels of consecutive views then overlap at their edges (measured for the compressed variant)
        self.fuse_small = (bool(fuse_small) and scatter_dim is not None and self.token_grid is None
                           and scatter_dim <= Engine.fused_max_dim(width, height)
                           and (small_image or len(self.eng) == 2 or bool(view_per_stream)))
        # split_encoder: blend_scatter_encoded in its producer / consumer form (GWBP_FLAG_SPLIT_ENCODER: one persistent launch per
        # view whose encoder waves and blend waves run concurrently; the compressed variant on large images)
        self.split_encoder = bool(split_encoder)
        for e in self.eng:
            e.set_split_encoder(self.split_encoder)
        self.front_priority = front_priority  # None: raised wave priority for the front exactly when the wide kernel runs
        self.choose_scatter_kernel(None, None)
        K = len(self.eng)
        self.lookahead = K - 1  # fronts the driver keeps enqueued ahead of the scatter
        # Small scenes whose blend + scatter is the fused kernel (K > 2 workspaces): every workspace gets a stream of its own
        # and a view runs ENTIRELY on it -- project, sort, blend+scatter in stream order, K views in flight, one event per
        # view (the map must be ready) instead of two, and the fused kernels of consecutive views overlap.  F and d take
        # atomics anyway.  (With separate blend and scatter kernels this schedule was measured to change nothing.)
        self.independent = K > 2 and self.fuse_small and view_per_stream is not False
        n_side = K if self.independent else max(1, K - 1)
        if side_streams is not None and not self.independent:
            n_side = max(1, min(int(side_streams), K - 1))
        self.sides = [torch.cuda.Stream(device=self.dev, priority=int(side_priority)) for _ in range(n_side)]
        self.side = self.sides[0]
        self.enc_stream = None  # encoder stream, created by the first encode_ahead()
        self.ev_front = [torch.cuda.Event() for _ in range(K)]
        self.ev_done = [torch.cuda.Event() for _ in range(K)]
        # counters: one accumulator per stream that adds to it (k_accum_stats is a plain read-modify-write)
        self.accums = [torch.zeros(32, dtype=torch.uint8, device=self.dev) for _ in range(K if self.independent else 1)]
        self.accum = self.accums[0]
        if self.independent:  # the host is the limit on such scenes: no stream context switch per call either
            for e, st in zip(self.eng, self.sides):
                e.bind_stream(st)
            self.ev_ready = [torch.cuda.Event() for _ in range(K)]
        self.ev_slot = [torch.cuda.Event() for _ in range(K)]  # view-per-stream schedule: "the view in this slot is done"
        self.slot_used = [False] * K
        self.i_front = 0    # views whose front stage has been enqueued
        self.i_scatter = 0  # views whose scatter stage has been enqueued
        self.pending = {}

    # records shorter than this many pairs on average: the 128-channel scatter kernel (C2 48 -> wide, C4 25 -> narrow)
    WIDE_MIN_PAIRS_PER_RECORD = 36.0

    def choose_scatter_kernel(self, n_pairs, n_headers) -> str:
        """D % 256 == 0 may go through the 256-channel scatter kernel.  It needs fewer vector instructions per (pair,
        channel) and leaves issue slots that the front stage can use at raised wave priority (4.08 vs 4.30 ms/view at
        C2), but costs more per (Gaussian, tile) record: with short records (C4: 25 pairs per record) it loses 5 %, and
        beside the 128-channel kernel the raised priority costs 6 %.  Called once without statistics (wide if the channel
        count allows) and again by the drivers with the first views' counters.  Safe in either direction while fronts
        are pending: every Engine remembers whether the view in its workspace was blended with the half-tile lists, and
        scatters a view blended without them through the 128-channel kernel (front() likewise recorded whether it has
        already added that view's denominators)."""
        wide = (self.allow_wide and self.scatter_dim is not None and self.scatter_dim % 256 == 0
                and self.token_grid is None)  # (token space: neither scatter kernel runs)
        if wide and n_pairs is not None and n_headers:
            wide = n_pairs / n_headers >= self.WIDE_MIN_PAIRS_PER_RECORD
        if wide and self.dev.type == "cuda" and not wide_kernel_selfcheck(self.dev):
            warnings.warn("the 256-channel scatter kernel of this build disagrees with the 128-channel one on the self-check "
                          "view (wide_kernel_selfcheck): using the 128-channel kernel.  Rebuild libgwbp.so "
                          "(python __graft_entry__.py) and report the toolchain version.", RuntimeWarning)
            wide = False
        self.wide = wide
        for e in self.eng:
            e.set_narrow_scatter(not wide)
            e.set_front_priority(wide if self.front_priority is None else bool(self.front_priority))
        return "wide" if wide else "narrow"

    # render=: where the view's RGB render is made, per blend of the front stage -- True: composited by that blend itself
    # (gwbp_blend_*_rgb), False: gwbp_render_pixels right after bin_sort on the same workspace.  The fused blend + scatter
    # kernels need the map the network makes from the render, so their views always take render_pixels.
    RENDER_IN_BLEND = {"store": True, "halves": True, "tokens": True}

    def front(self, view, means, quats, scales, opacities, d=None, scale_d=1.0, pixel_weights: Optional[torch.Tensor] = None,
              render=None, image: Optional[torch.Tensor] = None):
        """d (optional): the denominator accumulator.  With the 256-channel scatter kernel chosen, the view's share of d
        is added by the blend itself on the side stream (gwbp_blend_weights_d) and scatter() then leaves d alone: the
        denominators cost nothing on the scatter's stream.
        pixel_weights (optional): the view's [H, W] weight map, produced on the caller's stream before this call: the view's
        stream waits for it, and whichever stage blends the view (this one, or scatter() for the fused kernels) runs the
        weighted blend.
        render = (colors, sh_degree), image (optional): also render the view's RGB into `image`, an [H, W, 3] float32 tensor
        allocated on the caller's stream before this call (create_feature_field(render_colors=...)).  Returns the event the
        caller's stream waits on before it reads the image (None without one)."""
        K = len(self.eng)
        b = self.i_front % K
        side = self.sides[self.i_front % len(self.sides)]
        main = torch.cuda.current_stream(self.dev)
        if self.i_front < K:
            side.wait_stream(main)  # inputs produced on the caller's stream
        elif not self.independent:
            side.wait_event(self.ev_done[b])  # workspace b is free once scatter(i-K) has finished
        # (independent: scatter(i-K) was enqueued on this very stream)
        if pixel_weights is not None or image is not None:
            if self.i_front >= K:
                ready = torch.cuda.Event()
                ready.record(main)
                side.wait_event(ready)
            if pixel_weights is not None:
                pixel_weights.record_stream(side)  # (the map is also held in _Pending until the view's blend is enqueued)
            if image is not None:
                image.record_stream(side)  # (the caller owns the image: its memory is recycled behind this stream only)
        e = self.eng[b]
        ev_image = torch.cuda.Event() if image is not None else None
        if self.independent:  # the engine is bound to `side`
            e.project(view, means, quats, scales, opacities)
            e.bin_sort(view)
            if image is not None:  # (a fused kernel blends these views: render_pixels; colours allocated on `side`)
                with torch.cuda.stream(side):
                    e.render_rgb(view, e.view_colors(view, means, *render), image)
                ev_image.record(side)
            self.pending[self.i_front] = _Pending(view, False, False, False, pixel_weights)
            self.i_front += 1
            return ev_image
        with torch.cuda.stream(side):
            e.project(view, means, quats, scales, opacities)
            e.bin_sort(view)
            d_done = d is not None and self.wide and not self.fuse_small and self.token_grid is None
            kind = "tokens" if self.token_grid is not None else None if self.fuse_small else "halves" if e._wide_requested() \
                else "store"
            cols = e.view_colors(view, means, *render) if image is not None else None
            composite = cols is not None and kind is not None and self.RENDER_IN_BLEND[kind]
            if cols is not None and not composite:
                e.render_rgb(view, cols, image)
                ev_image.record(side)
            if self.token_grid is not None:
                if composite:
                    e.blend_tokens_rgb(view, *self.token_grid, cols, image, pixel_weights)
                elif pixel_weights is not None:
                    e.blend_tokens_weighted(view, *self.token_grid, pixel_weights)
                else:
                    e.blend_tokens(view, *self.token_grid)
            elif not self.fuse_small:
                if composite:
                    e.blend_weights_rgb(view, cols, image, pixel_weights, d=d if d_done else None, scale_d=scale_d)
                elif pixel_weights is not None:
                    e.blend_weighted(view, pixel_weights, d=d if d_done else None, scale_d=scale_d)
                else:
                    e.blend_weights(view, d=d if d_done else None, scale_d=scale_d)
            if composite:
                ev_image.record(side)
            self.ev_front[b].record(side)
        self.pending[self.i_front] = _Pending(view, d_done, not self.fuse_small, self.token_grid is not None, pixel_weights)
        self.i_front += 1
        return ev_image

    # Encoder workgroups per CU beside the pipeline (see encode_ahead): None = 1 next to the separate blend and small-D
    # scatter kernels (both latency-bound: C5 2.19 -> 1.96 ms/view against 4 per CU), 2 next to the fused blend+scatter
    # kernel, where one per CU makes the encoder itself the long pole (C5: 1.65 ms/view at 1, 1.42 at 2, 1.45 at 3)
    ENCODER_WORKGROUPS_PER_CU = None

    def encode_ahead(self, feats: torch.Tensor, encoder: torch.Tensor):
        """The compressed variant's per-pixel encoder (backproject_compressed.py:127) for a LATER view on a third stream:
        an HBM-streaming kernel that overlaps with the latency-bound scatter of the current view and the front stage of
        the next.  Call it for view v+1 before scatter(v) is enqueued; hand the returned (map, event) to scatter()."""
        main = torch.cuda.current_stream(self.dev)
        if self.enc_stream is None:
            self.enc_stream = torch.cuda.Stream(device=self.dev, priority=-1)
        ready = torch.cuda.Event()
        ready.record(main)  # the map was produced on the caller's stream
        with torch.cuda.stream(self.enc_stream):
            self.enc_stream.wait_event(ready)
            # one workgroup per CU: streaming harder doubles the memory latency of the front stage and the scatter beside it
            n_cu = torch.cuda.get_device_properties(self.dev).multi_processor_count
            per_cu = self.ENCODER_WORKGROUPS_PER_CU or (2.0 if self.fuse_small else 1.0)
            # stream=: in the view-per-stream schedule eng[0] is BOUND to sides[0]; the encoder must run here, behind
            # `ready`, and `done` must cover it
            out = self.eng[0].encode_map(feats, encoder, workgroups=max(1, int(per_cu * n_cu)), stream=self.enc_stream)
            done = torch.cuda.Event()
            done.record(self.enc_stream)
        feats.record_stream(self.enc_stream)
        out.record_stream(main)
        return out, done

    def scatter(self, feats, F, d, scale_f=1.0, scale_d=1.0, t0=None, t1=None, upsample=None, after=None, encoder=None,
                ready: bool = False):
        """t0/t1: optional timing events recorded right around the scatter launch (after the cross-stream waits).
        after: an event the feature map depends on (encode_ahead).
        encoder: scatter feats @ encoder with the encoder fused into the slab staging (Engine.scatter_encoded).
        ready: the map needs no cross-stream wait -- it was produced on scatter_stream() (a feature function run under
        `with torch.cuda.stream(pipe.scatter_stream())`) or is known to be complete (a pool built before the job); only
        looked at by the view-per-stream schedule, where that wait is a third of the host's time per view."""
        i = self.i_scatter
        b = i % len(self.eng)
        main = torch.cuda.current_stream(self.dev)
        if self.independent:
            # on the view's own stream, behind its front; the map was produced on the caller's stream
            side = self.sides[b]
            if not ready:
                ev = self.ev_ready[b]  # (its previous use, view i - K, was waited for on this same stream long ago)
                ev.record(main)
                side.wait_event(ev)
                feats.record_stream(side)
            if after is not None:
                side.wait_event(after)
            self._scatter_on(side, b, feats, F, d, scale_f, scale_d, t0, t1, upsample, encoder)  # engine bound to `side`
            self.ev_slot[b].record(side)
            self.slot_used[b] = True
            self.i_scatter += 1
            return
        if after is not None:
            main.wait_event(after)
        main.wait_event(self.ev_front[b])
        self._scatter_on(main, b, feats, F, d, scale_f, scale_d, t0, t1, upsample, encoder)
        self.ev_done[b].record(main)
        self.i_scatter += 1

    def _scatter_on(self, main, b, feats, F, d, scale_f, scale_d, t0, t1, upsample, encoder):
        e = self.eng[b]
        if t0 is not None:
            t0.record(main)
        p = self.pending.pop(self.i_scatter)
        view = p.view
        if p.tokens:
            if (upsample == "nearest" and encoder is None and tuple(feats.shape[:2]) == self.token_grid
                    and Engine.can_scatter_tokens(feats, view.height, view.width)):
                e.scatter_tokens(view, feats, F, d, scale_f, scale_d)
            else:  # this view's map does not suit the token path after all: blend a weight store here, then the usual scatter
                if p.pw is not None:
                    e.blend_weighted(view, p.pw)
                else:
                    e.blend_weights(view)
                _scatter_weighted(e, view, feats, F, d, scale_f, scale_d, upsample, encoder)
        elif not p.blended:
            _blend_and_scatter(e, view, feats, F, d, scale_f, scale_d, upsample, encoder, pw=p.pw)
        else:
            _scatter_weighted(e, view, feats, F, None if p.d_done else d, scale_f, scale_d, upsample, encoder)
        if t1 is not None:
            t1.record(main)
        e.accumulate_stats(self.accums[b if self.independent else 0])

    def wait_for_slot(self) -> None:
        """View-per-stream schedule: block the HOST until the view that last used the next scatter's slot is done, i.e. keep the
        host at most K views ahead of the device.  Call it before producing a view's feature map.  Without it nothing
        throttles the host there (a view's kernels wait for nothing the host waits for), and a feature function that
        allocates a fresh map per view -- 3.47 GB at C2 size -- runs the caching allocator into the ground: a map handed to a
        side stream is only recycled once that stream has passed it, so the host allocates dozens of maps before the first is
        free again, and the allocator's out-of-memory path (synchronise, release, retry) then stalls the job for seconds
        (the CLI at C5 size: 1.1 s or 6 s for the same command).  No-op in the other schedules: there the maps are
        consumed on the caller's stream and recycled in stream order."""
        if self.independent:
            b = self.i_scatter % len(self.eng)
            if self.slot_used[b]:
                self.ev_slot[b].synchronize()

    def scatter_stream(self) -> torch.cuda.Stream:
        """The stream the NEXT scatter() runs on (the caller's current stream unless a view runs on a stream of its own)."""
        if self.independent:
            return self.sides[self.i_scatter % len(self.eng)]
        return torch.cuda.current_stream(self.dev)

    def stream_of(self, i: int) -> torch.cuda.Stream:
        """The stream view i's FRONT stage runs on (timing events of a driver)."""
        return self.sides[i % len(self.sides)]

    def join(self):
        """Make the caller's stream wait for everything enqueued so far (the accumulators are complete behind it)."""
        main = torch.cuda.current_stream(self.dev)
        for side in self.sides:
            main.wait_stream(side)

    def release(self):
        """End of the job: the caller's stream waits for everything enqueued, and engines that were bound to a stream of
        this pipeline follow torch's current stream again (an engine handed in by the caller outlives the pipeline)."""
        self.join()
        if self.independent:
            for e in self.eng:
                e.bind_stream(None)

    def reset_stats(self):
        self.join()
        for a in self.accums:
            a.zero_()

    def stats_async(self):
        """(host copies of the counter accumulators, their events): enqueue a device-to-pinned-host copy of the counters behind
        the work enqueued so far on their streams; when every event.query() is true the copies may be decoded
        (Engine.decode_stats).  Nothing synchronises."""
        copies, events = [], []
        streams = self.sides if self.independent else [torch.cuda.current_stream(self.dev)]
        for a, st in zip(self.accums, streams):
            host = torch.empty(a.shape, dtype=a.dtype, pin_memory=True)
            with torch.cuda.stream(st):
                host.copy_(a, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st)
            copies.append(host)
            events.append(ev)
        return copies, events

    def stats(self):
        """Counters summed over the views scattered so far; synchronises."""
        self.join()
        out: Dict[str, int] = {}
        for a in self.accums:
            for k, v in Engine.decode_stats(a).items():
                if k == "blend_kind":  # a per-view fact, not a counter
                    continue
                out[k] = (out.get(k, 0) | v) if k == "overflow" else out.get(k, 0) + v
        return out


# images of at least this many 16 x 16 tiles run the compressed variant's fused kernel in its producer / consumer form by default
# (create_feature_field(encoder_split=None)): 16 tiles per CU on MI355X, below which the ring's start-up and tail outweigh the overlap
SPLIT_ENCODER_MIN_TILES = 4096

# create_feature_field looks at the accumulated overflow flags after view 2 and then every this many views (a non-blocking
# copy of the counters, read back a few views later): a capacity overflow in view 150 of 200 restarts the job after at most
# this many more views instead of after the last one
OVERFLOW_CHECK_EVERY = 32


def pipeline_depth(n_gaussians: int, width: int, height: int, dim: Optional[int] = None, encoder_in_blend: bool = False) -> int:
    """Workspaces (views in flight) of the ViewPipeline.
    Small scenes: 4 -- three front stages in flight on three side streams: a view is ~35 dependent launches of 5-20 us each
    and the chain, not the chip, is the limit (C1: 0.49 -> 0.19 ms/view; 5 and more lose again: the streams start sharing
    hardware queues).
    Large scenes: 3.  Since round 4 the 256-channel scatter kernel prefetches its next slab under the tail of the running
    pass, which leaves the ONE front stage beside it too few idle slots to keep up (C2 at depth 2: front 3.82 ms against a
    3.70 ms scatter); with two fronts in flight the scatter kernel is the long stage again (3.91 -> 3.71 ms/view; C4
    10.15 -> 10.02; a fourth workspace adds nothing).  Maps narrow enough for the fused blend + scatter kernel (`dim` <= 16 on
    large images, the compressed variant) keep 2: that kernel's schedule is built for two workspaces (C5: 1.47 against 1.98).
    `encoder_in_blend` (round 5: the compressed variant's encoder inside the fused kernel's tile prologue,
    gwbp_blend_scatter_encoded): 4, every view entirely on a stream of its own -- one such kernel runs its HBM-bound prologues
    and its issue-bound blend loops in lockstep (1.29 ms alone = encoder 0.58 + blend 0.70), the kernels of four views in
    flight overlap them (C5: 1.27-1.33 ms/view; 3 workspaces 1.37-1.41, 5: 1.39-1.41, 6: 1.36-1.37; the separate encoder one
    view ahead: 1.38-1.44)."""
    if n_gaussians <= 250_000 and width * height <= 1_000_000:
        return 4
    if encoder_in_blend:
        return 4
    if dim is not None and dim <= Engine.fused_max_dim(width, height):
        return 2
    return 3


# the inputs every attempt of create_feature_field works on (gaussians = (means, quats, scales, opacities); camera = the
# camera_model / rasterize_mode keywords of Engine.view)
# pixel_weight_fn: v -> the view's [height, width] weight map, or None (unweighted)
# render: a _Render -- the views' RGB renders are made by the front and handed to feature_fn(v, image) -- or None
_Job = namedtuple("_Job", "gaussians F d sf sd feature_fn view_ids vm_host K_host width height camera encoder upsample "
                          "pixel_weight_fn render", defaults=(None, None))
# what rasterization(..., colors, sh_degree=sh_degree) renders: [N, 3] colours (sh_degree None) or [N, K, 3] SH coefficients
_Render = namedtuple("_Render", "colors sh_degree")


def _render_of(render_colors, sh_degree, n: int, device, view_fn=None) -> Optional[_Render]:
    """Check the render_colors / sh_degree keywords of the drivers before any GPU work; None without render_colors."""
    if render_colors is None:
        if sh_degree is not None:
            raise ValueError("sh_degree needs render_colors (the SH coefficients it evaluates)")
        return None
    if view_fn is not None:
        raise ValueError("view_fn takes a feature map only: it cannot hand the view's render to the network")
    if not torch.is_tensor(render_colors):
        raise ValueError(f"render_colors must be a tensor, got {type(render_colors).__name__}")
    if render_colors.dtype != torch.float32:
        raise ValueError(f"render_colors must be float32, got {render_colors.dtype}")
    if render_colors.device != torch.device(device):
        raise ValueError(f"render_colors must be on the Gaussians' device {device}, got {render_colors.device}")
    shape = tuple(render_colors.shape)
    if sh_degree is None:
        if shape != (n, 3):
            raise ValueError(f"render_colors without sh_degree must be [N, 3] = [{n}, 3] colours, got {list(shape)}")
        return _Render(render_colors, None)
    if isinstance(sh_degree, bool) or not isinstance(sh_degree, int) or not 0 <= sh_degree <= 3:
        raise ValueError(f"sh_degree must be an int in 0..3 (the SH kernel's degrees), got {sh_degree!r}")
    if len(shape) != 3 or shape[0] != n or shape[2] != 3 or shape[1] < (sh_degree + 1) ** 2:
        raise ValueError(f"render_colors with sh_degree={sh_degree} must be [N, K, 3] SH coefficients with N = {n} and "
                         f"K >= {(sh_degree + 1) ** 2}, got {list(shape)}")
    return _Render(render_colors, int(sh_degree))


def _render_view(eng: Engine, job: _Job, v: int, view=None) -> torch.Tensor:
    """View v's RGB render by project + bin_sort + render_pixels on `eng` (on the caller's stream): the render of a view whose
    map is needed before its front stage (_plan), and of the serial paths whose blend follows the map."""
    if view is None:
        view = eng.view(job.vm_host[v], job.K_host, job.width, job.height, **job.camera)
    eng.project(view, *job.gaussians)
    eng.bin_sort(view)
    return eng.render_rgb(view, eng.view_colors(view, job.gaussians[0], *job.render))


def _call_fn(job: _Job, v: int, image=None):
    """feature_fn(v), or feature_fn(v, image) for a job that renders."""
    return job.feature_fn(v) if job.render is None else job.feature_fn(v, image)


class _Renders:
    """The pipelined drivers' handoff of the views' renders: front(j) enqueues view j's front stage through pipe.front, with a
    fresh image allocated on the caller's stream when the job renders (and view j needs one), and take(j) returns that image
    behind the event after which it is written, waited for on torch's current stream (None without render_colors)."""

    def __init__(self, pipe: "ViewPipeline", job: _Job, views, skip_first: bool = False):
        self.pipe, self.job, self.views = pipe, job, views
        self.skip_first = skip_first  # view 0 was rendered by _plan: its front renders nothing
        self.images = {}  # j -> (view j's image, its event)

    def front(self, j: int) -> None:
        job, pwf = self.job, self.job.pixel_weight_fn
        img = None
        if job.render is not None and not (j == 0 and self.skip_first):
            img = torch.empty(job.height, job.width, 3, device=job.F.device)
        ev = self.pipe.front(self.views[j], *job.gaussians, job.d, job.sd,
                             pixel_weights=pwf(job.view_ids[j]) if pwf is not None else None, render=job.render, image=img)
        if img is not None:
            self.images[j] = (img, ev)

    def take(self, j: int) -> Optional[torch.Tensor]:
        if self.job.render is None:
            return None
        img, ev = self.images.pop(j)
        torch.cuda.current_stream(img.device).wait_event(ev)
        return img


# one attempt's schedule, decided before its first view from the options and the first map (_plan).  first_map: view 0's map,
# fetched early when its layout decides the schedule.  encode: where the encoder runs -- None (no encoder) | "blend" (the fused
# blend + scatter kernel's tile prologue) | "staging" (the scatter kernel's slab staging) | "ahead" (a separate kernel on a
# third stream while the view before is scattered: the feature function runs one view ahead, two full-width maps are alive)
_Plan = namedtuple("_Plan", "pipelined first_map token_grid encode depth split view_per_stream fuse_small",
                   defaults=(None, None, None, 0, False, None, True))


def _plan(job: _Job, pipeline, token_space, fuse_small, fuse_encoder, encoder_in_blend, encoder_split, split_allowed,
          eng: Optional[Engine] = None) -> _Plan:
    """create_feature_field's schedule for one attempt (the predicates and feature_fn are called in this order).  A job that
    renders gets view 0's render for an early map from a standalone project + bin_sort + render_pixels on `eng`."""
    if not (pipeline and len(job.view_ids) > 1):
        return _Plan(False)
    if _lib.hw_queues_late():
        # Somebody touched the GPU before this package was imported (a notebook, another library): the request for
        # hardware queues came too late and the pipeline's streams would share queues.  That costs speed, not results,
        # so the DRIVER degrades by itself: one stream, same F and d.  Constructing a ViewPipeline
        # explicitly still raises -- whoever asks for the overlapped schedule by name should hear that it cannot run.
        warnings.warn("gsbp_amd was imported after the HIP runtime had started: GPU_MAX_HW_QUEUES=%d could not be "
                      "requested, create_feature_field runs its views on ONE stream (pipeline=False; ~20 %% slower at "
                      "BASELINE size).  Import gsbp_amd, or set the variable, before the first CUDA/HIP call."
                      % _lib.HW_QUEUES_WANTED, RuntimeWarning, stacklevel=3)
        return _Plan(False)
    encoder, upsample, width, height = job.encoder, job.upsample, job.width, job.height
    first_map = None
    if encoder is not None or upsample == "nearest":
        v0 = job.view_ids[0]
        first_map = _call_fn(job, v0, _render_view(eng, job, v0) if job.render is not None else None)
    # the dino shape -- a nearest-upsampled map whose texels are at least a tile wide and high, D % 4 == 0 -- goes
    # through token space (Engine.blend_tokens / scatter_tokens); decided on the first map, checked per view
    token_grid = (tuple(first_map.shape[:2]) if (token_space and upsample == "nearest" and encoder is None
                                                 and Engine.can_scatter_tokens(first_map, height, width)) else None)
    enc_blend = (encoder is not None and fuse_small and not fuse_encoder and upsample is None
                 and encoder_in_blend is not False and Engine.can_blend_scatter_encoded(first_map, encoder))
    n, d_out = job.F.shape
    depth = pipeline_depth(n, width, height, d_out, encoder_in_blend=enc_blend) if pipeline is True else max(2, int(pipeline))
    split = bool(enc_blend and split_allowed and (encoder_split if encoder_split is not None
                                                  else (-(-width // 16)) * (-(-height // 16)) >= SPLIT_ENCODER_MIN_TILES))
    encode = (None if encoder is None else "blend" if enc_blend else "staging"
              if fuse_encoder and upsample is None and Engine.can_fuse_encoder(first_map, encoder) else "ahead")
    return _Plan(True, first_map, token_grid, encode, depth, split, True if (enc_blend and depth > 2) else None,
                 fuse_small and not (fuse_encoder and encoder is not None))


def _run_pipelined(job: _Job, plan: _Plan, eng: Engine, allow_wide: bool, stream_safe: bool) -> Dict[str, int]:
    """The views through a ViewPipeline of plan.depth workspaces (eng's and new ones); returns the counters.  An overflow seen
    after view 2 or by a later probe (every OVERFLOW_CHECK_EVERY views) ends the pass early: the counters then show it."""
    (means, _, _, _), F, d, sf, sd, _, ids, _, _, width, height, _, encoder, upsample, _, render = job
    n, first_map = means.shape[0], plan.first_map
    pipe = ViewPipeline(n, width, height, means.device, scatter_dim=F.shape[1], token_grid=plan.token_grid,
                        split_encoder=plan.split, allow_wide=allow_wide, fuse_small=plan.fuse_small,
                        view_per_stream=plan.view_per_stream,
                        engines=[eng] + [Engine(n, width, height, device=means.device, tight_binning=eng.tight_binning,
                                                isect_cap=eng.isect_cap, pair_cap=eng.pair_cap)
                                         for _ in range(plan.depth - 1)])
    views = [eng.view(job.vm_host[v], job.K_host, width, height, **job.camera) for v in ids]
    # (a weight map and an image are made on the caller's stream right before their view's front is enqueued; view 0's map may
    # exist already: _plan rendered that view by itself)
    renders = _Renders(pipe, job, views, skip_first=first_map is not None)
    front = renders.front

    def fmap(j):  # view j's map, made on torch's current stream (behind the view's render)
        if render is not None and j == 0 and first_map is not None:
            return first_map  # (a job that renders has view 0's image from _plan only: its map is not made twice)
        return _call_fn(job, ids[j], renders.take(j))

    for j in range(min(pipe.lookahead, len(ids))):
        front(j)
    enc_blend, staging = plan.encode == "blend", plan.encode == "staging"
    ahead = pipe.encode_ahead(first_map, encoder) if plan.encode == "ahead" else None
    probe = None  # (pinned copy of the counters, event): an overflow costs at most OVERFLOW_CHECK_EVERY views
    for i, v in enumerate(ids):
        if i == 2:  # one host sync per job: views 0 and 1 are counted, pick the scatter kernel for the rest
            st01 = pipe.stats()
            if st01["overflow"]:
                break
            pipe.choose_scatter_kernel(st01["n_pairs"], st01["n_headers"])
        if probe is not None and all(e.query() for e in probe[1]):  # non-blocking: the copy was enqueued views ago
            if any(Engine.decode_stats(a)["overflow"] for a in probe[0]):
                break
            probe = None
        if i > 2 and i % OVERFLOW_CHECK_EVERY == 0 and probe is None:
            probe = pipe.stats_async()
        if i + pipe.lookahead < len(ids):
            front(i + pipe.lookahead)
        pipe.wait_for_slot()  # (view-per-stream schedule only: the host stays at most `depth` maps ahead)
        if enc_blend or staging:  # the encoder inside the fused blend + scatter kernel or the scatter kernel's staging
            feats, fenc = (first_map if i == 0 else fmap(i)), encoder
            if staging and not Engine.can_fuse_encoder(feats, encoder):
                feats, fenc = eng.encode_map(feats, encoder), None
            pipe.scatter(feats, F, d, sf, sd, encoder=fenc)
            continue
        if encoder is not None:
            feats, after = ahead
            if i + 1 < len(ids):
                ahead = pipe.encode_ahead(fmap(i + 1), encoder)
        elif stream_safe:
            # (view-per-stream schedule: the feature function runs on the stream that consumes its map)
            with torch.cuda.stream(pipe.scatter_stream()):
                feats, after = fmap(i), None
        elif upsample == "nearest" and i == 0:
            feats, after = first_map, None
        else:
            feats, after = fmap(i), None  # on the caller's stream; scatter() waits for it with an event
        pipe.scatter(feats, F, d, sf, sd, upsample=upsample, after=after, ready=encoder is None and stream_safe)
    stats = pipe.stats()
    pipe.release()
    return stats


def _run_serial(job: _Job, eng: Engine, fuse_small: bool, token_space: bool) -> Dict[str, int]:
    """The views one after the other on the caller's stream; returns the counters (synchronises)."""
    accum = torch.zeros(32, dtype=torch.uint8, device=job.F.device)
    if job.render is not None:
        return _run_serial_rendered(job, eng, fuse_small, token_space, accum)
    for v in job.view_ids:
        feats = job.feature_fn(v)
        if job.encoder is not None:
            # backproject_compressed.py:127 through the hand-written kernel, whose domain includes the reference's 512 -> 16
            # encoder; anything else RAISES (Engine.encode_map): the drivers never switch to a library GEMM behind the
            # caller's back (whoever wants one encodes in the feature function and passes encoder=None)
            feats = eng.encode_map(feats, job.encoder)
        view = eng.view(job.vm_host[v], job.K_host, job.width, job.height, **job.camera)
        pw = job.pixel_weight_fn(v) if job.pixel_weight_fn is not None else None
        if (pw is None and job.upsample is None and not (fuse_small and Engine.can_blend_scatter(feats))
                and _lib.is_default_camera(view)):
            eng.backproject_view(view, *job.gaussians, feats, job.F, job.d, job.sf, job.sd)  # project, sort, blend, scatter: one C call
        else:  # (gwbp_backproject_view has no weight map: a weighted view always takes the stages)
            eng.project(view, *job.gaussians)
            eng.bin_sort(view)
            _blend_and_scatter(eng, view, feats, job.F, job.d, job.sf, job.sd, job.upsample, fuse=fuse_small,
                               tokens=token_space, pw=pw)
        eng.accumulate_stats(accum)
    return Engine.decode_stats(accum)


def _run_serial_rendered(job: _Job, eng: Engine, fuse_small: bool, token_space: bool, accum: torch.Tensor) -> Dict[str, int]:
    """_run_serial of a job that renders: per view project, bin_sort, render_pixels, feature_fn(v, image), then the blend and
    scatter that suit the map (never gwbp_backproject_view: the map exists only after the front)."""
    for v in job.view_ids:
        view = eng.view(job.vm_host[v], job.K_host, job.width, job.height, **job.camera)
        feats = job.feature_fn(v, _render_view(eng, job, v, view))
        if job.encoder is not None:
            feats = eng.encode_map(feats, job.encoder)
        pw = job.pixel_weight_fn(v) if job.pixel_weight_fn is not None else None
        _blend_and_scatter(eng, view, feats, job.F, job.d, job.sf, job.sd, job.upsample, fuse=fuse_small, tokens=token_space,
                           pw=pw)
        eng.accumulate_stats(accum)
    return Engine.decode_stats(accum)


def _overflow_action(overflow: int, split_allowed: bool, attempt: int) -> Optional[str]:
    """After an attempt with these overflow flags: None (done), "grow" (the workspace) or "no_split" (rebuild without the
    producer / consumer kernel); raises where a rerun cannot help."""
    if overflow & 16:
        # a wave of the producer / consumer kernel gave up waiting on its LDS ring (its waits are bounded so that a
        # scheduling accident cannot hang the device): the accumulators are incomplete.  Never seen in 2000-view soaks
        # and the fuzz; if it happens, say so and build the field again with the one-wave-per-tile form of the kernel.
        if not split_allowed:
            raise RuntimeError("gwbp_stats.overflow bit 4 (ring stall) without the producer / consumer kernel: internal error")
        warnings.warn("a wave of gwbp_blend_scatter_encoded's producer / consumer kernel gave up waiting on its LDS ring "
                      "(gwbp_stats.overflow bit 4); building the field again with encoder_split=False -- please report it",
                      RuntimeWarning, stacklevel=3)
        return "no_split"
    if overflow & 8:
        raise RuntimeError("gwbp_blend_tokens met a tile that spans more than 2 x 2 texels (gwbp_stats.overflow bit 3): "
                           "the map is finer than Engine.token_geometry_ok() admitted")
    if overflow & 4:
        raise RuntimeError("a view was scattered with a kernel that did not match its blend (gwbp_stats.overflow "
                           "bit 2): F and d are incomplete")
    if not overflow:
        return None
    if attempt == 5:
        raise RuntimeError(f"workspace overflow (flags {overflow}) after five enlargements")
    return "grow"


def create_feature_field(means, quats, scales, opacities, viewmats, K, width: int, height: int,
                         feature_fn: Callable[[int], torch.Tensor], dim: int, reduction: str = "sum",
                         encoder: Optional[torch.Tensor] = None, engine: Optional[Engine] = None,
                         views: Optional[Sequence[int]] = None, view_fn=None, pipeline: bool = True,
                         return_partials: bool = False, verbose: bool = False, upsample: Optional[str] = None,
                         gather: bool = True, allow_wide: bool = True, fuse_encoder: bool = False,
                         fuse_small: bool = True, feature_fn_stream_safe: bool = False,
                         encoder_in_blend: Optional[bool] = None, token_space: bool = True,
                         encoder_split: Optional[bool] = None, camera_model: str = "pinhole",
                         rasterize_mode: str = "classic",
                         pixel_weight_fn: Optional[Callable[[int], torch.Tensor]] = None,
                         render_colors: Optional[torch.Tensor] = None, sh_degree: Optional[int] = None,
                         out_dtype: torch.dtype = torch.float32):
    """Build the [N, dim_out] per-Gaussian feature field.

    means/quats/scales/opacities: post-activation Gaussians (backproject.py:55-57), device tensors.
    viewmats [V,4,4], K [3,3]; feature_fn(v) -> feats[H,W,dim] float32, float16 or bfloat16 on the same device (stands in for
    the LSeg/DINO forward of backproject.py:102-113 / :236-249).  A half map gets the schedule an fp32 map of its shape gets;
    the 128- and 256-channel scatter kernels and token space read it as it is (Engine.scatter, Engine.scatter_tokens), the
    other kernels (D <= 64, the encoder) from a .float() copy made at the call.  F and d equal those of feats.float().
    reduction: "sum" (lseg, backproject.py:127,145) or "mean" (dino, backproject.py:263,283).
    encoder [dim, dim_out]: backproject_compressed.py:127 (feats @ encoder before back-projection).
    upsample="nearest" | "bilinear": feature_fn returns the network's LOW-RESOLUTION map [h,w,dim] (dino patch tokens,
    backproject.py:242-243; the normalised lseg map, :108-109); the upsampling to (height, width) of
    backproject.py:244-248 / :110-112 happens while the scatter kernel stages its tile slabs instead of materialising
    an [H,W,dim] map per view.
    views: explicit list of view indices for this rank (default: interleaved shard over the process group).
    view_fn: injection point for the per-view accumulate (tests drive the sharding/reduction logic on CPU).
    fuse_encoder: with `encoder`, apply it inside the scatter kernel's slab staging (gwbp_scatter_encoded: the full-width map
    is read once, no [H,W,dim_out] intermediate) when the map's layout allows; False (default, measured faster in the
    three-stream pipeline: C5 2.19 vs 2.29 ms/view; the fused kernel wins on one stream, 2.51 vs 2.70) = a separate encode
    kernel one view ahead on a third stream (gwbp_encode_map).
    encoder_in_blend: with `encoder`, apply it inside the fused blend + scatter kernel's tile prologue (gwbp_blend_scatter_encoded:
    one kernel per view, no [H,W,dim_out] map, four views in flight on streams of their own).  None (default) = whenever the
    first map's layout allows and fuse_small is on (C5: 1.27-1.33 against 1.38-1.44 ms/view for the encoder one view ahead);
    False = never.
    encoder_split: with encoder_in_blend, run that kernel in its producer / consumer form (GWBP_FLAG_SPLIT_ENCODER: one persistent
    launch per view, encoder waves and blend waves around an LDS ring of encoded tiles).  None (default) = on images of at least
    SPLIT_ENCODER_MIN_TILES tiles, where a CU's encoder waves have tiles enough to stream; False = never.
    token_space: with upsample="nearest", maps whose texels are at least a 16 x 16 tile wide and high and whose channel count is a
    multiple of 4, 64 or more (the dino variant's 64 x 64 x 1024 patch tokens at 1600 x 1060; the other DINOv2 backbones' 384,
    768, 1536) are back-projected in TOKEN space: the blend
    leaves per-(Gaussian, tile) weight sums of the tile's 2 x 2 tokens and every F row that receives weight is updated with ONE
    plain read-modify-write per view from the L2-resident token map -- no atomics, no weight store (csrc/token.hip).  False keeps
    the pixel-slab kernels (gwbp_scatter_upsampled) for such maps too.
    fuse_small: maps of at most 16 channels (after the encoder) are blended AND scattered by one kernel
    (gwbp_blend_scatter: no weight store, no scatter kernel; C5 1.96 -> 1.42 ms/view); False keeps the two-kernel form.
    feature_fn_stream_safe: STREAM CONTRACT of feature_fn.  False (default): feature_fn runs on the caller's current stream
    and every map is handed to its consumer stream with an event -- any feature function is safe, including one that
    returns a prefetched tensor, reuses a static output buffer or replays a graph (the buffer must still not be overwritten
    before the view that reads it has been scattered: `pipeline` views may be in flight).  True: in the view-per-stream
    schedule (small scenes, <= 32-channel maps) feature_fn is called under `torch.cuda.stream(<the consuming stream>)` and
    no event is recorded (a third of the host time per view there); only for functions that allocate and produce their
    output entirely on torch's current stream at call time.
    pipeline: overlap the front stages of the next view(s) with the scatter of view v (ViewPipeline); True = depth chosen by
    pipeline_depth(N, width, height, dim_out), an int >= 2 = that many workspaces, False = one stream.
    gather: under a process group, all-gather the finalised row blocks so that every rank returns the whole [N, dim_out]
    field; False returns this rank's block only (rows row0 .. of `return_partials`' stats["row0"]).
    return_partials: also return (F_rows, d, stats): the summed, un-normalised accumulators (this rank's row block of F,
    all of d) and the counters.
    camera_model ("pinhole" | "ortho" | "fisheye") / rasterize_mode ("classic" | "antialiased"): gsplat's projection options of
    the scene (a scene trained antialiased is back-projected with w = (o x compensation) T); every path above reads them from
    the projection (gwbp_project_camera), the one-call gwbp_backproject_view is used for pinhole / classic only.
    pixel_weight_fn: v -> c_v, a [height, width] weight map of view v at FULL resolution whatever `upsample` is (bool, uint8 with
    non-zero = 1, float16, bfloat16 or float32 on the device; any non-negative strides): which pixels count and how much --
    undistortion borders, sky or transients, a segmenter's don't-care region, a network's confidence.  Every view then adds
        F[g] += scale_f * sum_p w_g(p) c_v(p) f_v(p),     d[g] += scale_d * sum_p w_g(p) c_v(p)
    (the reference's loop, backproject.py:115-151, with both targets multiplied by c_v); the transmittance is unchanged.  Every
    schedule above runs its weighted blend (the serial path then never takes gwbp_backproject_view); a row whose d is 0
    finalises to 0, and reduction="mean" keeps its scales.  It is called on the caller's stream up to `pipeline` views before
    the view's feature_fn, and the map must not be overwritten before that view has been scattered.
    render_colors / sh_degree: the reference's per-view loop renders each view (rasterization(..., colors_all, sh_degree=3),
    backproject.py:89-100) and runs the 2-D network on that RENDER.  With render_colors ([N, 3] float32 colours, or [N, K, 3] SH
    coefficients with sh_degree 0..3, meaning what rasterization()'s colors / sh_degree mean) the front stage that projects and
    sorts the view for the lift also renders it, and the callback is called as feature_fn(v, image): image is a fresh contiguous
    [height, width, 3] float32 device tensor that the caller owns and may keep, equal bit for bit to
    rasterization(means, quats, scales, opacities, render_colors, viewmats[v][None], K[None], width, height, sh_degree=sh_degree,
    camera_model=..., rasterize_mode=...)[0][0] (no background; unweighted whatever pixel_weight_fn is).  The storing and token
    blends composite it while they blend (gwbp_blend_*_rgb); the fused blend + scatter schedules render it with render_pixels on
    the same workspace before their blend.  Not with view_fn.
    feature_fn may be called more than once per view: a workspace overflow restarts the job with larger capacities, and every
    view's map is asked for again.
    out_dtype: torch.float32 (default), torch.float16 or torch.bfloat16 -- the type of the returned field.  The accumulators F and d
    stay float32; the finalise writes its row block in out_dtype (the float32 value rounded once, to nearest even: bit for bit
    field.to(out_dtype), without the float32 field) and the all-gather moves that.  A finalised row has unit norm, so both half
    types hold it; prompt_scores, knn_search, fit_pca, fit_kmeans, neighbor_similarity, smooth_features and sample_field read
    such a field as it is.
    """
    if out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"out_dtype must be torch.float32, torch.float16 or torch.bfloat16, got {out_dtype}")
    render = _render_of(render_colors, sh_degree, means.shape[0], means.device, view_fn)
    dist, rank, world = _dist()
    n = means.shape[0]
    d_out = dim if encoder is None else encoder.shape[1]
    F, d, F_store = alloc_accumulators(n, d_out, means.device, world)
    if reduction not in ("sum", "mean"):
        raise ValueError(reduction)
    sf, sd = (1.0, 1.0) if reduction == "sum" else (1.0 / (height * width * d_out), 1.0 / (height * width * 3))
    # one D2H copy of the cameras, not one per view
    job = _Job((means, quats, scales, opacities), F, d, sf, sd, feature_fn,
               list(views) if views is not None else view_shard(viewmats.shape[0], rank, world),
               viewmats.detach().cpu(), K.detach().cpu(), width, height,
               dict(camera_model=camera_model, rasterize_mode=rasterize_mode), encoder, upsample, pixel_weight_fn, render)
    if view_fn is not None and pixel_weight_fn is not None:
        raise ValueError("view_fn takes a feature map only: it cannot apply pixel_weight_fn's weights")

    t0 = time.time()
    stats: Dict[str, int] = {}
    if view_fn is None:
        eng = engine or Engine(n, width, height, device=means.device, tight_binning=True)  # same F and d, shorter tile lists
        split_allowed = True
        for attempt in range(6):  # a capacity overflow invalidates the accumulators: grow the workspace, start over
            plan = _plan(job, pipeline, token_space, fuse_small, fuse_encoder, encoder_in_blend, encoder_split, split_allowed, eng)
            pipeline = plan.pipelined and pipeline  # (a late hardware-queue request downgrades the job once)
            stats = (_run_pipelined(job, plan, eng, allow_wide, feature_fn_stream_safe) if plan.pipelined
                     else _run_serial(job, eng, fuse_small, token_space))
            action = _overflow_action(stats["overflow"], split_allowed, attempt)
            if action is None:
                break
            if action == "grow":
                eng.grow(stats, views=len(job.view_ids))
            else:
                split_allowed = False
            F.zero_()
            d.zero_()
    else:
        eng = None
        for v in job.view_ids:
            feats = feature_fn(v)
            view_fn(v, feats if encoder is None else feats @ encoder)
    # The single exchange step: reduce-scatter of F (+ all-reduce of d), row-local finalise of this rank's block
    # (backproject.py:166-169 needs nothing but the row), and an all-gather of the finalised blocks only when the caller
    # wants the whole field on every rank (the reference writes one file, backproject.py:330).
    F_rows, d_rows, row0 = reduce_partials_sharded(F, d, F_store)
    if eng is None:
        out_rows = finalize_reference(F_rows, d_rows, out_dtype)
    else:
        out_rows = eng.finalize(F_rows, d_rows) if out_dtype == torch.float32 else eng.finalize_typed(F_rows, d_rows, out_dtype)
    out = gather_rows(out_rows, n) if gather else out_rows
    if verbose and rank == 0:
        print("Time taken for feature backprojection", time.time() - t0)  # backproject.py:171
    if return_partials:
        # F_rows/d: the SUMMED accumulators (this rank's row block of F starting at row0, and all of d)
        return out, F_rows, d, dict(stats, row0=row0)
    return out


class _LabelPipeline(ViewPipeline):
    """The ViewPipeline of create_label_field: the front stage blends a weight store and adds the view's denominators on its side
    stream (gwbp_blend_weights_d), the scatter stage is Engine.scatter_labels, which then adds F only.  No feature scatter kernel
    is chosen and no fused or token-space blend runs: the label kernel reads the weight store."""

    def __init__(self, *args, num_classes: int, **kw):
        self.num_classes = int(num_classes)
        super().__init__(*args, scatter_dim=None, fuse_small=False, **kw)

    def choose_scatter_kernel(self, n_pairs, n_headers) -> str:
        self.wide = True  # (what front() reads: the blend takes the record sums and adds d)
        for e in self.eng:
            e.set_narrow_scatter(False)
            e.set_front_priority(False)
        return "labels"

    def _scatter_on(self, main, b, labels, F, d, scale_f, scale_d, t0, t1, upsample, encoder):
        e = self.eng[b]
        if t0 is not None:
            t0.record(main)
        p = self.pending.pop(self.i_scatter)
        e.scatter_labels(p.view, labels, F, None if p.d_done else d, self.num_classes, scale_f, scale_d, upsample=upsample)
        if t1 is not None:
            t1.record(main)
        e.accumulate_stats(self.accums[0])


def _run_labels_pipelined(job: _Job, eng: Engine, depth: int, num_classes: int, pipe_cls=None) -> Dict[str, int]:
    """create_label_field's views through a _LabelPipeline (or `pipe_cls`, a subclass) of `depth` workspaces; an overflow seen
    after view 2 or by a later probe ends the pass early (as in _run_pipelined)."""
    (means, _, _, _), F, d, sf, sd, _, ids, _, _, width, height, _, _, upsample, _, _ = job
    n = means.shape[0]
    pipe = (pipe_cls or _LabelPipeline)(n, width, height, means.device, num_classes=num_classes,
                          engines=[eng] + [Engine(n, width, height, device=means.device, tight_binning=eng.tight_binning,
                                                  isect_cap=eng.isect_cap, pair_cap=eng.pair_cap) for _ in range(depth - 1)])
    views = [eng.view(job.vm_host[v], job.K_host, width, height, **job.camera) for v in ids]

    renders = _Renders(pipe, job, views)  # (weight maps and images are made on the caller's stream before their view's front)
    front, image_of = renders.front, renders.take

    for j in range(min(pipe.lookahead, len(ids))):
        front(j)
    probe = None
    for i, v in enumerate(ids):
        if i == 2 and pipe.stats()["overflow"]:
            break
        if probe is not None and all(e.query() for e in probe[1]):
            if any(Engine.decode_stats(a)["overflow"] for a in probe[0]):
                break
            probe = None
        if i > 2 and i % OVERFLOW_CHECK_EVERY == 0 and probe is None:
            probe = pipe.stats_async()
        if i + pipe.lookahead < len(ids):
            front(i + pipe.lookahead)
        pipe.scatter(_call_fn(job, v, image_of(i)), F, d, sf, sd, upsample=upsample)
    stats = pipe.stats()
    pipe.release()
    return stats


def _blend_rendered(eng: Engine, job: _Job, v: int, view) -> torch.Tensor:
    """The serial label and mask paths' weight-store blend of a projected, sorted view (weighted by pixel_weight_fn) with the RGB
    composite of job.render; returns the image."""
    cols = eng.view_colors(view, job.gaussians[0], *job.render)
    pw = job.pixel_weight_fn(v) if job.pixel_weight_fn is not None else None
    return eng.blend_weights_rgb(view, cols, pixel_weights=pw)[0]


def _run_labels_serial(job: _Job, eng: Engine, num_classes: int) -> Dict[str, int]:
    """create_label_field's views one after the other on the caller's stream; the label kernel adds d too (synchronises)."""
    accum = torch.zeros(32, dtype=torch.uint8, device=job.F.device)
    for v in job.view_ids:
        view = eng.view(job.vm_host[v], job.K_host, job.width, job.height, **job.camera)
        if job.render is not None:  # the blend composites the render; the labels are made from it behind the blend
            eng.project(view, *job.gaussians)
            eng.bin_sort(view)
            image = _blend_rendered(eng, job, v, view)
            labels = job.feature_fn(v, image)
        else:
            labels = job.feature_fn(v)
            eng.project(view, *job.gaussians)
            eng.bin_sort(view)
            if job.pixel_weight_fn is not None:
                eng.blend_weighted(view, job.pixel_weight_fn(v))
            else:
                eng.blend_weights(view)
        eng.scatter_labels(view, labels, job.F, job.d, num_classes, job.sf, job.sd, upsample=job.upsample)
        eng.accumulate_stats(accum)
    return Engine.decode_stats(accum)


def label_fractions(F: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """P = F / d[:, None] with 0 where d == 0: each Gaussian's share of its blend weight per class."""
    den = d[:, None]
    return torch.where(den > 0, F / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(F))


def create_label_field(means, quats, scales, opacities, viewmats, K, width: int, height: int,
                       label_fn: Callable[[int], torch.Tensor], num_classes: int, *, upsample: Optional[str] = None,
                       views: Optional[Sequence[int]] = None, pipeline: bool = True, gather: bool = True,
                       return_partials: bool = False, camera_model: str = "pinhole", rasterize_mode: str = "classic",
                       engine: Optional[Engine] = None, pixel_weight_fn: Optional[Callable[[int], torch.Tensor]] = None,
                       render_colors: Optional[torch.Tensor] = None, sh_degree: Optional[int] = None):
    """Lift per-view integer LABEL maps (a segmenter's class or instance ids, a binary mask) onto the Gaussians: the [N, num_classes]
    field P[g, k] = F[g, k] / d[g] (0 where d[g] == 0) with
        F[g, k] = sum_v sum_p w_g(p) [L_v(p) == k],    d[g] = sum_v sum_p w_g(p),
    i.e. the fraction of each Gaussian's blend weight that fell on class k.  This is create_feature_field on one_hot(L_v) with
    reduction "sum" (the reference's (render * feats).sum().backward(), backproject.py:127-131, with a 0/1 map), without the
    one-hot map: gwbp_scatter_labels adds one atomic per (Gaussian, tile) record and distinct label.  Rows sum to at most 1; the
    shortfall is the share that fell on labels outside [0, num_classes), which are ignored.  A 3-D mask is a threshold on a column.
    P is not L2-normalised like the feature field.

    label_fn(v) -> [height, width] (with upsample="nearest": any [h, w]) integer map on the device: uint8, bool, int16 or int32
    read as stored, int64 narrowed (engine.narrow_labels).
    views, pipeline (True, an int >= 2 workspaces, or False), gather, camera_model, rasterize_mode, engine: as create_feature_field.
    return_partials: also return (F_rows, d, stats) -- the summed accumulators (this rank's row block of F, all of d).
    pixel_weight_fn: v -> c_v, the view's [height, width] weight map (as create_feature_field's): F and d then sum w_g(p) c_v(p),
    so each row's fractions sum to 1 over the WEIGHTED pixels (pixels of weight 0 count for no class and not in d).
    render_colors / sh_degree: as create_feature_field's -- label_fn is then called as label_fn(v, image) with the view's RGB
    render, made by the front stage's blend; label_fn may be called more than once per view (an overflow restarts the job)."""
    if upsample not in (None, "nearest"):
        raise ValueError(f"upsample must be None or 'nearest' for label maps, got {upsample!r}")
    render = _render_of(render_colors, sh_degree, means.shape[0], means.device)
    dist, rank, world = _dist()
    n = means.shape[0]
    F, d, F_store = alloc_accumulators(n, int(num_classes), means.device, world)
    job = _Job((means, quats, scales, opacities), F, d, 1.0, 1.0, label_fn,
               list(views) if views is not None else view_shard(viewmats.shape[0], rank, world),
               viewmats.detach().cpu(), K.detach().cpu(), width, height,
               dict(camera_model=camera_model, rasterize_mode=rasterize_mode), None, upsample, pixel_weight_fn, render)
    pipelined = bool(pipeline) and len(job.view_ids) > 1
    if pipelined and _lib.hw_queues_late():
        warnings.warn("gsbp_amd was imported after the HIP runtime had started: create_label_field runs its views on ONE stream",
                      RuntimeWarning, stacklevel=2)
        pipelined = False
    depth = (pipeline_depth(n, width, height) if pipeline is True else max(2, int(pipeline))) if pipelined else 1
    eng = engine or Engine(n, width, height, device=means.device, tight_binning=True)
    stats: Dict[str, int] = {}
    for attempt in range(6):  # a capacity overflow invalidates the accumulators: grow the workspace, start over
        stats = (_run_labels_pipelined(job, eng, depth, int(num_classes)) if pipelined
                 else _run_labels_serial(job, eng, int(num_classes)))
        if _overflow_action(stats["overflow"], False, attempt) is None:
            break
        eng.grow(stats, views=len(job.view_ids))
        F.zero_()
        d.zero_()
    F_rows, d_rows, row0 = reduce_partials_sharded(F, d, F_store)
    P = label_fractions(F_rows, d_rows)
    out = gather_rows(P, n) if gather else P
    if return_partials:
        return out, F_rows, d, dict(stats, row0=row0)
    return out


class _MaskPipeline(_LabelPipeline):
    """The ViewPipeline of create_mask_feature_field: the front of create_label_field (a weight store, d added on the side stream);
    the scatter stage is Engine.scatter_mask_features of the view's (labels, table)."""

    def __init__(self, *args, **kw):
        super().__init__(*args, num_classes=1, **kw)

    def choose_scatter_kernel(self, n_pairs, n_headers) -> str:
        super().choose_scatter_kernel(n_pairs, n_headers)
        return "mask_features"

    def _scatter_on(self, main, b, mask, F, d, scale_f, scale_d, t0, t1, upsample, encoder):
        e = self.eng[b]
        if t0 is not None:
            t0.record(main)
        p = self.pending.pop(self.i_scatter)
        labels, table = mask
        e.scatter_mask_features(p.view, labels, table, F, None if p.d_done else d, scale_f, scale_d, upsample=upsample)
        if t1 is not None:
            t1.record(main)
        e.accumulate_stats(self.accums[0])


def _mask_of(mask_fn, v: int, dim: int, render: bool = False, image=None):
    """mask_fn(v) -> (labels, table) (mask_fn(v, image) for a job that renders), the table checked against the field's width."""
    out = mask_fn(v, image) if render else mask_fn(v)
    if not (isinstance(out, (tuple, list)) and len(out) == 2):
        raise ValueError(f"mask_fn({v}) must return (labels, table)")
    labels, table = out
    if not torch.is_tensor(table) or table.dim() != 2 or table.shape[1] != dim:
        raise ValueError(f"mask_fn({v}): table must be a [M, {dim}] tensor, got "
                         f"{tuple(table.shape) if torch.is_tensor(table) else type(table).__name__}")
    return labels, table


def _mask_spills(engines) -> int:
    return sum(int(e.mask_spilled.item()) for e in engines if getattr(e, "mask_spilled", None) is not None)


def _run_masks_pipelined(job: _Job, eng: Engine, depth: int, dim: int) -> Dict[str, int]:
    """create_mask_feature_field's views through a _MaskPipeline of `depth` workspaces (the schedule of _run_labels_pipelined)."""
    (means, _, _, _), F, d, sf, sd, mask_fn, ids, _, _, width, height, _, _, upsample, _, render = job
    n = means.shape[0]
    engines = [eng] + [Engine(n, width, height, device=means.device, tight_binning=eng.tight_binning,
                              isect_cap=eng.isect_cap, pair_cap=eng.pair_cap) for _ in range(depth - 1)]
    spilled0 = _mask_spills(engines)
    pipe = _MaskPipeline(n, width, height, means.device, engines=engines)
    views = [eng.view(job.vm_host[v], job.K_host, width, height, **job.camera) for v in ids]

    renders = _Renders(pipe, job, views)  # (weight maps and images are made on the caller's stream before their view's front)
    front, image_of = renders.front, renders.take

    for j in range(min(pipe.lookahead, len(ids))):
        front(j)
    probe = None
    for i, v in enumerate(ids):
        if i == 2 and pipe.stats()["overflow"]:
            break
        if probe is not None and all(e.query() for e in probe[1]):
            if any(Engine.decode_stats(a)["overflow"] for a in probe[0]):
                break
            probe = None
        if i > 2 and i % OVERFLOW_CHECK_EVERY == 0 and probe is None:
            probe = pipe.stats_async()
        if i + pipe.lookahead < len(ids):
            front(i + pipe.lookahead)
        pipe.scatter(_mask_of(mask_fn, v, dim, render is not None, image_of(i)), F, d, sf, sd, upsample=upsample)
    stats = pipe.stats()
    pipe.release()
    stats["mask_spilled"] = _mask_spills(engines) - spilled0
    return stats


def _run_masks_serial(job: _Job, eng: Engine, dim: int) -> Dict[str, int]:
    """create_mask_feature_field's views one after the other on the caller's stream; the apply kernel adds d too (synchronises)."""
    accum = torch.zeros(32, dtype=torch.uint8, device=job.F.device)
    spilled0 = _mask_spills([eng])
    for v in job.view_ids:
        if job.render is not None:  # (as _run_labels_serial)
            view = eng.view(job.vm_host[v], job.K_host, job.width, job.height, **job.camera)
            eng.project(view, *job.gaussians)
            eng.bin_sort(view)
            labels, table = _mask_of(job.feature_fn, v, dim, True, _blend_rendered(eng, job, v, view))
        else:
            labels, table = _mask_of(job.feature_fn, v, dim)
            view = eng.view(job.vm_host[v], job.K_host, job.width, job.height, **job.camera)
            eng.project(view, *job.gaussians)
            eng.bin_sort(view)
            if job.pixel_weight_fn is not None:
                eng.blend_weighted(view, job.pixel_weight_fn(v))
            else:
                eng.blend_weights(view)
        eng.scatter_mask_features(view, labels, table, job.F, job.d, job.sf, job.sd, upsample=job.upsample)
        eng.accumulate_stats(accum)
    stats = Engine.decode_stats(accum)
    stats["mask_spilled"] = _mask_spills([eng]) - spilled0
    return stats


def create_mask_feature_field(means, quats, scales, opacities, viewmats, K, width: int, height: int,
                              mask_fn: Callable[[int], Tuple[torch.Tensor, torch.Tensor]], dim: int, *, reduction: str = "sum",
                              upsample: Optional[str] = None, views: Optional[Sequence[int]] = None, pipeline: bool = True,
                              gather: bool = True, return_partials: bool = False, camera_model: str = "pinhole",
                              rasterize_mode: str = "classic", engine: Optional[Engine] = None,
                              pixel_weight_fn: Optional[Callable[[int], torch.Tensor]] = None,
                              render_colors: Optional[torch.Tensor] = None, sh_degree: Optional[int] = None,
                              out_dtype: torch.dtype = torch.float32):
    """Build the [N, dim] feature field from MASK-POOLED features: per view a segmenter's mask or instance map L_v and one
    embedding per mask, table E_v [M_v, dim] (SAM masks with a CLIP / LSeg vector each, superpixel-pooled DINO features).  The
    result equals create_feature_field(feature_fn=lambda v: E_v[L_v]) -- a zero row wherever a label lies outside [0, M_v), whose
    weight still counts in d -- up to the order of the sums, and is finalised the same way (L2-normalised, NaN -> 0), without the
    [H, W, dim] map: per (Gaussian, tile) record the weights are summed by label (csrc/mask_features.hip) and every F row that
    receives weight gets one read-modify-write per view from the table rows.

    mask_fn(v) -> (labels, table): labels [height, width] (with upsample="nearest": any [h, w], read with F.interpolate's nearest
    rule) on the device, uint8, bool, int16 or int32 read as stored, int64 narrowed; table [M_v, dim] float32, float16 or bfloat16
    with unit channel stride (a half table is widened as it is read: F equals that of table.float()).  M_v may differ per view.
    A dim that is no multiple of 4 materialises E_v[L_v] per view and takes the feature scatter (same F and d).
    reduction: "sum" or "mean", with create_feature_field's scales (the D of 1/(H W D) is dim).
    views, pipeline (True, an int >= 2 workspaces, or False), gather, return_partials, camera_model, rasterize_mode, engine,
    pixel_weight_fn: as create_feature_field.  stats (return_partials) gains "mask_spilled": records with more than four
    distinct labels, whose rest was added with atomics (F is then no longer the same bit for bit from run to run).
    render_colors / sh_degree: as create_feature_field's -- mask_fn is then called as mask_fn(v, image) with the view's RGB
    render, made by the front stage's blend; mask_fn may be called more than once per view (an overflow restarts the job).
    out_dtype: as create_feature_field's -- the finalised field in float32, float16 or bfloat16; the accumulators stay float32."""
    if out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"out_dtype must be torch.float32, torch.float16 or torch.bfloat16, got {out_dtype}")
    if upsample not in (None, "nearest"):
        raise ValueError(f"upsample must be None or 'nearest' for mask maps, got {upsample!r}")
    render = _render_of(render_colors, sh_degree, means.shape[0], means.device)
    if reduction not in ("sum", "mean"):
        raise ValueError(reduction)
    dim = int(dim)
    if dim < 1:
        raise ValueError(f"dim must be positive, got {dim}")
    dist, rank, world = _dist()
    n = means.shape[0]
    F, d, F_store = alloc_accumulators(n, dim, means.device, world)
    sf, sd = (1.0, 1.0) if reduction == "sum" else (1.0 / (height * width * dim), 1.0 / (height * width * 3))
    job = _Job((means, quats, scales, opacities), F, d, sf, sd, mask_fn,
               list(views) if views is not None else view_shard(viewmats.shape[0], rank, world),
               viewmats.detach().cpu(), K.detach().cpu(), width, height,
               dict(camera_model=camera_model, rasterize_mode=rasterize_mode), None, upsample, pixel_weight_fn, render)
    pipelined = bool(pipeline) and len(job.view_ids) > 1
    if pipelined and _lib.hw_queues_late():
        warnings.warn("gsbp_amd was imported after the HIP runtime had started: create_mask_feature_field runs its views on ONE "
                      "stream", RuntimeWarning, stacklevel=2)
        pipelined = False
    depth = (pipeline_depth(n, width, height) if pipeline is True else max(2, int(pipeline))) if pipelined else 1
    eng = engine or Engine(n, width, height, device=means.device, tight_binning=True)
    stats: Dict[str, int] = {}
    for attempt in range(6):  # a capacity overflow invalidates the accumulators: grow the workspace, start over
        stats = _run_masks_pipelined(job, eng, depth, dim) if pipelined else _run_masks_serial(job, eng, dim)
        if _overflow_action(stats["overflow"], False, attempt) is None:
            break
        eng.grow(stats, views=len(job.view_ids))
        F.zero_()
        d.zero_()
    F_rows, d_rows, row0 = reduce_partials_sharded(F, d, F_store)
    out_rows = eng.finalize(F_rows, d_rows) if out_dtype == torch.float32 else eng.finalize_typed(F_rows, d_rows, out_dtype)
    out = gather_rows(out_rows, n) if gather else out_rows
    if return_partials:
        return out, F_rows, d, dict(stats, row0=row0)
    return out


def prune_mask(d: torch.Tensor) -> torch.Tensor:
    """utils.prune_by_gradients (utils.py:222-271) keeps Gaussians whose accumulated colour-gradient norm is
    > 0 over all views; that norm is 2/(3HW) * sum_v sum_p w, i.e. the mask is exactly d > 0."""
    return d > 0


# ---- 3-D masks from 2-D masks by per-view voting (the binary / projection / gradient votes of a masklet lift) ------------------
VOTE_METHODS = ("binary", "projection", "gradient")


class _VotePipeline(_LabelPipeline):
    """The ViewPipeline of create_vote_field(method="binary"): the front stage blends a weight store WITHOUT the denominators
    (n counts views, not weight: no gwbp_blend_weights_d, hence no half-tile lists either), the scatter stage is
    Engine.vote_labels -- the bitset kernel and its commit -- into C and n."""

    def choose_scatter_kernel(self, n_pairs, n_headers) -> str:
        self.wide = False  # (what front() reads: the blend adds nothing to d)
        for e in self.eng:
            e.set_narrow_scatter(True)
            e.set_front_priority(False)
        return "votes"

    def _scatter_on(self, main, b, labels, C, n, scale_f, scale_d, t0, t1, upsample, encoder):
        e = self.eng[b]
        if t0 is not None:
            t0.record(main)
        p = self.pending.pop(self.i_scatter)
        e.vote_labels(p.view, labels, C, n, self.num_classes, upsample=upsample)
        if t1 is not None:
            t1.record(main)
        e.accumulate_stats(self.accums[0])


def _run_votes_serial(job: _Job, eng: Engine, num_classes: int) -> Dict[str, int]:
    """The binary vote's views one after the other on the caller's stream (synchronises)."""
    accum = torch.zeros(32, dtype=torch.uint8, device=job.F.device)
    for v in job.view_ids:
        view = eng.view(job.vm_host[v], job.K_host, job.width, job.height, **job.camera)
        if job.render is not None:  # the blend composites the render; the labels are made from it behind the blend
            eng.project(view, *job.gaussians)
            eng.bin_sort(view)
            labels = job.feature_fn(v, _blend_rendered(eng, job, v, view))
        else:
            labels = job.feature_fn(v)
            eng.project(view, *job.gaussians)
            eng.bin_sort(view)
            if job.pixel_weight_fn is not None:
                eng.blend_weighted(view, job.pixel_weight_fn(v))
            else:
                eng.blend_weights(view)
        eng.vote_labels(view, labels, job.F, job.d, num_classes, upsample=job.upsample)
        eng.accumulate_stats(accum)
    return Engine.decode_stats(accum)


def _run_votes_projected(job: _Job, eng: Engine, num_classes: int) -> Dict[str, int]:
    """The projection vote: per view project -> vote (no sort, no blend); a job that renders also sorts the view and renders it
    with render_pixels before label_fn(v, image).  Only the render can overflow a capacity (synchronises)."""
    accum = torch.zeros(32, dtype=torch.uint8, device=job.F.device)
    for v in job.view_ids:
        view = eng.view(job.vm_host[v], job.K_host, job.width, job.height, **job.camera)
        if job.render is not None:
            labels = job.feature_fn(v, _render_view(eng, job, v, view))
            eng.accumulate_stats(accum)
        else:
            labels = job.feature_fn(v)
            eng.project(view, *job.gaussians)
        pw = job.pixel_weight_fn(v) if job.pixel_weight_fn is not None else None
        eng.vote_projected(view, labels, job.F, job.d, num_classes, upsample=job.upsample, pixel_weights=pw)
    return Engine.decode_stats(accum)


def create_vote_field(means, quats, scales, opacities, viewmats, K, width: int, height: int,
                      label_fn: Callable[[int], torch.Tensor], num_classes: int, *, method: str = "binary",
                      upsample: Optional[str] = None, views: Optional[Sequence[int]] = None, pipeline: bool = True,
                      gather: bool = True, return_partials: bool = False, camera_model: str = "pinhole",
                      rasterize_mode: str = "classic", engine: Optional[Engine] = None,
                      pixel_weight_fn: Optional[Callable[[int], torch.Tensor]] = None,
                      render_colors: Optional[torch.Tensor] = None, sh_degree: Optional[int] = None):
    """Per-Gaussian VOTES of per-view label maps (a segmenter's masks or masklets): returns (C, n), C float32 [N, num_classes],
    n float32 [N].  The 3-D mask of two classes is mask3d_from_votes(C): votes = C[:, 1] - C[:, 0] > 0.
      method="binary":     C[g, k] = number of views in which g has at least one contributing pixel (w = alpha T > 0) of label k,
                           n[g] = number of views in which g has any contributing pixel (Engine.vote_labels: a bitset per view
                           over the weight store, no float atomic per pixel).
      method="projection": per view, a Gaussian with radius > 0 whose centre, rounded half to even (np.round of means2d), lies in
                           the image adds 1 to C[g, label there] and to n[g] (Engine.vote_projected: no sort, no blend).
      method="gradient":   C and n are create_label_field's raw sums F and d (sum_v sum_p w [L_v(p) == k] and sum_v sum_p w).
    A label outside [0, num_classes) is ignored: it counts in n and in no column.  Counts are exact up to 2^24 views.
    label_fn, upsample, views, pipeline, gather, camera_model, rasterize_mode, engine, pixel_weight_fn, render_colors / sh_degree:
    as create_label_field (label_fn(v, image) with render_colors).  With pixel_weight_fn a pixel of weight 0 casts no vote: for
    "binary" only entries with w c(p) > 0 vote, for "projection" a Gaussian whose pixel has c <= 0 does not vote at all.
    pipeline applies to "binary" and "gradient"; "projection" is one short kernel per view.
    return_partials: also return the counters, (C, n, stats) with stats["row0"] (C is this rank's row block when gather=False).
    A capacity overflow grows the workspace and starts over with C and n zeroed; if no attempt finishes cleanly it raises."""
    if method not in VOTE_METHODS:
        raise ValueError(f"method must be one of {VOTE_METHODS}, got {method!r}")
    if upsample not in (None, "nearest"):
        raise ValueError(f"upsample must be None or 'nearest' for label maps, got {upsample!r}")
    if isinstance(num_classes, bool) or int(num_classes) < 1:
        raise ValueError(f"num_classes must be a positive int, got {num_classes!r}")
    kw = dict(upsample=upsample, views=views, pipeline=pipeline, camera_model=camera_model, rasterize_mode=rasterize_mode,
              engine=engine, pixel_weight_fn=pixel_weight_fn, render_colors=render_colors, sh_degree=sh_degree)
    n_g = means.shape[0]
    if method == "gradient":  # the raw label-field sums: no kernel of its own
        _, C_rows, n_all, stats = create_label_field(means, quats, scales, opacities, viewmats, K, width, height, label_fn,
                                                     num_classes, gather=False, return_partials=True, **kw)
        row0 = stats["row0"]
    else:
        render = _render_of(render_colors, sh_degree, n_g, means.device)
        dist, rank, world = _dist()
        Cacc, n_acc, C_store = alloc_accumulators(n_g, int(num_classes), means.device, world)
        job = _Job((means, quats, scales, opacities), Cacc, n_acc, 1.0, 1.0, label_fn,
                   list(views) if views is not None else view_shard(viewmats.shape[0], rank, world),
                   viewmats.detach().cpu(), K.detach().cpu(), width, height,
                   dict(camera_model=camera_model, rasterize_mode=rasterize_mode), None, upsample, pixel_weight_fn, render)
        pipelined = method == "binary" and bool(pipeline) and len(job.view_ids) > 1
        if pipelined and _lib.hw_queues_late():
            warnings.warn("gsbp_amd was imported after the HIP runtime had started: create_vote_field runs its views on ONE "
                          "stream", RuntimeWarning, stacklevel=2)
            pipelined = False
        depth = (pipeline_depth(n_g, width, height) if pipeline is True else max(2, int(pipeline))) if pipelined else 1
        eng = engine or Engine(n_g, width, height, device=means.device, tight_binning=True)
        stats: Dict[str, int] = {}
        clean = False
        for attempt in range(6):  # a capacity overflow invalidates the counts: grow the workspace, start over
            if method == "projection":
                stats = _run_votes_projected(job, eng, int(num_classes))
            elif pipelined:
                stats = _run_labels_pipelined(job, eng, depth, int(num_classes), pipe_cls=_VotePipeline)
            else:
                stats = _run_votes_serial(job, eng, int(num_classes))
            if _overflow_action(stats["overflow"], False, attempt) is None:
                clean = True
                break
            eng.grow(stats, views=len(job.view_ids))
            Cacc.zero_()
            n_acc.zero_()
        if not clean:
            raise RuntimeError(f"create_vote_field: no pass over the views finished without a workspace overflow "
                               f"(flags {stats.get('overflow')})")
        C_rows, n_rows, row0 = reduce_partials_sharded(Cacc, n_acc, C_store)
        n_all = n_acc
    C_out = gather_rows(C_rows, n_g) if gather else C_rows
    n_out = n_all if gather else n_all[row0:row0 + C_rows.shape[0]]
    if return_partials:
        return C_out, n_out, dict(stats, row0=row0)
    return C_out, n_out


def mask3d_from_votes(C: torch.Tensor, positive: int = 1, negative: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mask3d, mask3d_inverted) of get_mask3d: votes = C[:, positive] - C[:, negative], mask3d = votes > 0,
    mask3d_inverted = votes < 0 (Gaussians that never voted, or as often for both classes, are in neither)."""
    if not torch.is_tensor(C) or C.dim() != 2:
        raise ValueError(f"C must be an [N, K] tensor of votes, got {type(C).__name__ if not torch.is_tensor(C) else tuple(C.shape)}")
    K = C.shape[1]
    for name, col in (("positive", positive), ("negative", negative)):
        if isinstance(col, bool) or not isinstance(col, int) or not 0 <= col < K:
            raise ValueError(f"{name} must be a column index in [0, {K}), got {col!r}")
    if positive == negative:
        raise ValueError(f"positive and negative must be different columns, got {positive} for both")
    votes = C[:, positive] - C[:, negative]
    return votes > 0, votes < 0
