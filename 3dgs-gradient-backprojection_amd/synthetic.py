"""Seeded synthetic scenes, cameras and feature maps for the BASELINE.json configs.

The reference runs on a trained garden scene + COLMAP poses + LSeg features (backproject.py:43-58,74,83-113);
none of those exist offline, so BASELINE.md section 4 / SURVEY.md section 8(d) define statistically similar seeded
inputs.  Everything here is generated on the CPU with explicit torch generators so that the CPU oracle and
the GPU path see bit-identical inputs; the large throughput-only feature maps may be generated on device.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

SCENE_SEED = 1234
CAMERA_SEED = 99
FEATURE_SEED0 = 10_000
ENCODER_SEED = 7


@dataclass(frozen=True)
class Config:
    name: str
    n_gaussians: int
    n_views: int
    width: int
    height: int
    feat_dim: int
    log_scale0: float  # median scale s0 (world units)
    garden: bool  # 70 % volume + 30 % ground disc
    encoder_dim: Optional[int] = None  # backproject_compressed.py: 512 -> 16
    # the 2-D network's OWN map shape, where the reference upsamples it to the view (None: the map is given at view resolution)
    lowres: Optional[tuple] = None     # (h, w) of the network map
    upsample: Optional[str] = None     # "nearest" (dino, backproject.py:244-248) | "bilinear" (lseg, backproject.py:110-112)
    reduction: str = "sum"             # "sum" (lseg, backproject.py:127,145) | "mean" (dino, backproject.py:263,283)
    normalize: bool = True             # L2-normalise over channels (lseg, backproject.py:109); dino's patch tokens are not


# BASELINE.json "configs" in order (C3 = C2 sharded over ranks).
CONFIGS: Dict[str, Config] = {
    "C1": Config("C1", 10_000, 4, 400, 300, 32, 0.03, False),
    "C2": Config("C2", 1_000_000, 200, 1600, 1060, 512, 0.004, True),
    "C4": Config("C4", 5_000_000, 300, 1600, 1060, 768, 0.002, True),
    "C5": Config("C5", 1_000_000, 200, 1600, 1060, 512, 0.004, True, encoder_dim=16),
    # The reference's feature maps AS THE REFERENCE PRODUCES THEM, at C2 geometry (a1 / a7 "as the reference runs them"):
    # dino: 64 x 64 x 1024 patch tokens, nearest-upsampled, .mean() reductions (backproject.py:201,242-249,263,283)
    "DINO64": Config("DINO64", 1_000_000, 200, 1600, 1060, 1024, 0.004, True, lowres=(64, 64), upsample="nearest",
                     reduction="mean", normalize=False),
    # ... and the same loop with the other DINOv2 backbones' widths (vits14 384, vitb14 768, vitg14 1536; 64 x 64 tokens each)
    "DINO64S": Config("DINO64S", 1_000_000, 200, 1600, 1060, 384, 0.004, True, lowres=(64, 64), upsample="nearest",
                      reduction="mean", normalize=False),
    "DINO64B": Config("DINO64B", 1_000_000, 200, 1600, 1060, 768, 0.004, True, lowres=(64, 64), upsample="nearest",
                      reduction="mean", normalize=False),
    "DINO64G": Config("DINO64G", 1_000_000, 200, 1600, 1060, 1536, 0.004, True, lowres=(64, 64), upsample="nearest",
                      reduction="mean", normalize=False),
    # lseg: 480 x 480 x 512 normalised map, bilinearly upsampled, .sum() reductions (backproject.py:102-113,127,145)
    "LSEG480": Config("LSEG480", 1_000_000, 200, 1600, 1060, 512, 0.004, True, lowres=(480, 480), upsample="bilinear"),
    # small shapes used by the parity tests and smoke()
    "T0": Config("T0", 512, 2, 96, 64, 8, 0.06, False),
    "T1": Config("T1", 4_000, 2, 200, 136, 24, 0.04, True),
    # T1 with a dino-shaped map: 8 x 12 x 256 tokens (17 x 16.7 pixel texels: at least a tile), nearest, .mean() -> token space
    "T1D": Config("T1D", 4_000, 2, 200, 136, 256, 0.04, True, lowres=(8, 12), upsample="nearest", reduction="mean",
                  normalize=False),
}


def make_scene(cfg: Config, seed: int = SCENE_SEED) -> Dict[str, torch.Tensor]:
    """Pre-activation splat dict with the reference's key names (utils.py:56-67,105-107)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = cfg.n_gaussians
    means = torch.rand(n, 3, generator=g) * 2.0 - 1.0
    if cfg.garden:
        n_ground = int(0.3 * n)
        r = 1.5 * torch.sqrt(torch.rand(n_ground, generator=g))
        th = 2.0 * math.pi * torch.rand(n_ground, generator=g)
        z = -1.0 + 0.1 * torch.rand(n_ground, generator=g)
        means[:n_ground] = torch.stack([r * torch.cos(th), r * torch.sin(th), z], dim=1)
    scaling = math.log(cfg.log_scale0) + 0.5 * torch.randn(n, 3, generator=g)
    rotation = torch.randn(n, 4, generator=g)  # unnormalised on purpose (backproject.py:57)
    opacity = 2.0 * torch.randn(n, generator=g)  # logits
    return {
        "means": means.contiguous(),
        "scaling": scaling.contiguous(),
        "rotation": rotation.contiguous(),
        "opacity": opacity.contiguous(),
    }


def activate(splats: Dict[str, torch.Tensor]):
    """backproject.py:55-57: opacities = sigmoid, scales = exp, quats raw."""
    return (
        splats["means"],
        splats["rotation"],
        torch.exp(splats["scaling"]),
        torch.sigmoid(splats["opacity"]),
    )


def intrinsics(cfg: Config) -> torch.Tensor:
    K = torch.zeros(3, 3)
    K[0, 0] = K[1, 1] = 1.2 * cfg.width
    K[0, 2] = cfg.width / 2.0  # cx = W/2, cy = H/2 exactly (backproject.py:85-86 inverts this)
    K[1, 2] = cfg.height / 2.0
    K[2, 2] = 1.0
    return K


def make_cameras(cfg: Config, seed: int = CAMERA_SEED, n_views: Optional[int] = None) -> torch.Tensor:
    """[V,4,4] world->camera matrices, OpenCV convention (utils.py:215-219 layout [R|t; 0 0 0 1])."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    v = cfg.n_views if n_views is None else n_views
    az = 2.0 * math.pi * torch.rand(v, generator=g)
    el = torch.deg2rad(10.0 + 30.0 * torch.rand(v, generator=g))
    rad = 3.5 * (1.0 + 0.1 * (2.0 * torch.rand(v, generator=g) - 1.0))
    return _look_at_origin(az, el, rad)


def _look_at_origin(az: torch.Tensor, el: torch.Tensor, rad: torch.Tensor) -> torch.Tensor:
    """[V,4,4] world->camera matrices of cameras at azimuth / elevation (radians) / distance that look at the origin, z up."""
    v = az.shape[0]
    c = torch.stack([rad * torch.cos(el) * torch.cos(az), rad * torch.cos(el) * torch.sin(az), rad * torch.sin(el)], 1)
    fwd = -c / c.norm(dim=1, keepdim=True)  # look at the origin
    up = torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd)
    right = torch.linalg.cross(fwd, up)
    right = right / right.norm(dim=1, keepdim=True)
    down = torch.linalg.cross(fwd, right)
    R = torch.stack([right, down, fwd], dim=1)  # rows = right, down, forward
    t = -(R @ c[:, :, None])[:, :, 0]
    vm = torch.zeros(v, 4, 4)
    vm[:, :3, :3] = R
    vm[:, :3, 3] = t
    vm[:, 3, 3] = 1.0
    return vm.contiguous()


def make_orbit(cfg: Config, n_views: int, elevation_deg: float = 25.0, radius: float = 3.5) -> torch.Tensor:
    """[n_views,4,4] world->camera matrices of an orbit: evenly spaced azimuths at one elevation and distance, looking at the
    origin like make_cameras' (consecutive views overlap, which a sequential association of per-view masks relies on)."""
    az = 2.0 * math.pi * torch.arange(n_views, dtype=torch.float32) / float(n_views)
    el = torch.deg2rad(torch.full((n_views,), float(elevation_deg)))
    return _look_at_origin(az, el, torch.full((n_views,), float(radius)))


INSTANCE_SEED = 60_000


def make_instances(means: torch.Tensor, n_instances: int = 4, seed: int = INSTANCE_SEED) -> torch.Tensor:
    """int32 [N] true instance of every Gaussian: the 3-D Voronoi cells of n_instances seeded sites in the means' bounding box."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    m = means.detach().cpu().float()
    lo, hi = m.min(dim=0).values, m.max(dim=0).values
    sites = lo + (hi - lo) * torch.rand(n_instances, 3, generator=g)
    return torch.cdist(m, sites).argmin(dim=1).to(torch.int32)


def make_instance_views(cfg: Config, viewmats: torch.Tensor, n_instances: int = 4, seed: int = INSTANCE_SEED, n_ids: Optional[int] = None,
                        device=None, argmax_fn=None):
    """(instance int32 [N], maps, perms): per-view instance maps as an "everything" segmenter gives them, ids unrelated between
    views.  instance = make_instances(means of make_scene(cfg)); view v's map is the argmax instance per pixel, -1 where the
    pixel's alpha lies below 0.5, with the ids renamed by perms[v], a seeded permutation (seed + 1 + v) of [0, n_ids) (n_ids
    defaults to n_instances): map = perms[v][instance id].  Rendered on `device` by the package's label render; with
    argmax_fn(v, instance) -> (argmax integer [H, W], alphas [H, W]) by the caller instead (the CPU oracle's render in the tests).
    maps: int32 [H, W] tensors on `device` (on the host with argmax_fn and no device)."""
    means, quats, scales, opac = activate(make_scene(cfg))
    instance = make_instances(means, n_instances, seed)
    n_ids = n_instances if n_ids is None else int(n_ids)
    if n_ids < n_instances:
        raise ValueError("n_ids must be at least n_instances")
    K = intrinsics(cfg)
    if argmax_fn is None:
        from ._views import front
        gauss = [t.to(device) for t in (means, quats, scales, opac)]
        inst_dev, K = instance.to(device), K.to(device)
    maps, perms = [], []
    for v in range(viewmats.shape[0]):
        if argmax_fn is None:
            eng, view, _ = front("make_instance_views", *gauss, viewmats[v].to(device), K, cfg.width, cfg.height, {})
            _, alphas, seg, _ = eng.render_labels(view, inst_dev, n_instances, want_maps=False, want_alphas=True, want_argmax=True)
        else:
            seg, alphas = (torch.as_tensor(t) for t in argmax_fn(v, instance))
            if device is not None:
                seg, alphas = seg.to(device), alphas.to(device)
        perm = torch.randperm(n_ids, generator=torch.Generator(device="cpu").manual_seed(seed + 1 + v)).to(torch.int32)
        seg = seg.to(torch.int64)
        ok = (seg >= 0) & (alphas >= 0.5)
        maps.append(torch.where(ok, perm.to(seg.device)[torch.where(ok, seg, 0)], -1).to(torch.int32))
        perms.append(perm)
    return instance, maps, perms


def make_feature_map(cfg: Config, view: int, device="cpu", dim: Optional[int] = None) -> torch.Tensor:
    """[H,W,D] fp32, N(0,1) then L2-normalised over D (mimics backproject.py:109); seed = 10000 + view.  Configs with a
    `lowres` shape return the network's own [h,w,D] map (what the reference upsamples to the view)."""
    d = cfg.feat_dim if dim is None else dim
    g = torch.Generator(device=device).manual_seed(FEATURE_SEED0 + view)
    h, w = cfg.lowres if cfg.lowres else (cfg.height, cfg.width)
    f = torch.randn(h, w, d, generator=g, device=device)
    if cfg.normalize:
        f /= f.norm(dim=-1, keepdim=True)
    return f


LABEL_SEED0 = 20_000


def make_label_map(cfg: Config, view: int, num_classes: int, device="cpu", n_seeds: int = 200, per_pixel: bool = False,
                   size: Optional[tuple] = None) -> torch.Tensor:
    """[H,W] int32 label map of view `view` (seed 20000 + view) with ids in [0, num_classes): piecewise constant -- the Voronoi
    cells of `n_seeds` random points, each cell one random id, like a segmenter's regions -- or, with per_pixel=True, an
    independent random id per pixel (the worst case of a per-record reduction by label).  size=(h, w): a map of that shape
    instead of the view's (a low-resolution segmenter output)."""
    h, w = size if size is not None else (cfg.height, cfg.width)
    g = torch.Generator(device="cpu").manual_seed(LABEL_SEED0 + view)
    if per_pixel:
        return torch.randint(0, num_classes, (h, w), generator=g, dtype=torch.int32).to(device)
    pts = torch.rand(n_seeds, 2, generator=g) * torch.tensor([float(h), float(w)])
    ids = torch.randint(0, num_classes, (n_seeds,), generator=g, dtype=torch.int32)
    pts, ids = pts.to(device), ids.to(device)
    ys = torch.arange(h, device=device, dtype=torch.float32) + 0.5
    xs = torch.arange(w, device=device, dtype=torch.float32) + 0.5
    out = torch.empty(h, w, dtype=torch.int32, device=device)
    step = max(1, (1 << 22) // max(1, w * n_seeds))  # rows per block: a [rows, w, n_seeds] distance table of ~16 MB
    for y0 in range(0, h, step):
        dy = (ys[y0:y0 + step, None, None] - pts[:, 0]) ** 2
        dx = (xs[None, :, None] - pts[:, 1]) ** 2
        out[y0:y0 + step] = ids[(dy + dx).argmin(dim=-1)]
    return out


MASK_TABLE_SEED0 = 40_000


def make_mask_features(cfg: Config, view: int, n_masks: int, dim: int, device="cpu", per_pixel: bool = False,
                       size: Optional[tuple] = None):
    """(labels, table) of view `view` for create_mask_feature_field: a [H,W] int32 map of mask ids in [0, n_masks) --
    make_label_map's Voronoi cells (n_masks seeds, so about one cell per mask) or, with per_pixel=True, a random id per pixel --
    and a [n_masks, dim] fp32 table of N(0,1) rows L2-normalised like a CLIP / LSeg embedding (seed 40000 + view).  size=(h, w):
    a low-resolution map of that shape."""
    labels = make_label_map(cfg, view, n_masks, device=device, n_seeds=n_masks, per_pixel=per_pixel, size=size)
    g = torch.Generator(device="cpu").manual_seed(MASK_TABLE_SEED0 + view)
    table = torch.randn(n_masks, dim, generator=g)
    table /= table.norm(dim=-1, keepdim=True)
    return labels, table.to(device)


PIXEL_WEIGHT_SEED0 = 30000


def make_pixel_weights(cfg: Config, view: int, device="cpu", kind: str = "mask", border: float = 0.05,
                       n_seeds: int = 40) -> torch.Tensor:
    """[H,W] per-pixel weight map of view `view` (seed 30000 + view) for create_feature_field(pixel_weight_fn=...): a band of
    `border` x the smaller side along the image edges (an undistortion border) and one of the Voronoi cells of `n_seeds` random
    points (a transient) are 0, everything else 1.  kind="mask": bool; kind="confidence": float32, the mask times a uniform
    random value in [0.25, 1) per pixel."""
    h, w = cfg.height, cfg.width
    g = torch.Generator(device="cpu").manual_seed(PIXEL_WEIGHT_SEED0 + view)
    b = int(border * min(h, w))
    keep = torch.zeros(h, w, dtype=torch.bool)
    keep[b:h - b, b:w - b] = True
    pts = torch.rand(n_seeds, 2, generator=g) * torch.tensor([float(h), float(w)])
    ys = torch.arange(h, dtype=torch.float32)[:, None, None] + 0.5
    xs = torch.arange(w, dtype=torch.float32)[None, :, None] + 0.5
    cell = ((ys - pts[:, 0]) ** 2 + (xs - pts[:, 1]) ** 2).argmin(dim=-1)
    keep &= cell != int(torch.randint(0, n_seeds, (1,), generator=g))
    if kind == "mask":
        return keep.to(device)
    if kind != "confidence":
        raise ValueError(f"kind must be 'mask' or 'confidence', got {kind!r}")
    conf = 0.25 + 0.75 * torch.rand(h, w, generator=g)
    return (conf * keep).to(device)


def upsample_map(cfg: Config, low: torch.Tensor) -> torch.Tensor:
    """The reference's own upsampling of a network map to the view ([h,w,D] -> [H,W,D]): F.interpolate(mode=cfg.upsample)
    (backproject.py:110-112 bilinear, align_corners=False; :244-248 nearest).  Used by checks and the CPU baseline, which
    back-project the materialised map like the reference does."""
    if cfg.upsample is None:
        return low
    kw = {"align_corners": False} if cfg.upsample == "bilinear" else {}
    up = torch.nn.functional.interpolate(low.permute(2, 0, 1)[None], size=(cfg.height, cfg.width), mode=cfg.upsample, **kw)
    return up[0].permute(1, 2, 0)


SH_SEED = 40000


def make_sh_coeffs(cfg: Config, degree: int = 3, device="cpu", seed: int = SH_SEED) -> torch.Tensor:
    """[N, (degree+1)^2, 3] SH coefficients (a trained scene's colors_all, backproject.py:59-60): a DC term that puts the base
    colour in [0, 1] after gsplat's +0.5, higher bands decaying with the degree.  For create_feature_field(render_colors=...)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = (degree + 1) ** 2
    sh = torch.randn(cfg.n_gaussians, k, 3, generator=g)
    band = torch.tensor([math.floor(math.sqrt(i)) for i in range(k)], dtype=torch.float32)
    sh *= (0.3 / (1.0 + band))[None, :, None]
    sh[:, 0] = (torch.rand(cfg.n_gaussians, 3, generator=g) - 0.5) / 0.28209479177387814
    return sh.contiguous().to(device)


def make_encoder(cfg: Config, seed: int = ENCODER_SEED) -> torch.Tensor:
    """Random stand-in for encoder_decoder.ckpt's encoder (backproject_compressed.py:26,127)."""
    assert cfg.encoder_dim is not None
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(cfg.feat_dim, cfg.encoder_dim, generator=g) / math.sqrt(cfg.feat_dim)


PROMPT_SEED = 31


def make_prompts(features: torch.Tensor, n_prompts: int = 4, n_pos: int = 1, seed: int = PROMPT_SEED):
    """Stand-ins for the text embeddings of segment.py (no text encoder exists here): `n_prompts` seeded rows of the finished
    field, each normalised to unit length, the first `n_pos` of them the positive prompts.  Rows without length are skipped.
    Returns (prompts [P, D] float32 on the host, n_pos)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    f = features.detach().float().cpu()
    live = torch.nonzero(f.norm(dim=1) > 0)[:, 0]
    assert live.numel() >= n_prompts >= n_pos >= 1
    pick = live[torch.randperm(live.numel(), generator=g)[:n_prompts]]
    return torch.nn.functional.normalize(f[pick], dim=1).contiguous(), int(n_pos)


def view_shard(n_views: int, rank: int, world: int) -> List[int]:
    """Views r, r+R, r+2R, ... (interleaved to balance scene coverage)."""
    return list(range(rank, n_views, world))
