"""Ask a finished feature field a question: prompt segmentation and clicks (the reference's segment.py, segment_compressed.py and
click_and_segment.py without their text encoder and windows).  Prompts are embedding vectors.

    scores = prompt_scores(features, prompts)                      # F.normalize(features) @ prompts.T, one pass, no second field
    mask3d = prompt_mask(features, prompts, n_pos, threshold=None)  # get_mask3d_lseg: best positive beats best negative
    feats, depth, alpha = probe_pixels(means, quats, scales, opacities, features, viewmat, K, W, H, xy)   # a click
    for mask2d, frame in render_prompt_mask(means, quats, scales, opacities, features, viewmats, K, W, H, prompts, n_pos): ...
    session = ClickSession(features); session.add_positive(feats[0]); mask3d = session.mask()
    extracted, deleted = apply_mask3d(splats, mask3d)

prompt_scores / prompt_mask run gwbp_prompt_scores and probe_pixels runs gwbp_probe_pixels (csrc/query.hip) on the caller's current
stream.  The 2-D mask of a frame is a P-channel render: max_pos > max_neg is invariant under the positive per-pixel normalisation of
the rendered feature, and rendering is linear, so mask2d = (best positive > best negative) of render(features @ prompts.T) -- the
[H, W, D] image of the reference is never made.  There is no PyTorch fallback: CPU tensors raise, and so does a missing library.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterator, List, Optional, Tuple

import torch

from ._lib import GwbpError, ptr
from ._views import field_rows, front, ld, require_device, run
from ._views import raster_kw as merged_raster_kw
from .pruning import PER_GAUSSIAN

MAX_P = 32            # GWBP_QUERY_MAX_P
MAX_D = 2048          # GWBP_PCA_MAX_D
MAX_PROBES = 4096     # GWBP_PROBE_MAX_PIXELS


def _prompts(prompts, d: int, device) -> torch.Tensor:
    if not torch.is_tensor(prompts) or prompts.dim() != 2:
        raise GwbpError("prompts must be a [P, D] tensor of embedding vectors")
    p = prompts.shape[0]
    if not 1 <= p <= MAX_P:
        raise GwbpError(f"the number of prompts must be in [1, {MAX_P}], got {p}")
    if prompts.shape[1] != d:
        raise GwbpError(f"features have D = {d}, prompts D = {prompts.shape[1]}")
    return prompts.to(device=device, dtype=torch.float32).contiguous()


def _query(features, prompts, n_pos: int, threshold, normalize: bool, want_mask: bool, want_scores: bool):
    x, ft = field_rows(features, "features")  # float16 / bfloat16 fields are read as stored: no float32 copy
    n, d = x.shape
    if d > MAX_D:
        raise GwbpError(f"D must be in [1, {MAX_D}], got {d}")
    t = _prompts(prompts, d, x.device)
    p, n_pos = t.shape[0], int(n_pos)
    if not 1 <= n_pos <= p:
        raise GwbpError(f"n_pos must be in [1, P = {p}], got {n_pos}")
    if want_mask and n_pos == p and threshold is None:
        raise GwbpError("a mask without negative prompts (n_pos == P) needs a threshold")
    thr = C.byref(C.c_float(float(threshold))) if threshold is not None else None
    mask = torch.empty(n, dtype=torch.uint8, device=x.device) if want_mask else None
    scores = torch.empty(n, p, dtype=torch.float32, device=x.device) if want_scores else None
    run("gwbp_prompt_scores_typed", x.device, C.c_int64(n), d, p, n_pos, ptr(x), ft, C.c_int64(ld(x)), ptr(t), int(bool(normalize)),
        thr, ptr(mask), ptr(scores))
    return mask, scores


def prompt_scores(features: torch.Tensor, prompts: torch.Tensor, normalize: bool = True) -> torch.Tensor:
    """scores [N, P]: features[g] . prompts[j] / max(|features[g]|, 1e-12) (F.normalize(features) @ prompts.T; a zero row scores
    0), or the bare dot products with normalize=False.  One pass over the field, exact fp32, bit-reproducible.  features: as
    knn_search (any row stride >= D, read in place; D <= 2048); 1 <= P <= 32."""
    return _query(features, prompts, 1, None, normalize, False, True)[1]


def prompt_mask(features: torch.Tensor, prompts: torch.Tensor, n_pos: int, threshold: Optional[float] = None,
                normalize: bool = True) -> torch.Tensor:
    """get_mask3d_lseg (segment.py:26-67) from its embeddings: bool [N], True where the best of the first n_pos prompts scores above
    the best of the others -- and, with a threshold, where prompt 0 scores above it.  n_pos == P (no negatives) is the threshold
    test alone and needs one.  A NaN score loses.  The field is read once, in place, whatever its row stride."""
    return _query(features, prompts, n_pos, threshold, normalize, True, False)[0].bool()


def mask_from_scores(scores: torch.Tensor, n_pos: int, threshold: Optional[float] = None) -> torch.Tensor:
    """The mask rule on a [..., P] score tensor in torch (the per-frame epilogue of render_prompt_mask; torch.max propagates NaN
    exactly as the kernel's maxima do)."""
    p = scores.shape[-1]
    if n_pos < p:
        mask = scores[..., :n_pos].max(dim=-1)[0] > scores[..., n_pos:].max(dim=-1)[0]
    else:
        if threshold is None:
            raise GwbpError("a mask without negative prompts (n_pos == P) needs a threshold")
        mask = torch.ones(scores.shape[:-1], dtype=torch.bool, device=scores.device)
    if threshold is not None:
        mask = mask & (scores[..., 0] > threshold)
    return mask


# ---- the field at a few pixels ---------------------------------------------------------------------------------------------------

def probe_pixels(means, quats, scales, opacities, features, viewmat, K, width, height, xy, **raster_kw):
    """(feats [M, D], depth [M], alpha [M]) of the pixels xy [M, 2] ((x, y) integers) of one view: what
    rasterization(..., colors=features, render_mode="RGB+D") holds at [0, y, x] -- bit for bit -- without rendering the other
    H W - M pixels (click_and_segment.py:241-262).  features: float32, float16 or bfloat16 [N, D], read as stored (a half field gives
    the bits of features.float(), and float32 feats).  A pixel outside the image gives zeros.  depth is gsplat's accumulated "D"
    channel, not the expected depth.  raster_kw: near_plane, far_plane, eps2d, radius_clip, camera_model, rasterize_mode.  The
    engine and the front cache are rasterization()'s: a probe after a rendered frame of the same view re-projects nothing."""
    require_device("probe_pixels", means)
    kw = merged_raster_kw("probe_pixels", raster_kw)
    x = field_rows(features, "features")[0]  # float16 / bfloat16 fields are read as stored: no float32 copy
    if x.shape[0] != means.shape[0]:
        raise GwbpError(f"{x.shape[0]} feature rows for {means.shape[0]} Gaussians")
    if x.shape[1] > MAX_D:
        raise GwbpError(f"D must be in [1, {MAX_D}], got {x.shape[1]}")
    xy = torch.as_tensor(xy, device=means.device).reshape(-1, 2).to(torch.int32)
    if not 1 <= xy.shape[0] <= MAX_PROBES:
        raise GwbpError(f"the number of probed pixels must be in [1, {MAX_PROBES}], got {xy.shape[0]}")
    eng, view, _ = front("probe_pixels", means, quats, scales, opacities, viewmat, K, width, height, kw)
    feats, _, alpha = eng.probe_pixels(view, xy, x, want_depth=False)
    # the depths as rasterization() computes them for its "+D" channel (one torch expression), rendered as a one-channel table
    vm = viewmat.to(means.device)
    z = (means @ vm[:3, :3].T + vm[:3, 3])[:, 2:3].contiguous()
    depth = eng.probe_pixels(view, xy, z, want_depth=False, want_alpha=False)[0][:, 0]
    return feats, depth, alpha


# ---- the 2-D mask of a frame -----------------------------------------------------------------------------------------------------

def overlay(frame: torch.Tensor, mask2d: torch.Tensor) -> torch.Tensor:
    """segment.py:227-231: frame uint8 [H, W, 3] * (0.75 + 0.25 mask [255, 0, 0] + 0.25 (1 - mask)), clipped, truncated to uint8."""
    m = mask2d[..., None].to(torch.float32)
    red = torch.tensor([255.0, 0.0, 0.0], device=frame.device)
    return (frame.to(torch.float32) * (0.75 + 0.25 * m * red + (1.0 - m) * 0.25)).clamp_(0.0, 255.0).to(torch.uint8)


def render_prompt_mask(means, quats, scales, opacities, features, viewmats, K, width, height, prompts, n_pos, colors=None,
                       sh_degree=None, **raster_kw) -> Iterator[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
    """segment.py:199-232 per view: (mask2d bool [H, W], frame uint8 [H, W, 3] or None) for every row of viewmats [C, 4, 4] (K:
    [3, 3] or [C, 3, 3]).  mask2d is where the rendered feature's best positive prompt beats its best negative one, computed as one
    P-channel render of prompt_scores(features, prompts, normalize=False) (see the module docstring); a pixel nothing covers is
    False.  With colors ([N, 3], or SH coefficients [N, K, 3] with sh_degree) the frame is the colour render, clip(x 255) as uint8,
    under the reference's overlay; without, None.  n_pos < P: the 2-D mask has no threshold form in the reference."""
    from .rasterization import rasterization
    p = prompts.shape[0] if torch.is_tensor(prompts) and prompts.dim() == 2 else 0
    if not 1 <= int(n_pos) < p:
        raise GwbpError(f"render_prompt_mask needs positive and negative prompts: 1 <= n_pos < P (got n_pos = {n_pos}, P = {p})")
    table = prompt_scores(features, prompts, normalize=False)
    Ks = K if K.dim() == 3 else K[None].expand(viewmats.shape[0], 3, 3)
    raster_kw = dict(raster_kw)
    raster_kw.setdefault("want_meta", False)
    for v in range(viewmats.shape[0]):
        s = rasterization(means, quats, scales, opacities, table, viewmats[v:v + 1], Ks[v:v + 1], width, height, **raster_kw)[0][0]
        mask2d = mask_from_scores(s, int(n_pos))
        frame = None
        if colors is not None:
            rgb = rasterization(means, quats, scales, opacities, colors, viewmats[v:v + 1], Ks[v:v + 1], width, height,
                                sh_degree=sh_degree, **raster_kw)[0][0]
            frame = overlay((rgb * 255.0).clamp_(0.0, 255.0).to(torch.uint8), mask2d)
        yield mask2d, frame


# ---- clicks ----------------------------------------------------------------------------------------------------------------------

class ClickSession:
    """The prompt state of click_and_segment.py:208-321 without its window: positive prompts come from clicks (the rendered
    feature at the pixel, probe_pixels), negatives from clicks or from `negatives` [P0, D] given up front (the script's encoded
    "other" text).  positions keeps what the caller passes beside each vector (the script's 3-D marker positions), untouched.
    mask() scores the field against the bare vectors, normalize=False, as the script does."""

    def __init__(self, features: torch.Tensor, negatives: Optional[torch.Tensor] = None):
        if not torch.is_tensor(features) or features.dim() != 2:
            raise GwbpError("features must be a [N, D] tensor")
        self.features = features
        self.positives: List[torch.Tensor] = []
        self.negatives: List[torch.Tensor] = []
        self.positive_positions: list = []
        self.negative_positions: list = []
        if negatives is not None:
            for row in negatives.reshape(-1, features.shape[1]):
                self.add_negative(row)

    def _vec(self, vec) -> torch.Tensor:
        v = torch.as_tensor(vec).detach().reshape(-1).to(device=self.features.device, dtype=torch.float32)
        if v.shape[0] != self.features.shape[1]:
            raise GwbpError(f"a prompt vector has {v.shape[0]} entries, the field D = {self.features.shape[1]}")
        if len(self.positives) + len(self.negatives) >= MAX_P:
            raise GwbpError(f"a session holds at most {MAX_P} prompts")
        return v.clone()

    def add_positive(self, vec, position=None) -> int:
        self.positives.append(self._vec(vec))
        self.positive_positions.append(position)
        return len(self.positives) - 1

    def add_negative(self, vec, position=None) -> int:
        self.negatives.append(self._vec(vec))
        self.negative_positions.append(position)
        return len(self.negatives) - 1

    def remove_positive(self, i: int) -> None:
        del self.positives[i]
        del self.positive_positions[i]

    def remove_negative(self, i: int) -> None:
        del self.negatives[i]
        del self.negative_positions[i]

    def prompts(self) -> Tuple[Optional[torch.Tensor], int]:
        """([P, D] positives then negatives, n_pos); (None, 0) without a prompt."""
        rows = self.positives + self.negatives
        return (torch.stack(rows) if rows else None), len(self.positives)

    def mask(self, threshold: Optional[float] = None) -> Optional[torch.Tensor]:
        """None while there is no positive prompt (the script then shows the whole scene); otherwise
        prompt_mask(features, positives + negatives, n_pos, normalize=False).  Without negatives a threshold is needed."""
        if not self.positives:
            return None
        t, n_pos = self.prompts()
        return prompt_mask(self.features, t, n_pos, threshold=threshold, normalize=False)


# ---- the extracted and the deleted scene -----------------------------------------------------------------------------------------

def apply_mask3d(splats: Dict[str, torch.Tensor], mask: torch.Tensor):
    """(extracted, deleted): copies of the splats dict with every per-Gaussian tensor (the keys prune_by_gradients indexes) cut to
    mask / ~mask; everything else (cameras, the COLMAP project) is shared (segment.py:70-95)."""
    n = splats["means"].shape[0]
    if mask.dtype != torch.bool or mask.shape != (n,):
        raise GwbpError(f"mask must be bool [{n}], got {mask.dtype} {tuple(mask.shape)}")
    out = []
    for keep in (mask, ~mask):
        cut = dict(splats)
        for k in PER_GAUSSIAN:
            if k in cut:
                cut[k] = cut[k][keep.to(cut[k].device)]
        out.append(cut)
    return out[0], out[1]


def encode_prompts(prompts: torch.Tensor, encoder: torch.Tensor) -> torch.Tensor:
    """segment_compressed.py:73-74: prompts [P, D_in] @ encoder [D_in, D], each row renormalised to unit length."""
    if prompts.dim() != 2 or encoder.dim() != 2 or prompts.shape[1] != encoder.shape[0]:
        raise GwbpError(f"prompts {tuple(prompts.shape)} do not fit the encoder {tuple(encoder.shape)}")
    return torch.nn.functional.normalize(prompts.float() @ encoder.float().to(prompts.device), dim=1)


def save_prompts(path: str, prompts: torch.Tensor, n_pos: int) -> None:
    torch.save({"prompts": prompts.detach().cpu().float(), "n_pos": int(n_pos)}, path)


def load_prompts(path: str):
    """(prompts [P, D] float32 on the host, n_pos) of a {"prompts": [P, D], "n_pos": int} .pt file."""
    d = torch.load(path, map_location="cpu")
    if not isinstance(d, dict) or "prompts" not in d or "n_pos" not in d:
        raise GwbpError(f"{path}: expected a dict with 'prompts' [P, D] and 'n_pos'")
    t = torch.as_tensor(d["prompts"]).float()
    if t.dim() != 2 or not 1 <= int(d["n_pos"]) <= t.shape[0]:
        raise GwbpError(f"{path}: prompts {tuple(t.shape)} with n_pos = {d['n_pos']}")
    return t, int(d["n_pos"])


def checkpoint_layout(splats: Dict[str, torch.Tensor]) -> dict:
    """segment.py:243-258 (save_to_ckpt): the gsplat checkpoint dict of a splats dict."""
    names = (("means", "means"), ("quats", "rotation"), ("scales", "scaling"), ("opacities", "opacity"), ("sh0", "features_dc"),
             ("shN", "features_rest"))
    return {"splats": {new: splats[old].detach().cpu() for new, old in names if old in splats}}
