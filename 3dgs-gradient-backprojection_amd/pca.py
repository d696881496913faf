"""PCA of a finished feature field and its two pictures (the reference's visualize_pca.py: sklearn PCA(3) on a host copy of the
field, then "PCA on Gaussians" or "PCA on renderings"), without the host copy, the CPU fit or the [H, W, D] render.

    basis = fit_pca(features)                         # sklearn.decomposition.PCA(3).fit(features)
    Y = pca_transform(features, basis)                # pca.transform(features)
    colors, lo, hi = pca_colors(features, basis)      # (Y - Y.min()) / (Y.max() - Y.min())
    for frame in render_pca(means, quats, scales, opacities, features, viewmats, K, W, H, mode="renderings", scale=1.0): ...

The [N, D] passes run in csrc/pca.hip on the caller's current stream: column means, the CENTRED Gram matrix on the fp32 matrix
cores (x - mean while a row chunk is staged; no second [N, D] tensor), the projection with its min / max.  The D x D part is
sklearn's covariance_eigh solver: float64 eigh of G / (N - 1) on the host, eigenvalues descending, each component's entry of
largest magnitude made positive.  There is no PyTorch fallback: CPU tensors raise, and so does a missing library.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Iterator, Optional

import torch

from ._lib import GwbpError, check, lib, ptr
from ._views import FIELD_TYPES, field_rows, ld, rows, run  # noqa: F401

MAX_K = 16            # GWBP_PCA_MAX_K
MAX_D = 2048          # GWBP_PCA_MAX_D
PROJECT_ROWS = 128    # GWBP_PCA_PROJECT_ROWS


@dataclass
class PCABasis:
    """mean [D] and components [k, D]: float32 on the field's device (what the projection kernel reads);
    explained_variance [k] and explained_variance_ratio [k]: float64 on the host, as sklearn's attributes of those names."""
    mean: torch.Tensor
    components: torch.Tensor
    explained_variance: torch.Tensor
    explained_variance_ratio: torch.Tensor
    n_samples: int

    def state_dict(self) -> dict:
        return {"mean": self.mean.cpu(), "components": self.components.cpu(), "explained_variance": self.explained_variance,
                "explained_variance_ratio": self.explained_variance_ratio, "n_samples": self.n_samples}

    @classmethod
    def from_state_dict(cls, d: dict, device=None) -> "PCABasis":
        return cls(d["mean"].to(device), d["components"].to(device), d["explained_variance"], d["explained_variance_ratio"],
                   int(d["n_samples"]))


# ---- host logic ------------------------------------------------------------------------------------------------------------------

def _check_sizes(features, n_components: Optional[int], min_rows: int) -> None:
    if not torch.is_tensor(features) or features.dim() != 2:
        raise GwbpError("features must be a [N, D] tensor")
    n, d = features.shape
    if n < min_rows:
        raise GwbpError(f"features need at least {min_rows} rows, got N = {n}")
    if not 1 <= d <= MAX_D:
        raise GwbpError(f"D must be in [1, {MAX_D}], got {d}")
    if n_components is not None:
        k = int(n_components)
        if not 1 <= k <= MAX_K:
            raise GwbpError(f"n_components must be in [1, {MAX_K}], got {k}")
        if k > d:
            raise GwbpError(f"n_components = {k} exceeds D = {d}")


def _eig_basis(cov: torch.Tensor, k: int):
    """The D x D half of sklearn's covariance_eigh solver on a float64 covariance matrix: (components [k, D], variances [k],
    ratios [k]), eigenvalues descending and clipped at 0, each component's first entry of largest magnitude made positive
    (svd_flip on the components).  A covariance without spread has ratio 0, not 0 / 0.  A non-finite entry raises, as sklearn does
    on NaN input."""
    if not bool(torch.isfinite(cov).all()):
        raise GwbpError("the features hold NaN or infinite entries (their covariance is not finite)")
    w, v = torch.linalg.eigh(cov.to(torch.float64).cpu())
    w, v = w.flip(0).clamp_min(0.0), v.flip(1)
    comps = v[:, :k].T.contiguous()
    lead = comps.gather(1, comps.abs().argmax(dim=1, keepdim=True))
    comps = comps * torch.where(lead < 0, -1.0, 1.0).to(comps.dtype)
    total = w.sum()
    ratio = w[:k] / total if float(total) > 0.0 else torch.zeros(k, dtype=torch.float64)
    return comps, w[:k].clone(), ratio


# ---- the [N, D] passes -----------------------------------------------------------------------------------------------------------

def _covariance(features: torch.Tensor):
    """(mean [D] float32, covariance [D, D] float64, both on the device) of the rows: gwbp_column_means + gwbp_centered_gram,
    the Gram over N - 1."""
    _check_sizes(features, None, 2)
    x, ft = field_rows(features, "features")
    n, d = x.shape
    need = C.c_size_t(0)
    check(lib().gwbp_pca_workspace_size(n, d, C.byref(need)), "gwbp_pca_workspace_size")
    ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device=x.device)
    mean = torch.empty(d, dtype=torch.float32, device=x.device)
    gram = torch.empty(d, d, dtype=torch.float64, device=x.device)
    run("gwbp_column_means_typed", x.device, C.c_int64(n), d, ptr(x), ft, C.c_int64(ld(x)), ptr(mean), ptr(ws), ws.numel())
    run("gwbp_centered_gram_typed", x.device, C.c_int64(n), d, ptr(x), ft, C.c_int64(ld(x)), ptr(mean), ptr(gram), ptr(ws), ws.numel())
    return mean, gram / float(n - 1)


def _project(x: torch.Tensor, mean: torch.Tensor, components: torch.Tensor):
    """(Y [N, k], minmax [ceil(N / 128), 2]) of gwbp_pca_project on checked rows (field_rows: in their own dtype)."""
    n, d = x.shape
    k = components.shape[0]
    if components.shape != (k, d) or mean.shape != (d,) or not 1 <= k <= MAX_K:
        raise GwbpError(f"the basis (mean {tuple(mean.shape)}, components {tuple(components.shape)}) does not fit D = {d}")
    mean = mean.to(device=x.device, dtype=torch.float32).contiguous()
    components = components.to(device=x.device, dtype=torch.float32).contiguous()
    y = torch.empty(n, k, dtype=torch.float32, device=x.device)
    mm = torch.empty(-(-n // PROJECT_ROWS), 2, dtype=torch.float32, device=x.device)
    run("gwbp_pca_project_typed", x.device, C.c_int64(n), d, k, ptr(x), FIELD_TYPES[x.dtype], C.c_int64(ld(x)), ptr(mean), ptr(components),
        ptr(y), ptr(mm))
    return y, mm


def fit_pca(features: torch.Tensor, n_components: int = 3) -> PCABasis:
    """sklearn.decomposition.PCA(n_components).fit(features) on a [N, D] device tensor, N >= 2, D <= 2048, n_components <=
    min(16, D).  features may have any row stride >= D and are read in place (float16 / bfloat16 as stored: widened exactly in the
    kernels, so the fit has the bits of the fit of features.float() without that copy; a tensor without unit stride inside a row is
    copied with .contiguous()).  Two fits of one tensor are bit-equal.  NaN or infinite
    entries raise GwbpError.  A field without spread (all rows equal) gives variance 0, ratio 0 and unit-vector components."""
    _check_sizes(features, n_components, 2)
    mean, cov = _covariance(features)
    comps, var, ratio = _eig_basis(cov, int(n_components))
    return PCABasis(mean, comps.to(torch.float32).to(mean.device), var, ratio, int(features.shape[0]))


def pca_transform(features: torch.Tensor, basis: PCABasis) -> torch.Tensor:
    """pca.transform(features): Y [N, k] = (features - mean) @ components.T in one pass over the rows (exact fp32)."""
    _check_sizes(features, None, 1)
    return _project(field_rows(features, "features")[0], basis.mean, basis.components)[0]


def pca_colors(features: torch.Tensor, basis: Optional[PCABasis] = None):
    """visualize_pca.py:40-52: (colors [N, 3] in [0, 1], lo, hi) with colors = (Y - lo) / (hi - lo), Y = pca_transform(features),
    and ONE lo = Y.min() and hi = Y.max() over all three channels (the reference's np.min(..., axis=(0, 1))), both 0-d device
    tensors, bit-equal to torch's.  basis None fits PCA(3) on the features.  A field without spread is 0.5 everywhere."""
    if basis is None:
        basis = fit_pca(features, 3)
    _check_sizes(features, None, 1)
    y, mm = _project(field_rows(features, "features")[0], basis.mean, basis.components)
    lo_hi = torch.stack([mm[:, 0].min(), mm[:, 1].max()])
    colors = torch.empty_like(y)
    run("gwbp_pca_colors", y.device, C.c_int64(y.numel()), ptr(y), ptr(lo_hi), ptr(colors))
    return colors, lo_hi[0], lo_hi[1]


# ---- the two pictures ------------------------------------------------------------------------------------------------------------

def _to_uint8(mode: str, values: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    """A float frame of _pca_frames as uint8 [H, W, 3].  gaussians: utils.torch_to_cv without its channel flip, clamp(0, 1) * 255
    truncated.  renderings: visualize_pca.py:100-108, (values - lo) / (hi - lo) * 255 truncated; values outside [lo, hi] (pixels the
    Gaussians do not cover fully) saturate at 0 / 255 where numpy's cast of the reference wraps."""
    if mode == "gaussians":
        return (values.clamp(0.0, 1.0) * 255.0).to(torch.uint8)
    span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
    return (values - lo).div_(span).mul_(255.0).clamp_(0.0, 255.0).to(torch.uint8)  # (one [H, W, 3] temporary)


def _pca_frames(means, quats, scales, opacities, features, viewmats, K, width, height, mode, basis, scale, raster_kw):
    """(basis, lo, hi, iterator over the float frames [H, W, 3]): gaussians -- the rendered colours; renderings -- pca.transform of
    the rendered features, by linearity render(F V^T) - mean V^T: a 3-channel render, never an [H, W, D] one."""
    from .rasterization import rasterization
    if mode not in ("gaussians", "renderings"):
        raise ValueError(f"mode must be 'gaussians' or 'renderings', got {mode!r}")
    if basis is None:
        basis = fit_pca(features, 3)
    if basis.components.shape[0] != 3:
        raise GwbpError(f"a picture needs 3 components, the basis has {basis.components.shape[0]}")
    colors, lo, hi = pca_colors(features, basis)
    offset = None
    if mode == "renderings":
        x = field_rows(features, "features")[0]
        colors = _project(x, torch.zeros_like(basis.mean), basis.components)[0]
        offset = (basis.components.double() @ basis.mean.double()).float().to(x.device)
    Ks = K if K.dim() == 3 else K[None].expand(viewmats.shape[0], 3, 3)
    scaled = scales * scale
    raster_kw = dict(raster_kw)
    raster_kw.setdefault("want_meta", False)

    def frames():
        for v in range(viewmats.shape[0]):
            out = rasterization(means, quats, scaled, opacities, colors, viewmats[v:v + 1], Ks[v:v + 1], width, height,
                                **raster_kw)[0][0]
            yield out if offset is None else out - offset
    return basis, lo, hi, frames()


def render_pca(means, quats, scales, opacities, features, viewmats, K, width, height, mode: str = "gaussians",
               basis: Optional[PCABasis] = None, scale: float = 1.0, **raster_kw) -> Iterator[torch.Tensor]:
    """The frames of visualize_pca.py, one uint8 [H, W, 3] device tensor per row of viewmats [C, 4, 4] (K: [3, 3] or [C, 3, 3]).

    mode "gaussians" (the reference's "PCA on Gaussians", which passes scale=0.2): rasterization(colors=pca_colors(features),
    scales * scale), clamp(0, 1) * 255 truncated.  mode "renderings" ("PCA on renderings"): pca.transform of the rendered
    features, normalised with the field's lo and hi, * 255, truncated -- computed as rasterization(features @ components.T) -
    mean @ components.T, which is the same by linearity.  Channel order: channel j is component j (R = the first); the reference
    flips to BGR only for cv2.  basis None fits PCA(3) on the features.  raster_kw (camera_model, rasterize_mode, near_plane, ...)
    goes to rasterization()."""
    _, lo, hi, frames = _pca_frames(means, quats, scales, opacities, features, viewmats, K, width, height, mode, basis, scale,
                                    raster_kw)
    for values in frames:
        yield _to_uint8(mode, values, lo, hi)
