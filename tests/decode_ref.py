"""numpy float64 reference of the decode-loss call (gwbp_decode_loss, gsbp_amd.decoded_field), written from its definition, the
literal loop it replaces on the oracle's render, and the seeded data of its tests.

    y = R C      e = y - M      g = w_p sign(e) (l1, sign(0) = 0)  |  w_p 2 e (l2),  w_p = s c_p
    loss = sum w_p |e|  |  sum w_p e^2      GR = g C^T      GC = R^T g
    a pixel whose map row holds a non-finite value: nothing in loss, GR, GC; a zero GR row; counted in n_bad

The scene is fidelity_ref's (70 x 45, N = 3000, 4 views).  A Gaussian is SENSITIVE when its latent gradient moves by more than TOL *
scale under a 2-ulp change of exp() (fidelity_ref's method): its pairs sit on the alpha >= 1/255 or T <= 1e-4 cuts.
"""
import functools

import numpy as np
import torch

import fidelity_ref as fid
from oracle import oracle as orc

TOL = fid.TOL
W, H, N, N_VIEWS = fid.W, fid.H, fid.N, fid.N_VIEWS
U = 2.0 ** -24

# ---- the fit test: maps rendered from a hidden rank-16 field ----------------------------------------------------------------------
FIT_RANK, FIT_DIM, FIT_STEPS, FIT_LR, FIT_SEED = 16, 32, 12, 0.05, 3
# The largest per-step relative difference between the literal loop's float32 and float64 loss histories (literal_fit), as measured
# on the CPU: 9.657e-08.  The GPU test allows 10 x what literal_fit gives where it runs between the fused and the literal loop on
# the device (the factor covers the different summation orders of fp32 hardware); tests/test_decode_loss_cpu.py checks that the
# figure stays of this size (another host's float32 matmul may round differently: within a factor 2).
FIT_F32_VS_F64 = 9.7e-8


def fit_margin():
    """10 x the largest per-step relative loss difference of the literal loop in float32 and float64, measured here."""
    h32, h64 = literal_fit(torch.float32), literal_fit(torch.float64)
    return 10.0 * max(abs(a - b) / b for a, b in zip(h32, h64))


def reference(R, C, M, loss="l1", scale=1.0, weights=None):
    """dict of float64 arrays for R [P, d], C [d, D], M [P, D] (any float type; non-finite rows are bad), weights [P] or None:
    loss, GR, GC, n_bad, bad, and what the rounding bounds are stated against: y, e, g (the gradient image), w (w_p, zero on bad
    rows), terms (the loss terms) and y_abs = |R| |C|."""
    R, C, M = np.asarray(R, np.float64), np.asarray(C, np.float64), np.asarray(M, np.float64)
    bad = ~np.isfinite(M).all(axis=1)
    w = np.full(R.shape[0], float(scale)) * (1.0 if weights is None else np.asarray(weights, np.float64))
    w = np.where(bad, 0.0, w)
    y = R @ C
    e = np.where(bad[:, None], 0.0, y - np.where(bad[:, None], 0.0, M))
    if loss == "l1":
        g, terms = w[:, None] * np.sign(e), w[:, None] * np.abs(e)
    else:
        g, terms = w[:, None] * 2.0 * e, w[:, None] * e * e
    return dict(loss=terms.sum(), terms=terms, GR=g @ C.T, GC=R.T @ g, n_bad=int(bad.sum()), bad=bad, y=y, e=e, g=g, w=w,
                y_abs=np.abs(R) @ np.abs(C))


def l1_map(y_ref, seed=0):
    """M = y_ref - delta with |delta| in [0.05, 1] * mean |y_ref| and random signs: in float64 no |e| = |delta| lies within
    0.05 * mean |y_ref| of zero, so no sign flips under fp32 rounding of y.  Returns (float32 M, the margin 0.05 mean |y_ref|);
    M is rounded to float32, which moves e by at most 2^-24 |M|."""
    rng = np.random.default_rng(seed)
    mean = float(np.abs(y_ref).mean())
    delta = rng.uniform(0.05, 1.0, y_ref.shape) * mean * rng.choice([-1.0, 1.0], y_ref.shape)
    return (y_ref - delta).astype(np.float32), 0.05 * mean


def kernel_inputs(P, d, D, seed=0, loss="l1"):
    """Seeded float32 (R [P, d], C [d, D], M [P, D]) of the kernel-alone tests; the l1 map comes from l1_map."""
    rng = np.random.default_rng(1000 * seed + 7 * d + D + P)
    R = rng.standard_normal((P, d)).astype(np.float32)
    C = rng.uniform(0.0, 1.0, (d, D)).astype(np.float32) - np.float32(0.3)
    y = R.astype(np.float64) @ C.astype(np.float64)
    if loss == "l1" and P > 0:
        M, _ = l1_map(y, seed)
    else:
        M = (y + rng.standard_normal((P, D))).astype(np.float32)
    return R, C, M


# ---- the literal loop on the oracle's render --------------------------------------------------------------------------------------
def scatter64(pr, image):
    """float64 [N, d]: sum over the pairs of w image[pix] -- the gradient of a render with respect to its table."""
    gid, pix, w, _ = pr
    out = np.zeros((N, image.shape[1]), np.float64)
    np.add.at(out, gid, w.astype(np.float64)[:, None] * image[pix])
    return out


def literal_view(pr, latents, conv, M, loss="l1"):
    """render -> @ conv -> mean loss -> gradients by hand, float64, from the pairs pr of one view: dict(loss, grad_latents,
    grad_conv, scale_latents).  scale_latents is the sum of the absolute values of ALL the terms of an entry, as fidelity_ref
    defines a scale: sum over the pairs of w sum_j |g[pix, j] conv[k, j]|.  (Not sum |w GR[pix]|: GR[pix, k] is itself a sum of D
    signed terms that may cancel to nearly nothing, and the fp32 rounding of that sum is relative to its terms, not to its value.)"""
    D = conv.shape[1]
    r = fid.render64(pr, latents)
    ref = reference(r, conv, np.asarray(M).reshape(H * W, D), loss, 1.0 / (H * W * D))
    gid, pix, w, _ = pr
    scale = np.zeros((N, latents.shape[1]), np.float64)
    np.add.at(scale, gid, np.abs(w.astype(np.float64))[:, None] * (np.abs(ref["g"]) @ np.abs(np.asarray(conv, np.float64)).T)[pix])
    return dict(loss=ref["loss"], grad_latents=scatter64(pr, ref["GR"]), grad_conv=ref["GC"], scale_latents=scale, render=r, GR=ref["GR"])


def sensitive_gaussians(view, latents, conv, M, loss="l1"):
    """(bool [N]: Gaussians whose latent gradient moves by more than TOL * scale under a 2-ulp exp(), bool [N]: Gaussians with a
    non-zero gradient)."""
    base = literal_view(fid.pairs(view), latents, conv, M, loss)
    out = np.zeros(N, bool)
    try:
        for ulp in (2, -2):
            orc.set_tunables(exp_ulp=ulp)
            moved = literal_view(fid._pairs(view), latents, conv, M, loss)
            out |= (np.abs(moved["grad_latents"] - base["grad_latents"]) > TOL * np.maximum(base["scale_latents"], 1e-30)).any(axis=1)
    finally:
        orc.set_tunables()
    return out, (base["grad_latents"] != 0).any(axis=1)


@functools.lru_cache(maxsize=None)
def view_case(d=32, D=48, seed=11):
    """Seeded float32 (latents [N, d], conv [d, D], l1 map of view 0 [H, W, D]) for the tests through rasterization()."""
    rng = np.random.default_rng(seed)
    latents = rng.standard_normal((N, d)).astype(np.float32)
    conv = rng.uniform(0.0, 1.0, (d, D)).astype(np.float32)
    y = fid.render64(fid.pairs(0), latents) @ conv.astype(np.float64)
    M, margin = l1_map(y, seed)
    return latents, conv, M.reshape(H, W, D), margin


# ---- the literal fit loop on the CPU -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_maps():
    """float32 [H, W, FIT_DIM] maps of the four views: the renders of hidden_latents [N, 16] @ hidden_decoder [16, FIT_DIM]."""
    rng = np.random.default_rng(FIT_SEED)
    hidden = rng.standard_normal((N, FIT_RANK)) @ (rng.standard_normal((FIT_RANK, FIT_DIM)) / 4.0)
    return tuple(fid.render64(fid.pairs(v), hidden).reshape(H, W, FIT_DIM).astype(np.float32) for v in range(N_VIEWS))


def fit_init(seed=0):
    """The generator state fit_decoded_field starts from: (decoder0 [16, FIT_DIM] float32, the views of the 12 steps)."""
    gen = torch.Generator().manual_seed(seed)
    decoder = torch.rand(FIT_RANK, FIT_DIM, generator=gen)
    order = []
    while len(order) < FIT_STEPS:
        order += torch.randperm(N_VIEWS, generator=gen).tolist()
    return decoder, order[:FIT_STEPS]


@functools.lru_cache(maxsize=None)
def literal_fit(dtype, seed=0):
    """The loss history of the literal loop on the CPU in `dtype`: render (the oracle's pairs as a sparse matrix) @ conv,
    F.mse_loss, torch.optim.Adam on both tensors, the views in fit_decoded_field's order."""
    decoder0, order = fit_init(seed)
    mats = []
    for v in range(N_VIEWS):
        gid, pix, w, _ = fid.pairs(v)
        idx = torch.from_numpy(np.stack([pix.astype(np.int64), gid.astype(np.int64)]))
        mats.append(torch.sparse_coo_tensor(idx, torch.from_numpy(w.astype(np.float32)).to(dtype), (H * W, N)).coalesce())
    maps = [torch.from_numpy(m).to(dtype).reshape(H * W, FIT_DIM) for m in fit_maps()]
    latents = torch.zeros(N, FIT_RANK, dtype=dtype, requires_grad=True)
    decoder = decoder0.to(dtype).requires_grad_(True)
    opt = torch.optim.Adam([latents, decoder], lr=FIT_LR)
    history = []
    for v in order:
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(torch.sparse.mm(mats[v], latents) @ decoder, maps[v])
        loss.backward()
        opt.step()
        history.append(float(loss.detach()))
    return tuple(history)
