"""TEST SUPPORT: the contract of the photometric loss (csrc/ssim.hip, gsbp_amd.photometric) in plain torch, with the
dtype as a parameter: float64 is the truth, float32 the floor of the project's floor rule.

    loss = (1 - lam) sum w |x - y| / (D Wa) + lam (1 - sum w ssim / (D Wv))

Two forms of the gradient: `loss_of` with torch's autograd, and `stored_map_backward`, the kernels' route -- the three maps w dmu, w d1,
w d12 of the forward, blurred again, combined per pixel.  tests/test_image_loss_ref_cpu.py holds them against each other and against
finite differences.  The `mutant` switches break one thing each; the same test shows that the floor rule sees every one of them.

Every blur is separable, horizontal then vertical, its 11 taps added in ascending order from zero over an image that reads zero
outside -- the kernels' chain without the fusing of the multiply-add, which no torch dtype offers.
"""
import math

import numpy as np
import torch

WIN, HALO = 11, 5
C1 = float(np.float32(0.01 ** 2))  # the float32 constants of csrc/ssim_math.h, widened: truth and kernel use the same numbers
C2 = float(np.float32(0.03 ** 2))
MUTANTS = ("drop_2xb", "drop_mu2_d12", "unnormalised_window", "same_over_valid_count")


def window(dtype=torch.float64, mutant=None):
    """g[i] = exp(-(i - 5)^2 / (2 1.5^2)), normalised to sum 1 in float64, rounded to float32 once, widened to `dtype`."""
    i = np.arange(WIN, dtype=np.float64)
    g = np.exp(-(i - HALO) ** 2 / (2 * 1.5 ** 2))
    if mutant != "unnormalised_window":
        g = g / g.sum()
    return torch.from_numpy(g.astype(np.float32)).to(dtype)


def blur(v, g):
    """The zero-padded ("same") blur of v [H, W, D]."""
    H, W, _ = v.shape
    p = torch.nn.functional.pad(v, (0, 0, HALO, HALO))
    h = torch.zeros_like(v)
    for i in range(WIN):
        h = h + g[i] * p[:, i:i + W]
    p = torch.nn.functional.pad(h, (0, 0, 0, 0, HALO, HALO))
    m = torch.zeros_like(v)
    for j in range(WIN):
        m = m + g[j] * p[j:j + H]
    return m


def window_mask(H, W, padding, dtype=torch.float64, device="cpu"):
    """[H, W]: 1 where the pixel is the centre of a window of this padding."""
    m = torch.zeros(H, W, dtype=dtype, device=device)
    if padding == "same":
        m[:] = 1
    elif H >= WIN and W >= WIN:
        m[HALO:H - HALO, HALO:W - HALO] = 1
    return m


def crop(t, padding):
    return t if padding == "same" else t[HALO:t.shape[0] - HALO, HALO:t.shape[1] - HALO]


def pointwise(x, y, g):
    """ssim and its partials d mu1 (total, m2 and m4 fixed), d s1, d s12 at every pixel of the full image, csrc/ssim_math.h's order."""
    mu1, mu2 = blur(x, g), blur(y, g)
    s1 = blur(x * x, g) - mu1 * mu1
    s2 = blur(y * y, g) - mu2 * mu2
    s12 = blur(x * y, g) - mu1 * mu2
    A = (2 * mu1) * mu2 + C1
    B = 2 * s12 + C2
    Cn = (mu1 * mu1 + mu2 * mu2) + C1
    Dn = (s1 + s2) + C2
    ab, cd = A * B, Cn * Dn
    ssim = ab / cd
    d12 = (2 * A) / cd
    d1 = -ab / (cd * Dn)
    dmu = (((2 * mu2) * B) / cd - ((2 * mu1) * ab) / (Cn * cd) - (2 * mu1) * d1)
    return ssim, dmu, d1, d12, mu2


def ssim_map(x, y, padding="valid", dtype=torch.float64):
    x, y = x.to(dtype), y.to(dtype)
    return crop(pointwise(x, y, window(dtype).to(x.device))[0], padding)


def sums(x, y, padding="valid", weights=None, dtype=torch.float64, mutant=None):
    """The table's first five entries, as `dtype` tensors with history: sum w ssim, sum w |x - y|, sum w (x - y)^2, Wv, Wa."""
    H, W, _ = x.shape
    w = torch.ones(H, W, dtype=dtype, device=x.device) if weights is None else weights.to(dtype)
    wv = w * window_mask(H, W, padding, dtype, x.device)
    ssim = pointwise(x, y, window(dtype, mutant).to(x.device))[0]
    e = x - y
    Wv = wv.sum()
    if mutant == "same_over_valid_count" and padding == "same":
        Wv = (w * window_mask(H, W, "valid", dtype, x.device)).sum()
    return (wv[..., None] * ssim).sum(), (w[..., None] * e.abs()).sum(), (w[..., None] * e * e).sum(), Wv, w.sum()


def loss_of(x, y, lam=0.2, padding="valid", weights=None, dtype=torch.float64, mutant=None):
    """The loss as a differentiable `dtype` scalar of x (cast inside: d loss / d x arrives in x's dtype), on x's device."""
    x, y = x.to(dtype), y.to(dtype)
    D = x.shape[2]
    s_ssim, s_l1, _, Wv, Wa = sums(x, y, padding, weights, dtype, mutant)
    zero = torch.zeros((), dtype=dtype, device=x.device)
    l1 = s_l1 / (D * Wa) if float(Wa) != 0 else zero
    ss = 1 - s_ssim / (D * Wv) if float(Wv) != 0 else zero
    return (1 - lam) * l1 + lam * ss


def autograd_gradient(x, y, lam=0.2, padding="valid", weights=None, dtype=torch.float64):
    xr = x.detach().to(dtype).requires_grad_(True)
    loss = loss_of(xr, y, lam, padding, weights, dtype)
    return loss.detach(), torch.autograd.grad(loss, xr)[0]


def stored_map_backward(x, y, lam=0.2, padding="valid", weights=None, dtype=torch.float64, mutant=None):
    """(loss, d loss / d x) by the kernels' route: v_x = s_s [a + 2 x b + y c] + s_1 w sign(x - y), with a, b, c the zero-padded blurs of
    w dmu, w d1, w d12 (zero where the pixel is no window), s_s = -lam / (D Wv), s_1 = (1 - lam) / (D Wa)."""
    x, y = x.detach().to(dtype), y.detach().to(dtype)
    H, W, D = x.shape
    g = window(dtype, mutant)
    w = torch.ones(H, W, dtype=dtype) if weights is None else weights.to(dtype)
    wv = (w * window_mask(H, W, padding, dtype))[..., None]
    ssim, dmu_part, d1, d12, mu2 = pointwise(x, y, g)
    dmu = dmu_part if mutant == "drop_mu2_d12" else dmu_part - mu2 * d12
    a, b, c = blur(wv * dmu, g), blur(wv * d1, g), blur(wv * d12, g)
    Wv, Wa = wv.sum(), w.sum()
    if mutant == "same_over_valid_count" and padding == "same":
        Wv = (w * window_mask(H, W, "valid", dtype)).sum()
    s_s = -lam / (D * Wv) if float(Wv) != 0 else torch.zeros((), dtype=dtype)
    s_1 = (1 - lam) / (D * Wa) if float(Wa) != 0 else torch.zeros((), dtype=dtype)
    inner = a + y * c if mutant == "drop_2xb" else (a + (2 * x) * b) + y * c
    grad = s_s * inner + (s_1 * w)[..., None] * torch.sign(x - y)
    e = x - y
    l1 = (w[..., None] * e.abs()).sum() / (D * Wa) if float(Wa) != 0 else 0.0
    ss = 1 - (wv * ssim).sum() / (D * Wv) if float(Wv) != 0 else 0.0
    return (1 - lam) * l1 + lam * ss, grad


# ---- inputs and the floor rule ------------------------------------------------------------------------------------------------------
def smooth_pair(H, W, D, seed=0, noise=0.05, ties=0.1):
    """A smooth seeded image pair in [0, 1] (float32 [H, W, D]): low-frequency waves, the render = the target plus another wave and
    noise, clamped; a share `ties` of the elements set equal to the target.  Uniform random images put SSIM near 0 and hide
    scale errors; these have SSIM around 0.5 .. 0.9."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * H + 3 * W + D)
    yy = torch.arange(H, dtype=torch.float64)[:, None, None]
    xx = torch.arange(W, dtype=torch.float64)[None, :, None]
    ph = torch.rand(4, D, generator=gen, dtype=torch.float64) * 2 * math.pi
    fr = 0.05 + 0.25 * torch.rand(4, D, generator=gen, dtype=torch.float64)
    target = 0.5 + 0.25 * torch.sin(fr[0] * yy + ph[0]) * torch.cos(fr[1] * xx + ph[1]) + 0.15 * torch.sin(fr[2] * (xx + yy) + ph[2])
    render = target + 0.08 * torch.cos(fr[3] * (xx - yy) + ph[3]) + noise * torch.randn(H, W, D, generator=gen, dtype=torch.float64)
    target = (target + 0.5 * noise * torch.randn(H, W, D, generator=gen, dtype=torch.float64)).clamp(0, 1).float()
    render = render.clamp(0, 1).float()
    tie = torch.rand(H, W, D, generator=gen) < ties
    return torch.where(tie, target, render).contiguous(), target.contiguous()


def smooth_weights(H, W, seed=0):
    """A float32 confidence map in [0, 1] with a block of exact zeros."""
    gen = torch.Generator().manual_seed(77 + seed + H * W)
    w = torch.rand(H, W, generator=gen)
    w[: max(1, H // 4), : max(1, W // 3)] = 0
    return w


def figures(t):
    """(Frobenius norm, max-abs) of a tensor, as floats in float64."""
    t = t.double()
    return float(t.norm()), float(t.abs().max()) if t.numel() else 0.0


def floor_ratios(got, truth, floor32):
    """Per figure (Frobenius, max-abs): |got - truth| / max(|float32 restatement - truth|, 2^-24 x the figure of truth)."""
    err, flo, nrm = figures(got.double() - truth.double()), figures(floor32.double() - truth.double()), figures(truth)
    return tuple(e / max(f, 2.0 ** -24 * n, 1e-300) for e, f, n in zip(err, flo, nrm))
