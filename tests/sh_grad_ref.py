"""The yardstick of the SH colours' backward (csrc/sh_math.h, csrc/sh.hip).

Truth is gsbp_amd.projection.sh_colors_torch under autograd in float64 on the CPU; the same in float32 is the noise floor.  A result is
held against the truth by the project's floor rule, per tensor and figure (Frobenius norm, max-abs):

    figure(got - truth) <= FACTOR x max(figure(float32 restatement - truth), 2^-24 x figure(truth))

`restate` is the backward's arithmetic in numpy float32, written as sh_math.h writes it, with the mutants a comparison must catch.

The inputs (make_case): seeded; every |mean - campos| >= 0.5 except row 0, which sits exactly at the camera centre and is checked on its
own and kept out of the norms (its v_means is about 1e11); the coefficients are scaled so that at least 20 % of the rows clamp in some
channel, and no pre-clamp value of the truth lies within 1e-4 of 0: the mask at the edge depends on the precision ((0 - 0.5) / C0 * C0 +
0.5 is just below 0 in float32 and exactly 0 in float64).
"""
import numpy as np
import torch

from gsbp_amd.projection import sh_colors_torch

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
C3 = (0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 1.445305721320277)
CAMPOS = (0.25, -0.5, 3.0)
EDGE = 1e-4
FIGURES = ("fro", "max")
TENSORS = ("colors", "v_coeffs", "v_means")


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def preclamp64(degree, means, coeffs, campos):
    """rgb + 0.5 of sh_colors_torch in float64, before the clamp: [N, 3]."""
    big = 1024.0  # the clamp hides what lies below 0: the DC term lifts every value above it by `big` (exactly representable) first
    with torch.no_grad():
        m, c = torch.from_numpy(means).double(), torch.from_numpy(coeffs).double()
        up = sh_colors_torch(degree, m, torch.cat([c[:, :1] + big / C0, c[:, 1:]], dim=1), campos) - big
    return up.numpy()


def make_case(n, degree, k, seed=0, scale=1.2):
    """dict(means, coeffs [n, k, 3], campos, v_colors, degree) in float32 numpy, by the rules of the module's docstring."""
    r = np.random.default_rng(1000 * seed + 16 * degree + k)
    campos = f32(CAMPOS)
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    means = f32(campos + d * r.uniform(0.6, 4.0, size=(n, 1)))
    means[0] = campos
    coeffs = f32(scale * r.normal(size=(n, k, 3)))
    coeffs[:, 0] -= np.float32(0.3 / C0)  # the DC term around 0.2: a good share of the channels below 0
    v_colors = f32(r.normal(size=(n, 3)))
    for _ in range(8):  # push what lies at the clamp's edge away from it, through the DC coefficient
        pre = preclamp64(degree, means, coeffs, campos.tolist())
        close = np.abs(pre) < 4 * EDGE
        if not close.any():
            break
        coeffs[:, 0][close] += np.float32(0.01 / C0)
    return dict(means=means, coeffs=coeffs, campos=campos, v_colors=v_colors, degree=degree)


def case_facts(case):
    """(the share of rows that clamp in some channel, the smallest |pre-clamp value|) of the float64 truth, row 0 included."""
    pre = preclamp64(case["degree"], case["means"], case["coeffs"], case["campos"].tolist())
    return float((pre < 0).any(axis=1).mean()), float(np.abs(pre).min())


def autograd(case, dtype, device="cpu", fn=sh_colors_torch):
    """dict(colors, v_coeffs, v_means) of fn(degree, means, coeffs, campos) under autograd in `dtype`, as float64 numpy."""
    m = torch.from_numpy(case["means"]).to(device, dtype).requires_grad_(True)
    c = torch.from_numpy(case["coeffs"]).to(device, dtype).requires_grad_(True)
    out = fn(case["degree"], m, c, case["campos"].tolist())
    gc, gm = torch.autograd.grad(out, (c, m), torch.from_numpy(case["v_colors"]).to(device, dtype), allow_unused=True)
    gm = torch.zeros_like(m) if gm is None else gm
    return {k: t.detach().cpu().double().numpy() for k, t in (("colors", out), ("v_coeffs", gc), ("v_means", gm))}


def basis_and_derivatives(degree, x, y, z, mutant=None):
    """b [nb] and (db/dx, db/dy, db/dz), each a list of float32 arrays, in sh_math.h's expressions."""
    one, zero = np.ones_like(x), np.zeros_like(x)
    F = np.float32
    b, dx, dy, dz = [F(C0) * one], [zero], [zero], [zero]
    if degree >= 1:
        b += [F(-C1) * y, F(C1) * z, F(-C1) * x]
        dx += [zero, zero, F(-C1) * one]
        dy += [F(-C1) * one, zero, zero]
        dz += [zero, F(C1) * one, zero]
    if degree >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [F(C2[0]) * xy, F(-C2[0]) * yz, F(C2[1]) * (F(2) * zz - xx - yy), F(-C2[0]) * xz, F(C2[2]) * (xx - yy)]
        dx += [F(C2[0]) * y, zero, F(-2) * F(C2[1]) * x, F(-C2[0]) * z, F(2) * F(C2[2]) * x]
        dy += [F(C2[0]) * x, F(-C2[0]) * z, F(-2) * F(C2[1]) * y, zero, F(-2) * F(C2[2]) * y]
        dz += [zero, F(-C2[0]) * y, F(4) * F(C2[1]) * z, F(-C2[0]) * x, zero]
    if degree >= 3:
        s = F(-1.0 if mutant == "sign_deg3" else 1.0)
        b += [F(-C3[0]) * y * (F(3) * xx - yy), F(C3[1]) * xy * z, F(-C3[2]) * y * (F(4) * zz - xx - yy),
              F(C3[3]) * z * (F(2) * zz - F(3) * xx - F(3) * yy), F(-C3[2]) * x * (F(4) * zz - xx - yy), F(C3[4]) * z * (xx - yy),
              F(-C3[0]) * x * (xx - F(3) * yy)]
        dx += [F(-6) * F(C3[0]) * xy, F(C3[1]) * yz, F(2) * F(C3[2]) * xy, F(-6) * F(C3[3]) * xz, F(-C3[2]) * (F(4) * zz - F(3) * xx - yy),
               F(2) * F(C3[4]) * xz, F(-3) * F(C3[0]) * (xx - yy)]
        dy += [F(-3) * F(C3[0]) * (xx - yy), F(C3[1]) * xz, F(-C3[2]) * (F(4) * zz - xx - F(3) * yy), F(-6) * F(C3[3]) * yz,
               F(2) * F(C3[2]) * xy, F(-2) * F(C3[4]) * yz, F(6) * F(C3[0]) * xy]
        dz += [zero, F(C3[1]) * xy, s * F(-8) * F(C3[2]) * yz, F(3) * F(C3[3]) * (F(2) * zz - xx - yy), F(-8) * F(C3[2]) * xz,
               F(C3[4]) * (xx - yy), zero]
    return b, dx, dy, dz


def restate(case, mutant=None):
    """sh_math.h's forward and backward in numpy float32 (sums in its order; the fmaf chains as multiply-adds rounded twice, which is
    inside the floor).  mutant: None | "sign_deg3" | "no_projection" | "no_mask" | "no_zero_rows"."""
    F = np.float32
    degree, means, coeffs, v = case["degree"], case["means"], case["coeffs"], case["v_colors"]
    nb, k_total = (degree + 1) ** 2, coeffs.shape[1]
    with np.errstate(all="ignore"):
        d = means - case["campos"][None, :]
        n = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], dtype=F)
        inv = F(1) / np.maximum(n, F(1e-12))
        x, y, z = d[:, 0] * inv, d[:, 1] * inv, d[:, 2] * inv
        b, dx, dy, dz = basis_and_derivatives(degree, x, y, z, mutant)
        rgb = np.zeros((len(means), 3), F)
        for k in range(nb):
            rgb = b[k][:, None] * coeffs[:, k] + rgb
        colors = np.maximum(rgb + F(0.5), F(0))
        passes = (rgb + F(0.5) >= 0) if mutant != "no_mask" else np.ones_like(rgb, dtype=bool)
        vm = np.where(passes, v, F(0))
        v_coeffs = np.zeros_like(coeffs) if mutant != "no_zero_rows" else coeffs.copy()
        vd = np.zeros((len(means), 3), F)
        for k in range(nb):
            v_coeffs[:, k] = b[k][:, None] * vm
            t = (coeffs[:, k, 0] * vm[:, 0] + coeffs[:, k, 1] * vm[:, 1]) + coeffs[:, k, 2] * vm[:, 2]
            vd[:, 0] += t * dx[k]
            vd[:, 1] += t * dy[k]
            vd[:, 2] += t * dz[k]
        dirs = np.stack([x, y, z], axis=1)
        dot = (x * vd[:, 0] + y * vd[:, 1]) + z * vd[:, 2]
        clamped = ~(n > F(1e-12))
        proj = vd if mutant == "no_projection" else vd - dirs * dot[:, None]
        v_means = np.where(clamped[:, None], vd * inv[:, None], proj * inv[:, None]).astype(F)
        if degree == 0:
            v_means = np.zeros_like(v_means)
    return dict(colors=colors.astype(np.float64), v_coeffs=v_coeffs.astype(np.float64), v_means=v_means.astype(np.float64))


def figures(a):
    a = np.asarray(a, np.float64)
    return dict(fro=float(np.linalg.norm(a)), max=float(np.abs(a).max()) if a.size else 0.0)


def ratios(got, truth, floor, skip_row0=True):
    """{(tensor, figure): figure(got - truth) / max(figure(floor - truth), 2^-24 figure(truth))}; a truth of all zeros admits nothing:
    the ratio is 0 where got is all zeros too and inf otherwise.  Row 0 (the camera centre) is left out."""
    s = slice(1, None) if skip_row0 else slice(None)
    out = {}
    for name in TENSORS:
        g, t, f = (np.asarray(v[name], np.float64)[s] for v in (got, truth, floor))
        eg, ef, ft = figures(g - t), figures(f - t), figures(t)
        for fig in FIGURES:
            bound = max(ef[fig], 2.0 ** -24 * ft[fig])
            out[(name, fig)] = 0.0 if eg[fig] == 0.0 else (eg[fig] / bound if bound > 0.0 else float("inf"))
    return out


def check_row0(case, got):
    """The Gaussian at the camera centre: its colour is the DC term's, and its v_means is v_dir 1e12 (relative 1e-5), v_dir from the
    degree-1 rows alone (every higher derivative vanishes at dir = 0)."""
    c0 = case["coeffs"][0].astype(np.float64)
    pre = C0 * c0[0] + 0.5
    assert np.allclose(got["colors"][0], np.maximum(pre, 0.0), rtol=1e-6, atol=1e-7)
    if case["degree"] == 0:
        assert not np.asarray(got["v_means"][0]).any()
        return
    v = np.where(pre >= 0, case["v_colors"][0].astype(np.float64), 0.0)
    t = c0 @ v
    want = np.array([-C1 * t[3], -C1 * t[1], C1 * t[2]]) * 1e12
    assert np.isfinite(got["v_means"][0]).all()
    assert np.abs(got["v_means"][0] - want).max() <= 1e-5 * np.abs(want).max(), (got["v_means"][0], want)
