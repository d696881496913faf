"""The yardstick of the SH colours' gradient to the camera centre (csrc/sh.hip's k_sh_eval_bwd_dev).

Truth is gsbp_amd.projection.sh_colors_torch under autograd in float64 on the CPU with `campos` a leaf beside the means and the
coefficients; the same in float32 is the noise floor.  The kernel's v_campos [3] is held against the truth by the project's floor rule,
per figure (Frobenius norm, max-abs) of the three numbers:

    figure(kernel - truth) <= FACTOR x max(figure(float32 CPU autograd - truth), 2^-24 x figure(truth))

The inputs are sh_grad_ref.make_case's, with one change: that case puts row 0 exactly at the camera centre, where v_means is about 1e11
and would be all there is to see in a sum over the rows.  Here row 0 is moved one unit away from the centre, and the promise about the
clamp's edge is restored for it the way make_case does.  (The row at the centre stays in the bit comparisons against the existing
kernels, which run on make_case's own case.)
"""
import numpy as np
import torch

import sh_grad_ref as ref
from gsbp_amd.projection import sh_colors_torch

FIGURES = ref.FIGURES


def make_case(n, degree, k, seed=0):
    case = ref.make_case(n, degree, k, seed=seed)
    r = np.random.default_rng(77 + 1000 * seed + 16 * degree + k)
    d = r.normal(size=3)
    case["means"][0] = ref.f32(case["campos"] + d / np.linalg.norm(d))
    for _ in range(8):
        pre = ref.preclamp64(degree, case["means"][:1], case["coeffs"][:1], case["campos"].tolist())
        close = np.abs(pre) < 4 * ref.EDGE
        if not close.any():
            break
        case["coeffs"][:1, 0][close] += np.float32(0.01 / ref.C0)
    return case


def autograd(case, dtype):
    """dict(colors, v_coeffs, v_means, v_campos) of sh_colors_torch under autograd in `dtype` on the CPU, as float64 numpy."""
    m = torch.from_numpy(case["means"]).to(dtype).requires_grad_(True)
    c = torch.from_numpy(case["coeffs"]).to(dtype).requires_grad_(True)
    cp = torch.from_numpy(case["campos"]).to(dtype).requires_grad_(True)
    out = sh_colors_torch(case["degree"], m, c, cp)
    gc, gm, gp = torch.autograd.grad(out, (c, m, cp), torch.from_numpy(case["v_colors"]).to(dtype), allow_unused=True)
    gm = torch.zeros_like(m) if gm is None else gm
    gp = torch.zeros_like(cp) if gp is None else gp
    return {k: t.detach().double().numpy() for k, t in (("colors", out), ("v_coeffs", gc), ("v_means", gm), ("v_campos", gp))}


def campos_ratios(got, truth, floor):
    """{figure: figure(got - truth) / max(figure(floor - truth), 2^-24 figure(truth))} of v_campos; a truth of all zeros admits
    nothing: the ratio is 0 where got is all zeros too and inf otherwise."""
    g, t, f = (np.asarray(v, np.float64) for v in (got, truth, floor))
    eg, ef, ft = ref.figures(g - t), ref.figures(f - t), ref.figures(t)
    out = {}
    for fig in FIGURES:
        bound = max(ef[fig], 2.0 ** -24 * ft[fig])
        out[fig] = 0.0 if eg[fig] == 0.0 else (eg[fig] / bound if bound > 0.0 else float("inf"))
    return out
