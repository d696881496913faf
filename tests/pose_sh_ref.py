"""The yardstick of render_splats(pose_grad=True): the dense restatement of tests/raster_grad_ref.py with the view matrix as a sixth
leaf, as in tests/camera_grad_ref.py, and the SH colours' camera centre -(R^T t) a FUNCTION of that leaf, so that the view matrix's
gradient holds the colours' share (through the view directions) beside the projection's.

`attached=False` detaches the centre: the gradient a trainer would get from rasterization(camera_grad=True) beside colours whose centre
was read on the host.  A comparison that cannot tell the two apart proves nothing about the link, so the case's coefficients are chosen
(SH_SCALE, verified on the CPU by tests/test_gpu_pose_grad.py's own assertion and by running this file) such that the detached gradient
lies far outside the FACTOR x floor rule.
"""
import torch

import camera_grad_ref as cg
import raster_grad_ref as rg

NAMES = cg.NAMES
SH_DEGREE = 2
# test_gpu_raster_grad._t0(sh=True) draws the coefficients as 0.4 randn; they are used as drawn.  Measured with fixed_cut on the CPU
# (python tests/pose_sh_ref.py): the detached centre puts the view matrix's gradient 4.4e-2 (Frobenius-relative; 5.0e-2 max-abs) from the
# truth, the float32 floor is 6.4e-7 (5.9e-7): four orders of magnitude outside FACTOR = 4.
SH_SCALE = 1.0


def case_of(t0_case):
    """test_gpu_raster_grad._t0(sh=True) with its coefficients scaled by SH_SCALE, at SH_DEGREE."""
    ins = t0_case["inputs"]
    return dict(t0_case, inputs=ins[:4] + (SH_SCALE * ins[4],), sh_degree=SH_DEGREE)


def gradients(dtype, inputs, G, A, viewmat, K, W, H, cut, sh_degree=SH_DEGREE, attached=True, **kw):
    """The six gradients (NAMES' order; the last one [4, 4], its bottom row zero) of sum(out G) + sum(alpha_img A) in `dtype`; inputs[4]
    holds the [N, K, 3] SH coefficients."""
    ins = [t.detach().cpu().to(dtype).requires_grad_(True) for t in inputs]
    vm = viewmat.detach().cpu().to(dtype).requires_grad_(True)
    campos = -(vm[:3, :3].T @ vm[:3, 3])
    out, alpha, _ = rg.rasterize(*ins, vm, K.cpu(), W, H, cut, sh_degree=sh_degree, campos=campos if attached else campos.detach(), **kw)
    loss = (out * G.cpu().to(dtype)).sum() + (alpha * A.cpu().to(dtype)).sum()
    grads = torch.autograd.grad(loss, ins + [vm], allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(grads, ins + [vm])]


def detached_is_outside(truth, floor, detached, factor):
    """Whether the detached centre's view-matrix gradient breaks the FACTOR x floor rule in both figures, and the figures."""
    (ffro, fmax), (dfro, dmax) = rg.errors(floor[5], truth[5]), rg.errors(detached[5], truth[5])
    return dfro > factor * ffro and dmax > factor * fmax, dict(floor_fro=ffro, floor_max=fmax, detached_fro=dfro, detached_max=dmax)


if __name__ == "__main__":  # the CPU verification of SH_SCALE: no kernel involved, the cut by camera_grad_ref.fixed_cut's rule
    import test_gpu_raster_grad as trg
    case = case_of(trg._t0(sh=True))
    G, A = trg._weights(case)
    geo = [t.double() for t in case["inputs"][:4]]
    args = (case["vm"], case["K"], case["W"], case["H"])
    cut = cg.fixed_cut(geo + [torch.zeros(geo[0].shape[0], 3, dtype=torch.float64)], case["vm"], *args[1:])
    truth = gradients(torch.float64, case["inputs"], G, A, *args, cut)
    floor = gradients(torch.float32, case["inputs"], G, A, *args, cut)
    detached = gradients(torch.float64, case["inputs"], G, A, *args, cut, attached=False)
    print(detached_is_outside(truth, floor, detached, trg.FACTOR))
