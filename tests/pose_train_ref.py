"""The case of train_scene(pose_opt=True, pose_noise=...)'s descent test, and its float64 yardstick.

The case: T0's full scene (every Gaussian, so that the only thing wrong with a render is its camera), its two views perturbed by
POSE_NOISE, POSE_STEPS steps at POSE_LR with the Gaussians held still.  The three numbers were chosen here, on the CPU, with no kernel
involved: yardstick_train() is train_scene's pose loop -- pose.PoseTraining in float64, the same view schedule, the literal photometric
loss -- around the dense float64 render of tests/raster_grad_ref.py, the cut re-decided at every pose by camera_grad_ref.fixed_cut's
rule, against the restatement's own renders from the true views.  `python tests/pose_train_ref.py` prints its pose_err; with the values
below the last is YARDSTICK_FACTOR x the first, which is below the 0.5 the choice was held to.
"""
import torch

import camera_grad_ref as cg
import raster_grad_ref as rg
from gsbp_amd import synthetic as syn
from gsbp_amd.photometric import _literal
from gsbp_amd.polish import view_schedule
from gsbp_amd.pose import PoseTraining

POSE_NOISE, POSE_LR, POSE_STEPS, SEED = 0.02, 5e-3, 60, 3
# pose_err 0.009947 -> 0.002346, the loss 0.1600 -> 0.0020.  (At POSE_LR = 2e-3 the factor is 0.503: the rate has decayed before the
# poses arrive; 4e-3 over 100 steps gives 0.204.)
YARDSTICK_FACTOR = 0.236
SH_C0 = 0.28209479177387814


def scene():
    """T0 as test_gpu_densify.t0_training_setup(stride=1) builds it, on the CPU: (cfg, geometry (means, quats, scales, opacities),
    colours [N, 3], K, viewmats)."""
    cfg = syn.CONFIGS["T0"]
    full = syn.make_scene(cfg)
    n = full["means"].shape[0]
    dc = (torch.rand(n, 1, 3, generator=torch.Generator().manual_seed(syn.SH_SEED)) - 0.5) / SH_C0
    geometry = (full["means"], full["rotation"], torch.exp(full["scaling"]), torch.sigmoid(full["opacity"]))
    return cfg, geometry, (SH_C0 * dc[:, 0] + 0.5).clamp_min(0.0), syn.intrinsics(cfg), syn.make_cameras(cfg)


def yardstick_train(noise=POSE_NOISE, lr=POSE_LR, steps=POSE_STEPS, seed=SEED, reg=0.0):
    cfg, geometry, colors, K, vms = scene()
    ins = [t.double() for t in geometry] + [colors.double()]
    W, H = cfg.width, cfg.height

    def render(vm):
        cut = cg.fixed_cut(ins, vm.detach(), K, W, H)
        return rg.render(*ins, vm, K, W, H, cut)[0]

    targets = [render(vm.double()).clamp(0.0, 1.0).detach() for vm in vms]
    poses = PoseTraining(vms, steps, seed, True, lr, reg, noise, dtype=torch.float64)
    losses = []
    for step, v in enumerate(view_schedule(vms.shape[0], seed, steps)):
        loss = _literal(render(poses.view(v)), targets[v], 0.2, "valid", None)
        loss.backward()
        poses.step(step)
        losses.append(float(loss.detach()))
    return dict(poses.history(), loss=losses)


if __name__ == "__main__":
    import sys
    args = [float(a) for a in sys.argv[1:3]] + [int(a) for a in sys.argv[3:4]]
    h = yardstick_train(*args)
    print("pose_err first, last, factor:", h["pose_err"][0], h["pose_err"][-1], h["pose_err"][-1] / h["pose_err"][0])
    print("loss first, last:", h["loss"][0], h["loss"][-1])
    print("pose_err:", [round(e, 6) for e in h["pose_err"]])
