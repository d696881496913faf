"""train_scene with the depth term: depth_fn in both forms, the history, the refusal, a descent check and the
command line.

THE DESCENT CHECK tests the loss, not the kernel.  One view of T0; the start is the true scene with every mean pushed away from that
view's camera centre along its ray, means' = c + (1 + DISPLACE) (means - c), scales as they were.  From one view such a start renders
nearly the true image (a ray keeps its pixel), so the photometric loss says little about where along the ray a Gaussian lies; the
depth term says it.  Only the means are trained (lr 1e-2), 40 steps, the same seeds twice: depth_lambda = 0 and depth_lambda = LAMBDA.
The run that trains on the term must end with the lower mean depth loss over its last five steps.  DISPLACE and LAMBDA were
established with the literal torch expression (tests/depth_loss_ref.literal_point_loss, its 1 / d guarded) standing in for the kernel
inside train_scene: see DESCENT below for the figures measured on an MI355X.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd.polish import render_splats
from test_gpu_densify import t0_training_setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 24
DISPLACE, LAMBDA, DESCENT_STEPS = 0.1, 1.0, 40
# DESCENT, measured on an MI355X, mean depth loss of the last five steps (first step 0.059434 in every run):
#   literal stand-in, DISPLACE 0.1:  lambda 0: 0.028295   lambda 0.1: 0.024278   lambda 1: 0.008570      (kernel: 0.028294, 0.024274, 0.008567)
#   literal stand-in, DISPLACE 0.25: lambda 0: 0.081987   lambda 0.1: 0.077715   lambda 1: 1.911264      (first step 4.09: at that
#       displacement samples fall on the rim of the pushed scene, 1 / d is huge there and Adam's first steps overshoot)
# The smallest setting with a clear margin: DISPLACE 0.1, LAMBDA 1 (a factor 3.3 between the two means; lambda 0.1 leaves 1.17).
QUIET = gsbp_amd.DensifyConfig(refine_start_iter=10 ** 6)  # no round, no reset: the set stays as it is


def true_depth_points(dev, full, vms, K, cfg, n=256, seed=7):
    """Per view: n seeded positions and the true scene's depth there under the loss's own sampling rule, empty samples dropped."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for v in range(vms.shape[0]):
        xy = (torch.rand(n, 2, generator=gen) * torch.tensor([cfg.width - 1.0, cfg.height - 1.0])).to(dev)
        with torch.no_grad():
            render, alpha = render_splats(full, vms[v], K, cfg.width, cfg.height, render_mode="RGB+D", return_alpha=True)
            d = gsbp_amd.sample_expected_depth(render, alpha, xy)
        out.append((xy[d > 0].contiguous(), d[d > 0].contiguous(), render, alpha))
    return out


@pytest.fixture(scope="module")
def setup(dev):
    cfg, start, K, vms, images = t0_training_setup(dev)
    _, full, _, _, _ = t0_training_setup(dev, stride=1)
    return cfg, start, full, K, vms, images, true_depth_points(dev, full, vms, K, cfg)


def test_both_forms_of_depth_fn_and_the_history(dev, setup):
    cfg, start, full, K, vms, images, truth = setup
    args = (start, vms, K, cfg.width, cfg.height, lambda v: images[v], STEPS)
    _, plain = gsbp_amd.train_scene(*args, cfg=QUIET, seed=1)
    assert "depth_loss" not in plain
    _, by_points = gsbp_amd.train_scene(*args, cfg=QUIET, seed=1, depth_fn=lambda v: truth[v][:2], depth_lambda=0.1)
    maps = [(t[2][..., 3] / t[3][..., 0].clamp_min(1e-10)).contiguous() for t in truth]  # the true expected depth, 0 where empty
    _, by_map = gsbp_amd.train_scene(*args, cfg=QUIET, seed=1, depth_fn=lambda v: maps[v], depth_lambda=0.1, depth_kind="depth")
    _, mixed = gsbp_amd.train_scene(*args, cfg=QUIET, seed=1, depth_fn=lambda v: None if v else truth[v][:2])
    for hist in (by_points, by_map, mixed):
        assert set(hist) == set(plain) | {"depth_loss"}
        assert len(hist["depth_loss"]) == STEPS == len(hist["loss"]) and np.isfinite(hist["depth_loss"]).all()
        assert np.isfinite(hist["loss"]).all() and hist["n"] == plain["n"]
    assert min(by_points["depth_loss"]) > 0 and min(by_map["depth_loss"]) > 0
    assert 0.0 in mixed["depth_loss"] and max(mixed["depth_loss"]) > 0   # a view without supervision adds nothing
    assert by_points["loss"] != plain["loss"]                              # the term is in the step's loss
    with pytest.raises(gsbp_amd.GwbpError, match="render_mode"):
        gsbp_amd.train_scene(*args, cfg=QUIET, depth_fn=lambda v: truth[v][:2], render_mode="RGB+ED")
    with pytest.raises(gsbp_amd.GwbpError, match="depth_fn"):
        gsbp_amd.train_scene(*args, cfg=QUIET, depth_fn=lambda v: 3.0)
    # under the MCMC strategy the term runs too
    _, hist = gsbp_amd.train_scene(*args[:-1], 6, strategy=gsbp_amd.MCMCConfig(cap_max=400, refine_start_iter=10 ** 6), seed=1,
                                   depth_fn=lambda v: truth[v][:2])
    assert len(hist["depth_loss"]) == 6 and np.isfinite(hist["depth_loss"]).all()


def displaced_run(dev, setup, depth_lambda):
    cfg, _, full, K, vms, images, truth = setup
    vm = vms[:1]
    centre = -(vm[0, :3, :3].T @ vm[0, :3, 3])
    start = dict(full, means=(centre + (1.0 + DISPLACE) * (full["means"] - centre)).contiguous())
    _, hist = gsbp_amd.train_scene(start, vm, K, cfg.width, cfg.height, lambda v: images[0], DESCENT_STEPS, cfg=QUIET, seed=2,
                                   params=("means",), lrs={"means": 1e-2}, depth_fn=lambda v: truth[0][:2], depth_lambda=depth_lambda)
    return hist["depth_loss"]


def test_training_on_the_term_lowers_it(dev, setup):
    without, with_term = displaced_run(dev, setup, 0.0), displaced_run(dev, setup, LAMBDA)
    a, b = float(np.mean(without[-5:])), float(np.mean(with_term[-5:]))
    print(f"mean depth loss of the last five steps: lambda 0: {a:.6f} (first step {without[0]:.6f}); lambda {LAMBDA}: {b:.6f}")
    assert abs(without[0] - with_term[0]) <= 1e-6 * without[0] and b < a


def test_the_command_line_writes_the_depth_losses(dev, tmp_path):
    out = str(tmp_path / "train")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "run_train.py"), "--synthetic", "T0", "--depth-loss", "--steps", "20",
                           "--out", out])
    hist = json.load(open(os.path.join(out, "history.json")))
    assert len(hist["depth_loss"]) == 20 and np.isfinite(hist["depth_loss"]).all() and min(hist["depth_loss"]) > 0
    assert hist["depth_lambda"] == 1e-2 and hist["depth_scale"] == 1.0
