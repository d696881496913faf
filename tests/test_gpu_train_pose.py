"""train_scene with pose_opt and pose_noise: the call without the keywords, the monitor, a descent condition chosen on
the float64 yardstick of tests/pose_train_ref.py, the option beside both strategies, the optimisers and the other loss terms, a densify
round on the way, the refusals, and run_train.py in process.
"""
import json
import math
import os
import sys

import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import pose_train_ref as ptr  # noqa: E402
from test_gpu_densify import probe_thresholds, t0_training_setup  # noqa: E402

import gsbp_amd  # noqa: E402
from gsbp_amd.polish import splat_geometry  # noqa: E402

pytestmark = pytest.mark.gpu
QUIET = gsbp_amd.DensifyConfig(refine_start_iter=10 ** 6)  # no round, no reset: the set stays as it is
POSE = dict(pose_opt=True, pose_opt_lr=1e-3, pose_noise=0.01)


@pytest.fixture(scope="module")
def setup(dev):
    return t0_training_setup(dev)


def check_pose_history(hist, vms, steps):
    v = vms.shape[0]
    assert hist["pose_adjust"].shape == (v, 9) and hist["pose_adjust"].dtype == torch.float32 and bool(hist["pose_adjust"].any())
    assert bool(torch.isfinite(hist["pose_adjust"]).all()) and not hist["pose_adjust"].requires_grad
    assert hist["viewmats"].shape == (v, 4, 4) and not torch.equal(hist["viewmats"], vms)
    assert len(hist["loss"]) == steps and all(math.isfinite(x) for x in hist["loss"])
    if "pose_err" in hist:
        assert len(hist["pose_err"]) == steps and all(math.isfinite(x) and x > 0 for x in hist["pose_err"])


def test_the_defaults_are_the_call_without_the_keywords(dev, setup):
    """The loss bits of the call that passes the four keywords at their defaults, on the two-tile crop of
    test_gpu_sh_grad.py::test_no_interval_is_the_call_without_the_keyword, where training is reproducible by construction."""
    cfg, start, K, vms, images = setup
    w, h = 32, 16
    x0, y0 = (cfg.width - w) // 2, (cfg.height - h) // 2
    Kc = K.clone()
    Kc[0, 2] -= x0
    Kc[1, 2] -= y0
    crops = [im[y0:y0 + h, x0:x0 + w].contiguous() for im in images]
    plain = gsbp_amd.train_scene(start, vms, Kc, w, h, lambda v: crops[v], 40, seed=3)[1]
    given = gsbp_amd.train_scene(start, vms, Kc, w, h, lambda v: crops[v], 40, seed=3, pose_opt=False, pose_opt_lr=1e-5,
                                 pose_opt_reg=1e-6, pose_noise=0.0)[1]
    assert len(plain["loss"]) == 40 and plain["loss"] == given["loss"] and plain["n"] == given["n"] and set(plain) == set(given)
    assert plain["loss"][-1] < plain["loss"][0] and len(set(plain["loss"])) == 40
    assert not {"pose_err", "pose_adjust", "viewmats"} & set(plain)


def test_noise_alone_leaves_a_constant_error(dev, setup):
    cfg, start, K, vms, images = setup
    args = (start, vms, K, cfg.width, cfg.height, lambda v: images[v], 6)
    _, plain = gsbp_amd.train_scene(*args, cfg=QUIET, seed=1)
    _, hist = gsbp_amd.train_scene(*args, cfg=QUIET, seed=1, pose_noise=0.02)
    assert set(hist) == set(plain) | {"pose_err", "viewmats"}
    assert len(hist["pose_err"]) == 6 and len(set(hist["pose_err"])) == 1 and hist["pose_err"][0] > 0
    assert hist["viewmats"].shape == vms.shape and not torch.equal(hist["viewmats"], vms)
    assert hist["loss"][0] > plain["loss"][0]  # (the perturbed views see the targets from elsewhere)
    _, again = gsbp_amd.train_scene(*args, cfg=QUIET, seed=1, pose_noise=0.02)
    assert torch.equal(again["viewmats"], hist["viewmats"]) and again["pose_err"] == hist["pose_err"]  # drawn from the seed
    _, other = gsbp_amd.train_scene(*args, cfg=QUIET, seed=2, pose_noise=0.02)
    assert not torch.equal(other["viewmats"], hist["viewmats"])
    # pose_opt without noise: a correction is learnt, and there is no truth to monitor against
    _, opt = gsbp_amd.train_scene(*args, cfg=QUIET, seed=1, pose_opt=True, pose_opt_lr=1e-3)
    assert set(opt) == set(plain) | {"pose_adjust", "viewmats"}
    check_pose_history(opt, vms, 6)


def test_the_poses_move_towards_the_truth(dev):
    """A condition, not a measurement: with the perturbed views of the true scene and the Gaussians held still (sh0 at rate 0, nothing
    else trained), the last pose_err is below the first.  The float64 dense yardstick under the same loop reaches
    ptr.YARDSTICK_FACTOR = 0.236 (tests/pose_train_ref.py, where noise, rate and step count were chosen for a factor of at most 0.5)."""
    cfg, full, K, vms, images = t0_training_setup(dev, stride=1)
    _, hist = gsbp_amd.train_scene(full, vms, K, cfg.width, cfg.height, lambda v: images[v], ptr.POSE_STEPS, cfg=QUIET, seed=ptr.SEED,
                                   params=("sh0",), lrs={"sh0": 0.0}, pose_opt=True, pose_opt_lr=ptr.POSE_LR, pose_opt_reg=0.0,
                                   pose_noise=ptr.POSE_NOISE)
    check_pose_history(hist, vms, ptr.POSE_STEPS)
    factor = hist["pose_err"][-1] / hist["pose_err"][0]
    print(f"pose_err {hist['pose_err'][0]:.6f} -> {hist['pose_err'][-1]:.6f}: x {factor:.4f} in {ptr.POSE_STEPS} steps; the float64 "
          f"yardstick: x {ptr.YARDSTICK_FACTOR:.4f}; loss {hist['loss'][0]:.5f} -> {hist['loss'][-1]:.5f}")
    assert ptr.YARDSTICK_FACTOR <= 0.5
    assert hist["pose_err"][-1] < hist["pose_err"][0]
    assert hist["loss"][-1] < hist["loss"][0]


def feature_setup(dev, cfg, K, vms):
    full = {k: t.to(dev) for k, t in gsbp_amd.synthetic.make_scene(cfg).items()}
    gen = torch.Generator().manual_seed(77)
    latents = torch.rand(full["means"].shape[0], 16, generator=gen).to(dev)
    decoder = (torch.rand(16, 32, generator=gen) / 16).to(dev)
    with torch.no_grad():
        return [gsbp_amd.render_latents(*splat_geometry(full), latents, vms[v], K, cfg.width, cfg.height)[0] @ decoder
                for v in range(vms.shape[0])]


@pytest.mark.parametrize("name", ["mcmc", "visible", "fused", "features", "depth", "interval"])
def test_pose_opt_beside_the_other_options(dev, setup, name):
    cfg, start, K, vms, images = setup
    steps, kw = 8, dict(cfg=QUIET)
    if name == "mcmc":
        steps, kw = 14, dict(strategy=gsbp_amd.MCMCConfig(refine_start_iter=3, refine_every=5, cap_max=290), opacity_reg=0.01,
                             scale_reg=0.01)
    elif name in ("visible", "fused"):
        kw["adam"] = name
    elif name == "features":
        maps = feature_setup(dev, cfg, K, vms)
        kw.update(feature_fn=lambda v: maps[v], feature_dim=32, latent_dim=16)
    elif name == "depth":
        gen = torch.Generator().manual_seed(7)
        xy = (torch.rand(64, 2, generator=gen) * torch.tensor([cfg.width - 1.0, cfg.height - 1.0])).to(dev)
        kw.update(depth_fn=lambda v: (xy, torch.full((64,), 3.0, device=dev)), depth_lambda=0.1)
    elif name == "interval":
        start = dict(start, features_rest=torch.zeros(start["means"].shape[0], 15, 3, device=dev))
        kw["sh_degree_interval"] = 2  # steps 2 .. at degree >= 1: the colours then depend on the camera centre
    trained, hist = gsbp_amd.train_scene(start, vms, K, cfg.width, cfg.height, lambda v: images[v], steps, seed=3, **POSE, **kw)
    check_pose_history(hist, vms, steps)
    assert "pose_adjust" not in trained and "viewmats" not in trained
    assert all(bool(torch.isfinite(t).all()) for t in trained.values() if torch.is_tensor(t))
    if name == "mcmc":
        assert [r["step"] for r in hist["rounds"]] == [5, 10] and trained["means"].shape[0] > start["means"].shape[0]
    if name == "features":
        assert len(hist["feature_loss"]) == steps and trained["features"].shape == (start["means"].shape[0], 16)
    if name == "depth":
        assert len(hist["depth_loss"]) == steps
    if name == "interval":
        assert hist["sh_degree"] == [min(s // 2, 3) for s in range(steps)] and bool(trained["features_rest"].any())


def test_a_densify_round_on_the_way(dev, setup):
    """The default strategy with a round inside: N changes, the [V, 9] table does not (it lives in history, not in the dict that the
    round moves row by row)."""
    cfg, start, K, vms, images = setup
    _, _, grow, opa = probe_thresholds(dev, start, K, vms, images, cfg)  # (the data's own thresholds: a round then changes the set)
    dcfg = gsbp_amd.DensifyConfig(refine_start_iter=3, refine_every=5, grow_grad2d=grow, prune_opa=opa, grow_scale3d=0.06,
                                  prune_scale3d=0.25)
    trained, hist = gsbp_amd.train_scene(start, vms, K, cfg.width, cfg.height, lambda v: images[v], 14, cfg=dcfg, seed=3, **POSE)
    check_pose_history(hist, vms, 14)
    assert [r["step"] for r in hist["rounds"]] == [5, 10] and any(r["n_after"] != r["n_before"] for r in hist["rounds"])
    assert trained["means"].shape[0] == hist["rounds"][-1]["n_after"] and len(set(hist["n"])) > 1


def test_bad_values_raise(dev, setup):
    cfg, start, K, vms, images = setup
    args = (start, vms, K, cfg.width, cfg.height, lambda v: images[v], 4)
    for name in ("pose_opt_lr", "pose_opt_reg", "pose_noise"):
        for bad in (-1e-3, float("nan"), float("inf"), "0.1", True):
            with pytest.raises(gsbp_amd.GwbpError, match=name):
                gsbp_amd.train_scene(*args, pose_opt=True, **{name: bad})
    with pytest.raises(gsbp_amd.GwbpError, match="pose_opt must be a bool"):
        gsbp_amd.train_scene(*args, pose_opt=1)
    for kw in (dict(pose_opt=True), dict(pose_noise=0.1)):
        with pytest.raises(gsbp_amd.GwbpError, match="at least one view"):
            gsbp_amd.train_scene(start, vms[:0], K, cfg.width, cfg.height, lambda v: images[v], 4, **kw)


def test_the_command_line_tool_takes_the_options(dev, tmp_path):
    import run_train
    out = str(tmp_path / "train")
    assert run_train.main(["--synthetic", "T0", "--steps", "10", "--pose-opt", "--pose-opt-lr", "1e-3", "--pose-noise", "0.01",
                           "--out", out]) == 0
    with open(os.path.join(out, "history.json")) as f:
        hist = json.load(f)
    assert len(hist["pose_err"]) == 10 == len(hist["loss"]) and hist["pose_opt"] is True and hist["pose_opt_lr"] == 1e-3
    assert hist["pose_noise"] == 0.01 and "pose_opt_reg" not in hist
    poses = torch.load(os.path.join(out, "poses.pt"))
    assert poses["pose_adjust"].shape == (2, 9) and poses["viewmats"].shape == (2, 4, 4) and poses["views"] == hist["views"]
    assert bool(poses["pose_adjust"].any())
    with open(os.path.join(out, "metrics.json")) as f:
        assert set(json.load(f)) == {"before", "after"}
    # the noise alone: no table; neither option: no file
    alone = str(tmp_path / "noise")
    assert run_train.main(["--synthetic", "T0", "--steps", "4", "--pose-noise", "0.01", "--out", alone]) == 0
    assert "pose_adjust" not in torch.load(os.path.join(alone, "poses.pt"))
    none = str(tmp_path / "none")
    assert run_train.main(["--synthetic", "T0", "--steps", "4", "--out", none]) == 0
    assert not os.path.exists(os.path.join(none, "poses.pt"))
    with open(os.path.join(none, "history.json")) as f:
        assert not {"pose_err", "pose_opt", "pose_noise"} & set(json.load(f))
    for argv in (["--pose-opt-lr", "1e-3"], ["--pose-opt-reg", "1e-6"]):
        with pytest.raises(SystemExit):
            run_train.main(["--synthetic", "T0", "--steps", "4", "--out", none] + argv)
    help_text = run_train.build_parser().format_help()
    assert all(opt in help_text for opt in ("--pose-opt", "--pose-opt-lr", "--pose-opt-reg", "--pose-noise"))
