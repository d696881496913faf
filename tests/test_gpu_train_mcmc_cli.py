"""run_train.py --strategy mcmc on the GPU, as a user starts it: a child process, forty steps on T0 from every second of its Gaussians
under a cap the growth reaches -- the files it writes and the rounds in its history -- and the command line of the default strategy,
which parses as it did before the option existed.
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import run_train  # noqa: E402

pytestmark = pytest.mark.gpu


def test_run_train_mcmc_in_a_child_process(tmp_path, dev):
    out = str(tmp_path / "train")
    done = subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), "--synthetic", "T0", "--steps", "40", "--strategy", "mcmc",
                           "--cap-max", "290", "--refine-start", "5", "--refine-every", "10", "--seed", "3", "--out", out],
                          capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout + done.stderr
    for name in ("trained.pt", "history.json", "metrics.json"):
        assert os.path.getsize(os.path.join(out, name)) > 0, name
    with open(os.path.join(out, "history.json")) as f:
        hist = json.load(f)
    assert hist["strategy"] == "mcmc" and hist["opacity_reg"] == hist["scale_reg"] == 0.01  # the reference's mcmc configuration
    assert hist["config"]["cap_max"] == 290 and hist["config"]["refine_stop_iter"] == 25000 and hist["config"]["min_opacity"] == 0.005
    rounds = hist["rounds"]
    assert [r["step"] for r in rounds] == [10, 20, 30] and set(rounds[0]) == {"step", "n_before", "n_after", "relocated", "added"}
    assert hist["n"][0] == 256 and hist["n"][-1] == rounds[-1]["n_after"] == 290 and max(hist["n"]) <= 290
    assert len(hist["loss"]) == 40 and all(math.isfinite(v) for v in hist["loss"])
    trained = torch.load(os.path.join(out, "trained.pt"))
    assert tuple(trained["means"].shape) == (290, 3) and bool(torch.isfinite(trained["means"]).all())
    with open(os.path.join(out, "metrics.json")) as f:
        assert math.isfinite(json.load(f)["after"]["mean"]["psnr"])


def test_the_default_command_line_parses_as_before():
    """Every option the trainer had keeps its default, and the new ones default to the default strategy with no regulariser."""
    args = vars(run_train.build_parser().parse_args(["--synthetic", "T0"]))
    before = dict(colmap=None, images=None, data_factor=1, synthetic="T0", camera_model="pinhole", rasterize_mode="classic", start_stride=2,
                  params=["means", "scales", "quats", "opacities", "sh0", "shN"], steps=7000, sh_degree=3, ssim_lambda=0.2, seed=0,
                  prune_opa=0.005, grow_grad2d=0.0002, grow_scale3d=0.01, prune_scale3d=0.1, refine_start=500, refine_stop=15000,
                  refine_every=100, reset_every=3000, pause_refine_after_reset=0, scene_scale=None, max_gaussians=None,
                  out="./results/train")
    assert {k: args[k] for k in before} == before
    new = {k: v for k, v in args.items() if k not in before}
    assert new == dict(strategy="default", cap_max=1_000_000, noise_lr=5e5, min_opacity=0.005, opacity_reg=None, scale_reg=None)
    with pytest.raises(SystemExit):
        run_train.build_parser().parse_args(["--synthetic", "T0", "--strategy", "other"])
