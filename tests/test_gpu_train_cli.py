"""run_train.py on the GPU: sixty steps on T0 from every second of its Gaussians, with thresholds a ten-step probe chose, through the
command line's main() -- the schedule, the files it writes, and that the set changed size the way the rounds say.

The probe's thresholds are a stress setting, not a training one: grow_grad2d at the median makes half of the counted Gaussians grow in
EVERY round, four rounds ten steps apart.  What they grow into is this test's choice.  With --grow-scale3d 0.06 (the scene's median
scale: half of the grown ones split) each round re-draws a quarter of a 256-Gaussian scene one standard deviation away from where it
was, and the loss does not come back in the nine steps that follow the last round: measured on an MI355X, 0.162 at step 20, 0.238 at
step 21, 0.217 at step 59 against 0.206 at step 0 (N 256 -> 1257); the same run without rounds ends at 0.094, and with the gradient
threshold four times the median at 0.157.  The splits are the rule's, bit for bit (test_gpu_densify.py::test_emit, ::test_densify_round_trip), so
this run grows by cloning instead -- --grow-scale3d above every scale of the scene, which the rule allows -- and ends at 0.168 with the
same four rounds (N 256 -> 876).  At a size where growth has room the rule pays as it stands: T1 from every second Gaussian, 200 steps,
29.6 dB with train_scene against 28.6 dB with polish_scene (profiles/densify.json)."""
import json
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import run_train  # noqa: E402
from test_gpu_densify import probe_thresholds, t0_training_setup  # noqa: E402

pytestmark = pytest.mark.gpu


def test_run_train_synthetic(tmp_path, dev):
    cfg, start, K, vms, images = t0_training_setup(dev)
    _, _, grow, opa = probe_thresholds(dev, start, K, vms, images, cfg)
    assert grow > 0 and 0 < opa < 0.5
    out = str(tmp_path / "train")
    rc = run_train.main(["--synthetic", "T0", "--steps", "60", "--refine-start", "10", "--refine-every", "10", "--start-stride", "2",
                         "--grow-grad2d", repr(grow), "--prune-opa", repr(opa), "--grow-scale3d", "10", "--prune-scale3d", "100",
                         "--seed", "3", "--out", out])
    assert rc == 0
    with open(os.path.join(out, "history.json")) as f:
        hist = json.load(f)
    with open(os.path.join(out, "metrics.json")) as f:
        metrics = json.load(f)
    loss, sizes, rounds = hist["loss"], hist["n"], hist["rounds"]
    assert len(loss) == len(sizes) == 60 and all(math.isfinite(v) for v in loss)
    assert [r["step"] for r in rounds] == [20, 30, 40, 50] and hist["resets"] == []
    assert sizes[0] == start["means"].shape[0] and len(set(sizes)) > 1  # N changed at least once ...
    by_step = {r["step"]: r for r in rounds}
    for s in range(1, 60):                                               # ... and only where a round says so, by what it says
        if sizes[s] != sizes[s - 1]:
            r = by_step[s - 1]
            assert (r["n_before"], r["n_after"]) == (sizes[s - 1], sizes[s])
    assert sum(r["cloned"] for r in rounds) > 0 and sum(r["pruned"] for r in rounds) > 0
    for r in rounds:
        assert r["n_before"] == r["pruned"] + r["kept"] + r["cloned"] + r["split"]
        assert r["n_after"] == r["kept"] + 2 * (r["cloned"] + r["split"]) == sizes[r["step"] + 1]
    assert loss[-1] < loss[0]
    trained = torch.load(os.path.join(out, "trained.pt"))
    n = sizes[-1] if rounds[-1]["step"] != 59 else rounds[-1]["n_after"]
    for k, tail in (("means", (3,)), ("scaling", (3,)), ("rotation", (4,)), ("opacity", ()), ("features_dc", (1, 3)), ("features_rest", (0, 3))):
        assert tuple(trained[k].shape) == (n,) + tail and bool(torch.isfinite(trained[k]).all()), k
    assert set(metrics) == {"before", "after"} and math.isfinite(metrics["after"]["mean"]["psnr"])
    print(f"T0 from every second Gaussian, 60 steps: N {sizes[0]} -> {n}, loss {loss[0]:.4f} -> {loss[-1]:.4f}, "
          f"PSNR {metrics['before']['mean']['psnr']:.2f} -> {metrics['after']['mean']['psnr']:.2f} dB")
