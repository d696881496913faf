"""run_localize.py in a fresh child process on the T0 scene: the table and the target are written to a temporary directory, the start
is the true view moved by the refinement case's twist (tests/camera_grad_ref.py), and the JSON it writes holds a 4 x 4 view matrix that
is closer to the truth than the start was."""
import json
import os
import subprocess
import sys

import pytest
import torch

import camera_grad_ref as cg
from gsbp_amd import rasterization
from gsbp_amd.pose import pose_error

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_localize_refines_a_perturbed_pose(dev, tmp_path):
    case = cg.pose_case()
    gauss = [t.to(dev) for t in case["inputs"]]
    with torch.no_grad():
        target = rasterization(*gauss, case["table"].to(dev), case["vm_true"].to(dev)[None], case["K"].to(dev)[None], case["W"],
                               case["H"], want_meta=False)[0][0]
    torch.save(case["table"], tmp_path / "table.pt")
    torch.save(target.cpu(), tmp_path / "target.pt")
    out = tmp_path / "pose.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_localize.py"), "--synthetic", "T0", "--field", str(tmp_path / "table.pt"),
                        "--target", str(tmp_path / "target.pt"), "--init-view", "0", "--perturb",
                        ",".join(str(x) for x in cg.POSE_TWIST0), "--steps", str(cg.POSE_STEPS), "--lr", str(cg.POSE_LR), "--out",
                        str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rep = json.loads(out.read_text())
    vm = torch.tensor(rep["viewmat"], dtype=torch.float64)
    assert vm.shape == (4, 4) and torch.equal(vm[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))
    assert len(rep["history"]) == cg.POSE_STEPS and rep["history"][-1] < rep["history"][0]
    start = torch.tensor(rep["initial_viewmat"], dtype=torch.float64)
    assert float((start - case["vm0"]).abs().max()) < 1e-6
    a0, d0 = pose_error(start, case["vm_true"])
    a1, d1 = pose_error(vm, case["vm_true"])
    print(f"run_localize.py: angle {a0:.4f} -> {a1:.4f} rad, distance {d0:.4f} -> {d1:.4f}")
    assert a1 < a0 and d1 < d0
