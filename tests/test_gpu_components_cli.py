"""run_instances.py --synthetic in a fresh child process: every file exists, instances.json is consistent with instances.pt, the
instances equal split_instances called directly, and --frames writes one frame per view."""
import json
import os
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import components, synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_splits_the_seeded_mask_into_instances(dev, tmp_path):
    out = tmp_path / "inst"
    cfg = syn.CONFIGS["C1"]
    means = syn.activate(syn.make_scene(cfg))[0].float().to(dev)
    mask, ball = components.synthetic_instances(means)
    seed = int(torch.nonzero(ball == 2)[0])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_instances.py"), "--synthetic", "C1", "--radius-factor", "2.0",
                        "--min-points", "3", "--min-size", "20", "--keep-largest", "1", "--seed-index", str(seed), "--frames",
                        "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert {"instances.pt", "instances.json", "mask3d.pt", "frames"} <= set(os.listdir(out))

    saved = torch.load(out / "instances.pt")
    assert set(saved) == {"instances", "sizes", "classes", "core"}
    n = means.shape[0]
    inst, sizes = saved["instances"], saved["sizes"]
    assert inst.shape == (n,) and inst.dtype == torch.int32 and saved["core"].shape == (n,) and saved["core"].dtype == torch.bool
    assert sizes.numel() >= 1 and torch.equal(sizes, torch.bincount(inst[inst >= 0].long(), minlength=sizes.numel()))
    assert bool((sizes[1:] <= sizes[:-1]).all()) and int(sizes.min()) >= 20 and saved["classes"].tolist() == [0] * sizes.numel()
    assert not bool((inst >= 0)[~mask.cpu()].any())  # nothing outside the mask is in an instance

    radius = gsbp_amd.suggest_radius(means, factor=2.0, mask=mask)
    want = gsbp_amd.split_instances(means, mask, radius, 3, 20)
    assert torch.equal(inst, want.instances.cpu()) and torch.equal(sizes, want.sizes.cpu()) and torch.equal(saved["core"], want.core.cpu())
    keep = torch.load(out / "mask3d.pt")
    assert torch.equal(keep, gsbp_amd.select_components(want, seeds=[seed], largest=1).cpu()) and bool(keep[inst == 0].all())

    rep = json.load(open(out / "instances.json"))
    assert rep["n"] == n and rep["live"] == int(mask.sum()) and rep["radius"] == radius and rep["min_points"] == 3
    assert rep["instances"] == sizes.numel() and rep["largest"] == sizes[:10].tolist() and rep["core"] == int(saved["core"].sum())
    assert rep["in_instances"] == int((inst >= 0).sum()) and rep["noise"] == rep["live"] - rep["in_instances"]
    assert rep["selected"] == int(keep.sum())
    grid = rep["grid"]
    assert grid["cells"] == grid["dims"][0] * grid["dims"][1] * grid["dims"][2] and grid["cell_size"] >= radius * (1 - 2.0 ** -23)
    assert 0 < grid["occupied_cells"] <= grid["cells"] and grid["points_in_cells"] == n

    frames = os.listdir(out / "frames")
    assert frames == ["frames.pt"] or len(frames) == cfg.n_views
    if frames == ["frames.pt"]:
        assert torch.load(out / "frames" / "frames.pt").shape == (cfg.n_views, cfg.height, cfg.width, 3)
