"""run_clean.py --synthetic: its files exist, its labels equal smooth_labels called directly, clean.json carries the grid statistics."""
import json
import os
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import spatial, synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_cleans_the_seeded_inputs(dev, tmp_path):
    out = tmp_path / "cleaned"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_clean.py"), "--synthetic", "C1", "--k", "8", "--remove-outliers",
                        "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert {"labels.pt", "mask3d.pt", "neighbors.pt", "clean.json"} <= set(os.listdir(out)) and "features.pt" not in os.listdir(out)

    means = syn.make_scene(syn.CONFIGS["C1"])["means"].float().to(dev)
    n = means.shape[0]
    noisy, clean = spatial.synthetic_labels(means, 6)
    dist, idx = gsbp_amd.spatial_knn(means, 8)
    nb = torch.load(out / "neighbors.pt")
    assert torch.equal(nb["idx"], idx.cpu()) and torch.equal(nb["dist"], dist.cpu())
    want = gsbp_amd.smooth_labels(means, noisy, 6, k=8)
    got = torch.load(out / "labels.pt")
    assert torch.equal(got, want.cpu())
    assert int((noisy != clean).sum()) > 0 and int((want.cpu() != noisy.cpu()).sum()) > 0  # (there was something to clean)

    mask, _ = spatial.synthetic_mask(means)
    smoothed = gsbp_amd.smooth_mask(means, mask, neighbors=idx)
    kept = gsbp_amd.remove_outliers(means, smoothed, k=8, std_ratio=2.0)
    assert torch.equal(torch.load(out / "mask3d.pt"), kept.cpu())

    rep = json.load(open(out / "clean.json"))
    assert rep["n"] == n and rep["k"] == 8 and rep["labels"]["changed"] == int((want.cpu() != noisy.cpu()).sum())
    assert rep["mask"]["before"] == int(mask.sum()) and rep["mask"]["after"] == int(kept.sum())
    assert rep["mask"]["outliers_removed"] == int(smoothed.sum()) - int(kept.sum())
    grid = rep["grid"]
    assert grid["cells"] == grid["dims"][0] * grid["dims"][1] * grid["dims"][2] and grid["cell_size"] > 0
    assert 0 < grid["occupied_cells"] <= grid["cells"] and grid["points_in_cells"] == n
    assert 1 <= grid["p99_occupancy"] <= grid["max_occupancy"]


def test_cli_smooths_a_field_from_a_file(dev, tmp_path):
    means = syn.make_scene(syn.CONFIGS["T0"])["means"].float().to(dev)
    feats = torch.randn(means.shape[0], 20, generator=torch.Generator().manual_seed(2))
    torch.save(feats, tmp_path / "f.pt")
    out = tmp_path / "o"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_clean.py"), "--synthetic", "T0", "--k", "4", "--features", str(tmp_path / "f.pt"),
                        "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert set(os.listdir(out)) == {"features.pt", "neighbors.pt", "clean.json"}
    assert torch.equal(torch.load(out / "features.pt"), gsbp_amd.smooth_features(means, feats.to(dev), k=4).cpu())
