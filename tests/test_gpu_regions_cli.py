"""run_regions.py --synthetic in fresh child processes: every file exists, regions.pt equals the library call, regions.json is consistent
with the tensors, a second run writes the same labels, and --levels / --frames / --save-similarity write what they say."""
import json
import os
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import regions, synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cli(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_regions.py"), "--synthetic", "C1", *args], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def scene(dev):
    means = syn.activate(syn.make_scene(syn.CONFIGS["C1"]))[0].float().to(dev)
    return means, regions.synthetic_regions(means)[0].to(dev)


def test_cli_grows_the_seeded_regions(dev, tmp_path):
    out, again = tmp_path / "reg", tmp_path / "again"
    cli("--sim-min", "0.9", "--min-size", "3", "--out", str(out))
    cli("--sim-min", "0.9", "--min-size", "3", "--out", str(again))
    assert {"regions.pt", "regions.json"} <= set(os.listdir(out)) and "frames" not in os.listdir(out)
    saved = torch.load(out / "regions.pt")
    assert set(saved) == {"labels", "sizes"}
    labels, sizes = saved["labels"], saved["sizes"]
    assert labels.numpy().tobytes() == torch.load(again / "regions.pt")["labels"].numpy().tobytes()

    means, feats = scene(dev)
    n = means.shape[0]
    want = gsbp_amd.similarity_components(means, feats, k=8, sim_min=0.9, min_size=3)
    assert labels.shape == (n,) and labels.dtype == torch.int32
    assert torch.equal(labels, want.labels.cpu()) and torch.equal(sizes, want.sizes.cpu())
    assert torch.equal(sizes, torch.bincount(labels[labels >= 0].long(), minlength=sizes.numel())) and int(sizes.min()) >= 3

    rep = json.load(open(out / "regions.json"))
    live = gsbp_amd.neighbor_similarity(feats, gsbp_amd.spatial_knn(means, 9)[1])[1]
    assert rep["n"] == n and rep["k"] == 8 and rep["thresholds"] == [0.9] and rep["radius"] is None and rep["min_size"] == 3
    assert rep["regions"] == sizes.numel() and rep["in_regions"] == int((labels >= 0).sum())
    assert rep["largest"] == sizes.sort(descending=True).values[:10].tolist()
    assert rep["dead_rows"] == n - int(live.sum()) > 0 and rep["live"] == int(want.core.sum()) == int(live.sum())
    q = rep["similarity_quantiles"]
    assert list(q) == ["0.01", "0.1", "0.25", "0.5", "0.75", "0.9", "0.99"] and list(q.values()) == sorted(q.values())
    assert -1.0 <= q["0.01"] and q["0.99"] <= 1.0 + 1e-6 and rep["valid_similarities"] > 0
    grid = rep["grid"]
    assert grid["cells"] == grid["dims"][0] * grid["dims"][1] * grid["dims"][2] and grid["points_in_cells"] == n


def test_cli_levels_frames_and_similarity(dev, tmp_path):
    out = tmp_path / "lev"
    cfg = syn.CONFIGS["C1"]
    cli("--levels", "0.5,0.9", "--radius-factor", "3", "--frames", "--save-similarity", "--out", str(out))
    assert {"regions.pt", "regions.json", "frames", "neighbors.pt", "similarity.pt"} <= set(os.listdir(out))
    saved = torch.load(out / "regions.pt")
    assert set(saved) == {"labels", "sizes", "levels"}
    means, feats = scene(dev)
    radius = gsbp_amd.suggest_radius(means, factor=3.0)
    nb = gsbp_amd.spatial_knn(means, 9)
    want = gsbp_amd.similarity_levels(means, feats, [0.5, 0.9], radius=radius, neighbors=nb)
    assert torch.equal(saved["levels"], want.cpu()) and torch.equal(saved["labels"], want[1].cpu())
    assert torch.equal(saved["sizes"], torch.bincount(saved["labels"][saved["labels"] >= 0].long()))
    rep = json.load(open(out / "regions.json"))
    assert rep["thresholds"] == [0.5, 0.9] and rep["radius"] == radius
    assert rep["regions_per_level"] == [int(row.max()) + 1 for row in saved["levels"]] and rep["regions"] == rep["regions_per_level"][1]
    nbs = torch.load(out / "neighbors.pt")
    assert torch.equal(nbs["idx"], nb[1].cpu()) and torch.equal(nbs["dist"], nb[0].cpu())
    sim = torch.load(out / "similarity.pt")
    got = gsbp_amd.neighbor_similarity(feats, nb[1])[0].cpu()
    assert torch.equal(torch.isnan(sim), torch.isnan(got)) and torch.equal(sim[~torch.isnan(sim)], got[~torch.isnan(got)])
    frames = os.listdir(out / "frames")
    assert frames == ["frames.pt"] or len(frames) == cfg.n_views
    if frames == ["frames.pt"]:
        assert torch.load(out / "frames" / "frames.pt").shape == (cfg.n_views, cfg.height, cfg.width, 3)
