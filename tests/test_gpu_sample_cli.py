"""run_sample.py --synthetic in a fresh child process: every file exists with its shapes, the tensors equal the library calls, and
the counts of sample.json are consistent with them."""
import argparse
import json
import os
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import cli, regions, sample

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_samples_the_synthetic_scene(dev, tmp_path):
    out = tmp_path / "smp"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_sample.py"), "--synthetic", "C1", "--num-classes", "6", "--fallback",
                        "nearest", "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert {"sampled_features.pt", "sampled_labels.pt", "point_gaussians.pt", "sample.json", "metrics.json"} <= set(os.listdir(out))
    gauss = cli.load_scene(argparse.Namespace(synthetic="C1"), dev).gauss  # (activated on the device, as the command line does)
    n = gauss[0].shape[0]
    pts = sample.synthetic_points(gauss[0])
    q = pts.shape[0]
    pgs = torch.load(out / "point_gaussians.pt")
    want = gsbp_amd.point_gaussians(pts, *gauss, k=8)
    assert pgs["idx"].shape == (q, 8) and pgs["idx"].dtype == torch.int32 and pgs["weights"].shape == (q, 8) and pgs["n_contrib"].shape == (q,)
    assert torch.equal(pgs["points"], pts.cpu()) and torch.equal(pgs["idx"], want.idx.cpu())
    assert torch.equal(pgs["weights"], want.weights.cpu()) and torch.equal(pgs["n_contrib"], want.n_contrib.cpu())
    sf, sl = torch.load(out / "sampled_features.pt"), torch.load(out / "sampled_labels.pt")
    assert sf["features"].shape == (q, 64) and sf["valid"].shape == (q,) and sf["wsum"].shape == (q,)
    assert sl["labels"].shape == (q,) and sl["labels"].dtype == torch.int32 and sl["share"].shape == (q,)
    assert torch.equal(sf["valid"], pgs["n_contrib"] > 0) and torch.equal(sl["labels"] >= 0, sf["valid"])
    assert bool(((sl["share"] > 0) & (sl["share"] <= 1))[sf["valid"]].all()) and bool(torch.isfinite(sf["features"]).all())

    rep = json.load(open(out / "sample.json"))
    assert rep["n"] == n and rep["points"] == q == rep["finite_points"] and rep["k"] == 8 and rep["radius"] == want.radius
    assert rep["valid"] == int(sf["valid"].sum()) and rep["truncated"] == int((pgs["n_contrib"] > 8).sum()) <= rep["valid"]
    assert rep["fallback"] == q - rep["valid"] >= 16 and rep["labelled"] == rep["valid"]
    feats = regions.synthetic_regions(gauss[0])[0].to(dev)
    near = gsbp_amd.spatial_knn(gauss[0], 1, queries=pts[~sf["valid"].to(dev)].contiguous())[1][:, 0].long()
    assert torch.equal(sf["features"][~sf["valid"]], feats[near].cpu())  # the fallback filled the points where nothing counts
    assert 0.0 <= rep["beyond_radius"] <= 0.011 and rep["beyond_radius"] == want.beyond_radius
    qs = rep["n_contrib_quantiles"]
    assert list(qs.values()) == sorted(qs.values()) and qs["0.0"] == 0 and qs["1.0"] == int(pgs["n_contrib"].max())
    ws = rep["wsum_quantiles"]
    assert list(ws.values()) == sorted(ws.values()) and ws["0.0"] >= sample.ALPHA_MIN
    grid = rep["grid"]
    assert grid["cells"] == grid["dims"][0] * grid["dims"][1] * grid["dims"][2] and grid["points_in_cells"] == n
    met = json.load(open(out / "metrics.json"))
    counts = torch.tensor(met["counts"])
    assert counts.shape == (6, 3) and int(counts[:, 2].sum()) == q and int(counts[:, 1].sum()) == rep["valid"]
    assert 0.0 <= met["miou"] <= 1.0
