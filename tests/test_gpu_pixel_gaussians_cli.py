"""run_pick.py --synthetic in a fresh child process: the documented files exist with their shapes, and they equal the library calls."""
import argparse
import json
import os
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import cli

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_picks_the_gaussians_under_a_click(dev, tmp_path):
    out = tmp_path / "pick"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_pick.py"), "--synthetic", "C1", "--click", "0:200,150", "--k", "4",
                        "--id-maps", "--median-depth", "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    scene = cli.load_scene(argparse.Namespace(synthetic="C1"), dev)  # (activated on the device, as the command line does)
    n_views = scene.viewmats.shape[0]
    assert set(os.listdir(out)) == ({"picked.pt", "pick.json"} | {f"id_map_{v:04d}.pt" for v in range(n_views)}
                                    | {f"median_depth_{v:04d}.pt" for v in range(n_views)})
    cam = (scene.K, scene.width, scene.height)
    picked = torch.load(out / "picked.pt")
    want = gsbp_amd.pick_gaussians(*scene.gauss, scene.viewmats[0], *cam, xy=[[200, 150]], k=4)
    assert want.numel() > 0 and picked["ids"].dtype == torch.int64 and torch.equal(picked["ids"], want.cpu())
    assert picked["clicks"].tolist() == [[0, 200, 150]]
    pg = gsbp_amd.pixel_gaussians(*scene.gauss, scene.viewmats[0], *cam, k=4, xy=[[200, 150]])
    for name in pg._fields:
        assert torch.equal(picked["lists"][name], getattr(pg, name).cpu()), name
    assert picked["lists"]["ids"].shape == (1, 4)
    rep = json.load(open(out / "pick.json"))
    assert rep["n"] == scene.gauss[0].shape[0] and rep["k"] == 4 and rep["clicks"] == [[0, 200, 150]]
    assert rep["picked"] == want.numel() and rep["heaviest"] == want[:10].tolist()
    for v in (0, n_views - 1):
        full = gsbp_amd.pixel_gaussians(*scene.gauss, scene.viewmats[v], *cam, k=1)
        id_map, depth = torch.load(out / f"id_map_{v:04d}.pt"), torch.load(out / f"median_depth_{v:04d}.pt")
        assert id_map.shape == depth.shape == (scene.height, scene.width) and id_map.dtype == torch.int32
        assert torch.equal(id_map, full.ids[..., 0].cpu()) and torch.equal(depth, full.median_depth.cpu())
