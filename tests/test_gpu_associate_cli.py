"""run_associate.py on the GPU: the files it writes, and its renamed maps fed to the existing label lift."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import associate_ref as ref

import gsbp_amd
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_associate_synthetic_writes_maps_the_label_lift_reads(tmp_path, dev):
    """--synthetic C1: association.pt, maps/<name>.pt, associate.json, votes.pt and frames.  create_label_field on the renamed maps
    gives a field whose row argmax is `groups` wherever the votes have a maximum clear of both kernels' rounding
    (associate_ref.clear_maximum)."""
    out = str(tmp_path / "assoc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_associate.py"), "--synthetic", "C1", "--save-votes", "--frames",
                        "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cfg = syn.CONFIGS["C1"]
    names = [f"view_{v:04d}" for v in range(cfg.n_views)]
    a = torch.load(os.path.join(out, "association.pt"))
    votes = torch.load(os.path.join(out, "votes.pt"))
    with open(os.path.join(out, "associate.json")) as f:
        rep = json.load(f)
    n_groups = a["n_groups"]
    assert a["maps"].shape == (cfg.n_views, 6) and a["maps"].dtype == torch.int32 and a["groups"].shape == (cfg.n_gaussians,)
    assert votes.shape == (cfg.n_gaussians, 256) and votes.dtype == torch.int64 and 1 <= n_groups <= 256
    assert rep["n_groups"] == n_groups and len(rep["per_view"]) == cfg.n_views and sum(rep["group_sizes"]) == rep["grouped"]
    assert rep["per_view"][0]["opened"] >= 1 and rep["iou_min"] == 0.2 and rep["min_mass"] == 1.0
    assert os.path.exists(os.path.join(out, "frames", "frame_0000.png")) or os.path.exists(os.path.join(out, "frames", "frames.pt"))
    maps = [torch.load(os.path.join(out, "maps", nm + ".pt")) for nm in names]
    assert all(m.shape == (cfg.height, cfg.width) and m.dtype == torch.int32 and int(m.max()) < n_groups for m in maps)
    assert torch.equal(gsbp_amd.associate.group_of_votes(votes), a["groups"])

    gauss = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    K, vms = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg).to(dev)
    P = gsbp_amd.create_label_field(*gauss, vms, K, cfg.width, cfg.height, lambda v: maps[v].to(dev), n_groups, pipeline=False)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    n_entries = np.zeros(cfg.n_gaussians, np.int64)
    for v in range(cfg.n_views):
        view = eng.view(vms[v], K, cfg.width, cfg.height)
        eng.project(view, *gauss)
        eng.bin_sort(view)
        eng.blend_weights(view)
        n_entries += np.bincount(eng.dump_pairs(view)[0].cpu().numpy(), minlength=cfg.n_gaussians)
    clear = torch.from_numpy(ref.clear_maximum(votes.numpy(), n_entries))
    assert int(clear.sum()) > 0.5 * int((a["groups"] >= 0).sum()) > 0
    assert torch.equal(P.argmax(dim=1).cpu()[clear].int(), a["groups"][clear])
