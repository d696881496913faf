"""run_backproject.py --votes: votes.pt equals create_vote_field on the same scene and label maps, count for count."""
import os
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("method", ["binary", "projection"])
def test_cli_votes_equal_the_api(dev, tmp_path, method):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_backproject.py"), "--synthetic", "C1", "--num-classes", "2",
                        "--votes", method, "--results-dir", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = torch.load(tmp_path / "votes.pt")
    assert out["method"] == method and set(out) == {"counts", "views", "method", "mask3d", "mask3d_inverted"}
    cfg = syn.CONFIGS["C1"]
    # the CLI's scene: the pre-activation parameters moved to the device, then activated there
    means, quats, scales, opac = syn.activate({k: v.to(dev) for k, v in syn.make_scene(cfg).items()})
    C, n = gsbp_amd.create_vote_field(means, quats, scales, opac, syn.make_cameras(cfg), syn.intrinsics(cfg), cfg.width,
                                      cfg.height, lambda v: syn.make_label_map(cfg, v, 2, device=dev), 2, method=method)
    assert torch.equal(out["counts"], C.cpu()) and torch.equal(out["views"], n.cpu()) and float(n.sum()) > 0
    m3, m3i = gsbp_amd.mask3d_from_votes(C)
    assert torch.equal(out["mask3d"], m3.cpu()) and torch.equal(out["mask3d_inverted"], m3i.cpu())
    assert bool(m3.any()) and bool(m3i.any())
