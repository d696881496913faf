"""The camera models / antialiased mode against captures of REAL gsplat 1.4.0 (tools/capture_gsplat_fixture.py CAMERA_CASES:
fisheye, ortho and pinhole + antialiased on T1), when they have been committed as tests/golden/gsplat_camera_*.npz; skipped
otherwise.  Until then the projection variants are pinned by the float64 restatement (tests/test_gpu_camera_models.py) only."""
import os

import numpy as np
import pytest
import torch

from util import capture_report, capture_tool

import gsbp_amd
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cases():
    return capture_tool().CAMERA_CASES


@pytest.mark.parametrize("fname,cfgname,model,mode", _cases(), ids=[c[0] for c in _cases()])
def test_hip_camera_models_against_gsplat_capture(dev, fname, cfgname, model, mode):
    """Same bar as tests/test_gpu_parity.py::test_hip_against_gsplat_capture: 99 % of the rows within 1e-4, at most 0.2 %
    threshold rows beyond it; and, under antialiased, the compensations of view 0."""
    path = os.path.join(GOLD, fname)
    if not os.path.exists(path):
        pytest.skip(f"{fname} not captured yet (needs CUDA + gsplat==1.4.0)")
    cap = dict(np.load(path))
    cfg = syn.CONFIGS[cfgname]
    g = capture_tool().case_inputs(cfgname)
    W, H = cfg.width, cfg.height
    t = {k: torch.from_numpy(np.asarray(g[k])).to(dev) for k in ("means", "quats", "scales", "opac", "K", "vms")}
    feats = [torch.from_numpy(f) for f in g["feats"]]
    cam = dict(camera_model=model, rasterize_mode=mode)
    out, F, d, _ = gsbp_amd.create_feature_field(t["means"], t["quats"], t["scales"], t["opac"], t["vms"], t["K"], W, H,
                                                  lambda v: feats[v].to(dev), feats[0].shape[-1], return_partials=True, **cam)
    eng = gsbp_amd.Engine(t["means"].shape[0], W, H, device=dev)
    proj = eng.project(eng.view(t["vms"][0].cpu(), t["K"].cpu(), W, H, **cam), t["means"], t["quats"], t["scales"], t["opac"],
                       want_outputs=True)
    rep = capture_report(cap, out.cpu().numpy(), F.cpu().numpy(), d.cpu().numpy(),
                         *[proj[k].cpu().numpy() for k in ("radii", "means2d", "conics", "depths")])
    print("HIP vs gsplat capture", fname, rep)
    for k in ("F", "d", "out"):
        assert rep[k]["p99"] <= 1e-4, (k, rep[k])
        assert rep[k]["rows_over_1e-4"] <= max(1, int(0.002 * rep[k]["rows"])) and rep[k]["max"] <= 1e-2, (k, rep[k])
    if mode == "antialiased" and "v0_compensations" in cap:
        theirs = np.asarray(cap["v0_compensations"]).reshape(-1)
        mine = proj["compensations"].cpu().numpy()
        ids = cap["v0_gaussian_ids"] if "v0_gaussian_ids" in cap else np.arange(mine.shape[0])
        assert np.abs(mine[ids] - theirs).max() <= 1e-5
