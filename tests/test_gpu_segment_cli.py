"""run_segment.py --synthetic C1 in a fresh process: every output is written and the saved 3-D mask equals prompt_mask called directly."""
import glob
import os
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import segment as seg
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_writes_masks_and_renders(dev, tmp_path):
    out = tmp_path / "seg"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_segment.py"), "--synthetic", "C1", "--click", "0:200,150", "--export",
                        "--out", str(out)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    cfg = syn.CONFIGS["C1"]
    field = torch.load(out / "features.pt")
    prompts, n_pos = seg.load_prompts(str(out / "prompts.pt"))
    assert field.shape == (cfg.n_gaussians, cfg.feat_dim) and prompts.shape == (4, cfg.feat_dim) and n_pos == 1
    mask = torch.load(out / "mask3d.pt")
    assert mask.dtype == torch.bool and mask.shape == (cfg.n_gaussians,)
    # the click of the command line, repeated here: one more positive prompt in front of the file's negatives
    gauss = tuple(t.to(dev) for t in syn.activate(syn.make_scene(cfg)))
    vec = gsbp_amd.probe_pixels(*gauss, field.to(dev), syn.make_cameras(cfg)[0].to(dev), syn.intrinsics(cfg).to(dev), cfg.width,
                                cfg.height, [[200, 150]])[0]
    full = torch.cat([prompts[:1].to(dev), vec, prompts[1:].to(dev)])
    assert torch.equal(mask, gsbp_amd.prompt_mask(field.to(dev), full, 2).cpu())
    assert 0 < int(mask.sum()) < cfg.n_gaussians
    for sub in ("mask2d", "extracted", "deleted"):
        pngs = sorted(glob.glob(str(out / sub / "frame_*.png")))
        if pngs:
            from PIL import Image
            assert len(pngs) == cfg.n_views and Image.open(pngs[0]).size == (cfg.width, cfg.height)
        else:
            frames = torch.load(out / sub / "frames.pt")
            assert frames.shape == (cfg.n_views, cfg.height, cfg.width, 3) and frames.dtype == torch.uint8
    for name, keep in (("extracted.pt", mask), ("deleted.pt", ~mask)):
        ck = torch.load(out / name)["splats"]
        assert ck["means"].shape == (int(keep.sum()), 3) and ck["quats"].shape == (int(keep.sum()), 4)
