"""run_pca.py --synthetic C1 in both modes: the three outputs are written and the saved colours equal pca_colors of the saved field."""
import glob
import os
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import pca
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", ["gaussians", "renderings"])
def test_cli_writes_basis_colours_and_frames(dev, tmp_path, mode):
    out = tmp_path / mode
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_pca.py"), "--synthetic", "C1", "--mode", mode, "--out", str(out)],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    cfg = syn.CONFIGS["C1"]
    field = torch.load(out / "features.pt")
    saved = torch.load(out / "pca_colors.pt")
    basis = pca.PCABasis.from_state_dict(torch.load(out / "pca_basis.pt"), device=dev)
    assert field.shape == (cfg.n_gaussians, cfg.feat_dim) and basis.components.shape == (3, cfg.feat_dim)
    assert basis.n_samples == cfg.n_gaussians and float(basis.explained_variance_ratio.sum()) <= 1.0 + 1e-12
    colors, lo, hi = gsbp_amd.pca_colors(field.to(dev))
    assert torch.equal(saved["colors"], colors.cpu()) and saved["lo"] == float(lo) and saved["hi"] == float(hi)
    refit = gsbp_amd.fit_pca(field.to(dev))
    assert torch.equal(refit.components, basis.components) and torch.equal(refit.mean, basis.mean)
    pngs = sorted(glob.glob(str(out / "frame_*.png")))
    if pngs:
        from PIL import Image
        assert len(pngs) == cfg.n_views
        want = next(gsbp_amd.render_pca(*_scene(cfg, dev), field.to(dev), *_cameras(cfg, dev), cfg.width, cfg.height, mode=mode,
                                        basis=basis, scale=0.2 if mode == "gaussians" else 1.0))
        import numpy as np
        assert np.array_equal(np.asarray(Image.open(pngs[0])), want.cpu().numpy())
    else:
        frames = torch.load(out / "frames.pt")
        assert frames.shape == (cfg.n_views, cfg.height, cfg.width, 3) and frames.dtype == torch.uint8


def _scene(cfg, dev):
    return tuple(t.to(dev) for t in syn.activate(syn.make_scene(cfg)))


def _cameras(cfg, dev):
    return syn.make_cameras(cfg).to(dev), syn.intrinsics(cfg).to(dev)
