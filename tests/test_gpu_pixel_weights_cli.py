"""run_backproject.py --pixel-weights: the CLI's field equals create_feature_field / create_label_field with the same maps."""
import os
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4  # the repository's tolerance: F is summed by atomics, the finalised rows of small norm amplify the order


def _cli(tmp, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_backproject.py"), "--synthetic", "C1", "--no-prune",
                        "--results-dir", str(tmp), *flags], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("kind", ["mask", "confidence"])
@pytest.mark.parametrize("labels", [False, True])
def test_cli_pixel_weights_equal_the_api(dev, tmp_path, kind, labels):
    cfg = syn.CONFIGS["C1"]
    flags = ["--pixel-weights", kind] + (["--num-classes", "6"] if labels else [])
    _cli(tmp_path, *flags)
    out = torch.load(tmp_path / ("label_field.pt" if labels else "features_lseg.pt"))
    means, quats, scales, opac = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    args = (means, quats, scales, opac, syn.make_cameras(cfg), syn.intrinsics(cfg), cfg.width, cfg.height)

    def pw(v):
        return syn.make_pixel_weights(cfg, v, device=dev, kind=kind)
    if labels:
        ref = gsbp_amd.create_label_field(*args, lambda v: syn.make_label_map(cfg, v, 6, device=dev), 6, pixel_weight_fn=pw)
    else:
        ref = gsbp_amd.create_feature_field(*args, lambda v: syn.make_feature_map(cfg, v, device=dev), cfg.feat_dim,
                                            pixel_weight_fn=pw)
        unweighted = gsbp_amd.create_feature_field(*args, lambda v: syn.make_feature_map(cfg, v, device=dev), cfg.feat_dim)
        assert float((ref - unweighted).abs().max()) > 1e-3  # the maps do change the field
    assert out.shape == ref.shape and float((out - ref.cpu()).abs().max()) <= TOL
