"""run_fit_field.py --synthetic C1 --steps 4 --score in a fresh process: decoded_field.pt, history.json and fidelity.json are
written, and the history is finite."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_writes_the_field_its_history_and_both_scores(dev, tmp_path):
    out = tmp_path / "fit"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_fit_field.py"), "--synthetic", "C1", "--steps", "4", "--score",
                        "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    cfg = syn.CONFIGS["C1"]
    field = torch.load(out / "decoded_field.pt")
    assert set(field) == {"features", "conv"}
    assert field["features"].shape == (cfg.n_gaussians, 128) and field["conv"].shape == (128, cfg.feat_dim)
    assert bool(torch.isfinite(field["features"]).all()) and bool(torch.isfinite(field["conv"]).all())
    hist = json.load(open(out / "history.json"))
    assert hist["steps"] == 4 and len(hist["history"]) == 4 and all(math.isfinite(x) and x > 0 for x in hist["history"])
    assert hist["D"] == cfg.feat_dim and len(hist["views"]) == cfg.n_views
    rep = json.load(open(out / "fidelity.json"))
    assert set(rep) == {"decoded", "lifted"}
    for k in rep:
        assert rep[k]["views_scored"] == cfg.n_views and set(rep[k]["overall"]) == {"cosine", "mae", "mse", "relative"}
