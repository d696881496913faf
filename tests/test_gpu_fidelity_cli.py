"""run_fidelity.py --synthetic C1 in a fresh process: table.pt, fidelity.json and one weight map per view are written, and
fidelity.json is field_fidelity(table.pt)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_writes_table_report_and_weight_maps(dev, tmp_path):
    out, weights = tmp_path / "fidelity", tmp_path / "weights"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_fidelity.py"), "--synthetic", "C1", "--out", str(out),
                        "--weights-out", str(weights), "--cosine-min", "0.1"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    cfg = syn.CONFIGS["C1"]
    table = torch.load(out / "table.pt")
    assert table.shape == (cfg.n_views, 8) and table.dtype == torch.float64
    assert bool((table[:, 6] == cfg.width * cfg.height).all()) and bool((table[:, 7] == cfg.feat_dim).all())
    assert bool((table[:, 4] > 0).all()) and bool((table[:, 5] == 0).all()) and bool((table[:, 4] <= table[:, 6]).all())
    rep = json.load(open(out / "fidelity.json"))
    want = gsbp_amd.field_fidelity(table)
    assert rep["views_scored"] == cfg.n_views and rep["D"] == cfg.feat_dim and len(rep["views"]) == cfg.n_views
    for k in ("cosine", "mae", "mse", "relative"):
        assert rep["overall"][k] == pytest.approx(want["overall"][k], rel=1e-12)
        assert rep["per_view"][k] == pytest.approx(want["per_view"][k].tolist(), rel=1e-12)
    assert -1.0 <= rep["overall"]["cosine"] <= 1.0 and rep["overall"]["relative"] > 0
    for name in rep["views"]:   # named as run_backproject.py --pixel-weights reads them
        w = torch.load(weights / (name + ".pt"))
        assert w.dtype == torch.bool and w.shape == (cfg.height, cfg.width)
