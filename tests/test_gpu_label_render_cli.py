"""run_evaluate.py --synthetic C1 --num-classes 8 in a fresh process: every output is written and metrics.json is
miou_recall(counts.pt)."""
import glob
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


def test_cli_writes_counts_metrics_and_frames(dev, tmp_path):
    out = tmp_path / "eval"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_evaluate.py"), "--synthetic", "C1", "--num-classes", "8",
                        "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    cfg = syn.CONFIGS["C1"]
    counts = torch.load(out / "counts.pt")
    assert counts.shape == (cfg.n_views, 8, 3) and counts.dtype == torch.int64
    assert bool((counts[..., 2].sum(dim=1) == cfg.width * cfg.height).all())   # every pixel of a synthetic map has a class
    assert int(counts[..., 0].sum()) > 0 and bool((counts[..., 0] <= counts[..., 1]).all())
    labels = torch.load(out / "labels.pt")
    assert labels.shape == (cfg.n_gaussians,) and 0 <= int(labels.min()) and int(labels.max()) < 8
    metrics = json.load(open(out / "metrics.json"))
    want = gsbp_amd.miou_recall(counts)
    assert metrics["miou"] == pytest.approx(want["miou"], rel=1e-12) and metrics["mean_recall"] == pytest.approx(want["mean_recall"], rel=1e-12)
    assert metrics["n_present"] == want["n_present"] == 7 and metrics["num_classes"] == 8 and metrics["scored_views"] == cfg.n_views
    assert {int(i): x for i, x in metrics["iou"].items()} == pytest.approx(want["iou"])
    assert {int(i): x for i, x in metrics["recall"].items()} == pytest.approx(want["recall"])
    for sub in ("argmax", "tinted"):
        pngs = sorted(glob.glob(str(out / sub / "frame_*.png")))
        if pngs:
            from PIL import Image
            assert len(pngs) == cfg.n_views and Image.open(pngs[0]).size == (cfg.width, cfg.height)
        else:
            frames = torch.load(out / sub / "frames.pt")
            assert frames.shape == (cfg.n_views, cfg.height, cfg.width, 3) and frames.dtype == torch.uint8
