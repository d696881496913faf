"""run_cluster.py --synthetic: its four kinds of output exist, the codes are codes, the report matches the fit, and a second run writes
the same bits."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_cli(out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_cluster.py"), "--synthetic", "C1", "--k", "8", "--iters", "5",
                        "--smooth-k", "4", "--frames", "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def test_cli_clusters_the_seeded_field_twice_alike(dev, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    run_cli(a)
    assert {"codebook.pt", "codes.pt", "cluster.json", "frames"} <= set(os.listdir(a))
    frames = os.listdir(a / "frames")
    assert frames == ["frames.pt"] or sorted(frames) == [f"frame_{v:04d}.png" for v in range(4)]
    book, codes = torch.load(a / "codebook.pt"), torch.load(a / "codes.pt")
    assert book.shape == (8, 64) and book.dtype == torch.float32 and codes.shape == (10000,) and codes.dtype == torch.int32
    assert int(codes.min()) >= -1 and int(codes.max()) < 8
    rep = json.load(open(a / "cluster.json"))
    assert rep["k"] == 8 and rep["n"] == 10000 and 1 <= rep["n_iter"] <= 5 and len(rep["history"]) == rep["n_iter"]
    assert len(rep["counts"]) == 8 and sum(rep["counts"]) + rep["unassigned"] == 10000 and rep["reseeds"] >= 0
    assert rep["smooth_k"] == 4 and 0.5 < rep["mean_cosine"] <= 1.0 + 1e-6 and rep["inertia"] == rep["history"][-1]
    run_cli(b)
    assert torch.equal(torch.load(b / "codes.pt"), codes) and torch.equal(torch.load(b / "codebook.pt"), book)
    assert json.load(open(b / "cluster.json")) == rep
