"""run_transfer.py --synthetic: the file's labels and counts equal transfer_labels on the same seeded inputs."""
import os
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import transfer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_labels_equal_the_api(dev, tmp_path):
    out = tmp_path / "labels.pt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_transfer.py"), "--synthetic", "--k", "5", "--counts", "--out", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = torch.load(out)
    q, s, labels = transfer.synthetic_transfer()
    lab, cnt = gsbp_amd.transfer_labels(q.to(dev), s.to(dev), labels, k=5, return_counts=True)
    assert set(got) == {"labels", "counts", "k", "num_classes"} and got["k"] == 5 and got["num_classes"] == int(labels.max()) + 1
    assert torch.equal(got["labels"], lab.cpu()) and torch.equal(got["counts"], cnt.cpu())
    assert int((lab >= 0).sum()) == q.shape[0] and int(cnt.sum()) == 5 * q.shape[0]


def test_cli_reads_example_files(dev, tmp_path):
    q, s, labels = transfer.synthetic_transfer(n=500, m=64, d=24)
    torch.save(q, tmp_path / "features.pt")
    torch.save({"features": s, "labels": labels.double().reshape(-1, 1)}, tmp_path / "examples.pt")
    out = tmp_path / "sub" / "labels.pt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_transfer.py"), "--features", str(tmp_path / "features.pt"),
                        "--examples", str(tmp_path / "examples.pt"), "--k", "3", "--out", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = torch.load(out)
    assert set(got) == {"labels", "k", "num_classes"}
    assert torch.equal(got["labels"], gsbp_amd.transfer_labels(q.to(dev), s.to(dev), labels, k=3).cpu())
