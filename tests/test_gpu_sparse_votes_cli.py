"""run_associate.py --votes sparse and run_backproject.py --sparse-slots on the GPU: the files they write."""
import json
import os
import subprocess
import sys

import pytest
import torch

from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_associate_sparse_writes_the_lists_and_their_stats(tmp_path, dev):
    """--synthetic C1 --votes sparse at the default 8 slots: association.pt carries the canonical lists, associate.json their
    stats, and no row overflows (the assert prints the count if one does: the default is not to be raised silently)."""
    out = str(tmp_path / "assoc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_associate.py"), "--synthetic", "C1", "--votes", "sparse",
                        "--max-groups", "65536", "--save-votes", "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cfg = syn.CONFIGS["C1"]
    a = torch.load(os.path.join(out, "association.pt"))
    with open(os.path.join(out, "associate.json")) as f:
        rep = json.load(f)
    n, n_groups = cfg.n_gaussians, a["n_groups"]
    assert a["keys"].shape == (n, 8) and a["keys"].dtype == torch.int32 and a["vals"].shape == (n, 8) and a["vals"].dtype == torch.int64
    assert a["spill"].shape == (n,) and a["certain"].shape == (n,) and a["groups"].shape == (n,) and 1 <= n_groups
    assert int(a["keys"].max()) < n_groups and bool(((a["keys"] >= 0) == (a["vals"] > 0)).all())
    st = rep["sparse_votes"]
    assert rep["votes"] == "sparse" and st["rows"] == n and st["slots"] == 8 and sum(st["slots_in_use"]) == n
    assert [v["overflow_rows"] for v in rep["per_view"]][-1] == st["overflow_rows"]
    assert st["overflow_rows"] == 0, f"{st['overflow_rows']} of {n} Gaussians overflow 8 slots on C1: {st}"
    assert bool(a["certain"].all()) and int(a["spill"].sum()) == 0
    # canonical order: the first slot is the argmax, which is the Gaussian's group
    first = torch.where(a["vals"][:, 0] > 0, a["keys"][:, 0], -1)
    assert torch.equal(first, a["groups"])
    votes = torch.load(os.path.join(out, "votes.pt"))
    assert votes.shape == (n, n_groups) and torch.equal(votes.sum(dim=1), a["vals"].sum(dim=1))


def test_run_backproject_sparse_slots_writes_the_field(tmp_path, dev):
    out = str(tmp_path / "field")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_backproject.py"), "--synthetic", "C1", "--num-classes", "1000",
                        "--sparse-slots", "8", "--no-prune", "--results-dir", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cfg = syn.CONFIGS["C1"]
    f = torch.load(os.path.join(out, "sparse_label_field.pt"))
    n = cfg.n_gaussians
    assert f["ids"].shape == (n, 8) and f["ids"].dtype == torch.int32 and f["fractions"].shape == (n, 8)
    assert f["fractions"].dtype == torch.float32 and f["spill_fraction"].shape == (n,) and f["total"].dtype == torch.int64
    assert f["num_classes"] == 1000 and f["slots"] == 8 and -1 <= int(f["ids"].min()) and int(f["ids"].max()) < 1000
    assert bool((f["fractions"][:, :-1] >= f["fractions"][:, 1:]).all())  # largest share first
    rows = f["fractions"].sum(dim=1) + f["spill_fraction"]
    assert float(rows.max()) <= 1.0 + 1e-6 and float(rows[f["total"] > 0].min()) > 0.99  # every synthetic pixel has a class
    assert f["stats"]["overflow_rows"] == int((f["spill_fraction"] > 0).sum())
    assert not os.path.exists(os.path.join(out, "label_field.pt"))
