"""run_train.py's feature options without a GPU: what the parser leaves in the namespace, what it refuses, and how a view's feature
map is read."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import run_train  # noqa: E402

NEW = ("feature_dim", "latent_dim", "feature_weight", "feature_maps")


def test_options_that_are_not_given_leave_no_trace():
    args = vars(run_train.build_parser().parse_args(["--synthetic", "T0"]))
    assert not any(k in args for k in NEW)
    args = vars(run_train.build_parser().parse_args(["--synthetic", "T0", "--feature-dim", "32", "--latent-dim", "16",
                                                     "--feature-weight", "0.5", "--feature-maps", "maps"]))
    assert {k: args[k] for k in NEW} == dict(feature_dim=32, latent_dim=16, feature_weight=0.5, feature_maps="maps")


@pytest.mark.parametrize("argv", [["--synthetic", "T0", "--latent-dim", "16"], ["--synthetic", "T0", "--feature-weight", "2"],
                                  ["--synthetic", "T0", "--feature-dim", "32", "--feature-maps", "maps"],
                                  ["--colmap", "model", "--images", "images", "--feature-dim", "32"]])
def test_inconsistent_feature_options_are_refused_before_anything_runs(argv):
    with pytest.raises(SystemExit) as e:
        run_train.main(argv)
    assert e.value.code == 2


def test_a_feature_map_is_read_by_image_stem_and_upsampled_bilinearly(tmp_path):
    g = torch.Generator().manual_seed(1)
    full, low = torch.rand(6, 8, 4, generator=g), torch.rand(3, 4, 4, generator=g)
    np.save(tmp_path / "a.npy", full.numpy())
    torch.save(low, tmp_path / "b.pt")
    got = run_train.load_feature_map(str(tmp_path), "a.png", "cpu", 8, 6, 4)
    assert torch.equal(got, full) and got.is_contiguous()
    got = run_train.load_feature_map(str(tmp_path), "b.JPG", "cpu", 8, 6, 4)
    want = torch.nn.functional.interpolate(low.permute(2, 0, 1)[None], (6, 8), mode="bilinear")[0].permute(1, 2, 0)
    assert tuple(got.shape) == (6, 8, 4) and torch.equal(got, want) and got.is_contiguous()
    assert run_train.load_feature_map(str(tmp_path), "c.png", "cpu", 8, 6, 4) is None
    with pytest.raises(SystemExit, match="expected"):
        run_train.load_feature_map(str(tmp_path), "a.png", "cpu", 8, 6, 5)
