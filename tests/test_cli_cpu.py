"""The command lines' shared half without a GPU (gsbp_amd.cli): every run_*.py parser against the options recorded before the
scene options were shared, and load_scene against the expressions the command lines used to spell out, on the committed COLMAP
fixture and on a synthetic config."""
import argparse
import importlib
import json
import os

import pytest
import torch

from gsbp_amd import cli, scene_io
from gsbp_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
SCRIPTS = ("run_backproject", "run_evaluate", "run_fidelity", "run_fit_field", "run_pca", "run_segment", "run_transfer")


def describe(ap):
    return [dict(option_strings=list(a.option_strings), dest=a.dest, default=a.default, choices=None if a.choices is None else list(a.choices),
                 type=getattr(a.type, "__name__", None), nargs=a.nargs, required=a.required, help=a.help) for a in ap._actions]


@pytest.mark.parametrize("script", SCRIPTS)
def test_parsers_declare_the_recorded_options(script):
    """tests/golden/cli_options.json: describe(build_parser()) of every script at the commit before add_scene_arguments existed."""
    with open(os.path.join(HERE, "golden", "cli_options.json")) as f:
        want = json.load(f)[script]
    got = json.loads(json.dumps(describe(importlib.import_module(script).build_parser())))
    assert [a["dest"] for a in got] == [a["dest"] for a in want]
    for a, b in zip(got, want):
        assert a == b, (script, a["dest"])


def test_scene_arguments_can_be_declared_in_parts():
    ap = argparse.ArgumentParser()
    cli.add_scene_arguments(ap, only=("synthetic",))
    cli.add_scene_arguments(ap, only=("max-views", "data-dir"), max_views_help="x")
    assert [a.dest for a in ap._actions[1:]] == ["synthetic", "data_dir", "max_views"] and ap._actions[-1].help == "x"
    with pytest.raises(ValueError, match="no scene options"):
        cli.add_scene_arguments(ap, only=("views",))


def _args(**kw):
    root = os.path.join(HERE, "golden", "colmap_sparse")
    return argparse.Namespace(**dict(dict(synthetic=None, checkpoint=os.path.join(root, "point_cloud.ply"), data_dir=root, format="ply",
                                          data_factor=2), **kw))


@pytest.mark.parametrize("on_host", [False, True])
def test_load_scene_of_a_checkpoint_is_what_the_command_lines_spelt_out(on_host):
    args = _args()
    scene = cli.load_scene(args, "cpu", activate_on_host=on_host)
    splats = scene_io.load_checkpoint(args.checkpoint, args.data_dir, format="ply", data_factor=2)
    K = splats["camera_matrix"].float()
    W, H = int(K[0, 2] * 2), int(K[1, 2] * 2)
    images = sorted(splats["colmap_project"].images.values(), key=lambda im: im.name)
    viewmats = torch.stack([scene_io.get_viewmat_from_colmap_image(im) for im in images])
    gauss = (splats["means"].float(), splats["rotation"].float(), torch.exp(splats["scaling"]).float(),
             torch.sigmoid(splats["opacity"]).float())
    assert torch.equal(scene.K, K) and (scene.width, scene.height) == (W, H) == (648, 420)
    assert scene.names == [im.name for im in images] and len(scene.names) > 1 and scene.names != [im.name for im in
                                                                                                    splats["colmap_project"].images.values()]
    assert torch.equal(scene.viewmats, viewmats) and scene.viewmats.shape == (len(images), 4, 4)
    assert len(scene.gauss) == 4 and all(torch.equal(a, b) and a.dtype == torch.float32 for a, b in zip(scene.gauss, gauss))
    assert scene.cfg is None and set(scene.splats) == set(splats)
    assert all(torch.equal(scene.splats[k], v) for k, v in splats.items() if torch.is_tensor(v))
    one = scene.first_views(1)
    assert torch.equal(one.viewmats, viewmats[:1]) and one.names == scene.names[:1] and one.gauss is scene.gauss
    assert scene.first_views(None) is scene


def test_load_scene_of_a_synthetic_config_is_the_generators_called_directly():
    cfg = syn.CONFIGS["C1"]
    scene = cli.load_scene(_args(synthetic="C1"), "cpu")
    raw = syn.make_scene(cfg)
    assert set(scene.splats) == set(raw) and all(torch.equal(scene.splats[k], raw[k]) for k in raw)
    assert all(torch.equal(a, b) and a.dtype == torch.float32 for a, b in zip(scene.gauss, syn.activate(raw)))
    assert torch.equal(scene.K, syn.intrinsics(cfg)) and torch.equal(scene.viewmats, syn.make_cameras(cfg))
    assert (scene.width, scene.height, scene.cfg) == (cfg.width, cfg.height, cfg)
    assert scene.names == [f"view_{v:04d}" for v in range(cfg.n_views)]
    one = scene.first_views(1)
    assert one.viewmats.shape == (1, 4, 4) and one.names == ["view_0000"]


def test_require_gpu_exits_with_the_programs_name(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match=r"run_x\.py needs a GPU \(there is no CPU path\)"):
        cli.require_gpu("run_x.py")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    cli.require_gpu("run_x.py")


def test_frame_writer_keeps_its_two_forms(tmp_path):
    w = cli.FrameWriter(str(tmp_path / "a"))
    w.add(3, torch.zeros(4, 5, 3, dtype=torch.uint8))
    w.close()
    assert os.path.exists(tmp_path / "a" / ("frame_0003.png" if w.image is not None else "frames.pt"))
