"""No-GPU checks of integer label maps (gwbp_scatter_labels, Engine.scatter_labels, create_label_field, the CLI's --label-maps):
the C ABI and its argument validation, the int64 narrowing, the CLI flags and the file loader."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

from gsbp_amd import _lib, narrow_labels
from gsbp_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scatter_labels_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gwbp.h")).read()
    for name, val in (("GWBP_LABEL_U8", 0), ("GWBP_LABEL_I16", 1), ("GWBP_LABEL_I32", 2)):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    assert "GWBP_API int gwbp_scatter_labels(" in hdr
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "gwbp_scatter_labels" in exported and "gwbp_scatter_labels" in _lib.EXPORTS
    assert (_lib.LABEL_U8, _lib.LABEL_I16, _lib.LABEL_I32) == (0, 1, 2)


def _call(label_type=_lib.LABEL_I32, K=4, ldf=4, F=True, ymap=False, xmap=False):
    """gwbp_scatter_labels with NULL caps, workspace and view: only the label arguments can be looked at before the caps."""
    buf = (C.c_char * 64)()
    fake = C.c_void_p(C.addressof(buf))
    return _lib.lib().gwbp_scatter_labels(None, None, 0, None, fake, label_type, 1, 1, K, fake if ymap else None,
                                          fake if xmap else None, 1.0, 1.0, fake if F else None, ldf, None, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(label_type=3), b"unknown label type"),
    (dict(label_type=-1), b"unknown label type"),
    (dict(K=0, ldf=0), b"num_classes must be positive"),
    (dict(K=-2), b"num_classes must be positive"),
    (dict(K=8, ldf=7), b"ldf"),
    (dict(F=False), b"null F"),
    (dict(ymap=True), b"both index maps or neither"),
    (dict(xmap=True), b"both index maps or neither"),
])
def test_label_arguments_are_einval_before_any_device_call(kw, msg):
    assert _call(**kw) == -1  # GWBP_EINVAL
    assert msg in _lib.lib().gwbp_last_error_string()


def test_valid_label_arguments_reach_the_caps_check():
    """With every label argument valid the call goes on to the caps -- NULL here, so EINVAL from make_layout, not from the
    label checks."""
    assert _call(ymap=True, xmap=True) == -1
    assert b"null caps" in _lib.lib().gwbp_last_error_string()


def test_int64_narrowing_ignores_out_of_range_ids():
    K = 7
    L = torch.tensor([[-5, K, 2 ** 40, 2 ** 40 + 3], [0, 3, K - 1, 2 ** 32 + 1]], dtype=torch.int64)
    n = narrow_labels(L, K)
    assert n.dtype == torch.int32
    assert n.tolist() == [[-1, -1, -1, -1], [0, 3, K - 1, -1]]
    every = torch.arange(K, dtype=torch.int64)
    assert torch.equal(narrow_labels(every, K), every.to(torch.int32))


def _parser():
    sys.path.insert(0, ROOT)
    import run_backproject
    return run_backproject


def test_cli_label_flags_parse_and_exclude_feature_maps():
    rb = _parser()
    p = rb.build_parser()
    a = p.parse_args(["--label-maps", "masks", "--num-classes", "5"])
    assert a.label_maps == "masks" and a.num_classes == 5 and a.feature_maps is None
    a = p.parse_args(["--synthetic", "C1", "--num-classes", "8"])
    assert a.synthetic == "C1" and a.num_classes == 8 and a.label_maps is None
    assert p.parse_args([]).label_maps is None and p.parse_args([]).num_classes is None
    with pytest.raises(SystemExit):
        p.parse_args(["--label-maps", "masks", "--feature-maps", "feats", "--num-classes", "5"])
    with pytest.raises(SystemExit):  # --label-maps without --num-classes: refused before anything touches the device
        rb.main(["--label-maps", "masks"])


def test_cli_label_loader_reads_integer_maps_and_rejects_float(tmp_path):
    rb = _parser()
    lab = torch.randint(-1, 9, (6, 10), dtype=torch.int16)
    torch.save(lab, tmp_path / "IMG_0001.JPG.pt")
    got = rb.load_label_map(str(tmp_path), "IMG_0001.JPG")
    assert got.dtype == torch.int16 and torch.equal(got, lab)
    torch.save(torch.rand(6, 10), tmp_path / "IMG_0002.JPG.pt")
    with pytest.raises(SystemExit, match="integer"):
        rb.load_label_map(str(tmp_path), "IMG_0002.JPG")
    torch.save(torch.zeros(6, 10, 3, dtype=torch.int32), tmp_path / "IMG_0003.JPG.pt")
    with pytest.raises(SystemExit, match="2-D"):
        rb.load_label_map(str(tmp_path), "IMG_0003.JPG")


def test_synthetic_label_maps_are_seeded_piecewise_constant():
    cfg = syn.CONFIGS["C1"]
    a, b = syn.make_label_map(cfg, 0, 8), syn.make_label_map(cfg, 0, 8)
    assert a.dtype == torch.int32 and tuple(a.shape) == (cfg.height, cfg.width) and torch.equal(a, b)
    assert int(a.min()) >= 0 and int(a.max()) < 8
    assert not torch.equal(a, syn.make_label_map(cfg, 1, 8))
    # Voronoi cells: neighbouring pixels mostly agree; the per-pixel map does not
    same = float((a[:, 1:] == a[:, :-1]).float().mean())
    r = syn.make_label_map(cfg, 0, 1000, per_pixel=True)
    assert same > 0.95 and float((r[:, 1:] == r[:, :-1]).float().mean()) < 0.01
    assert tuple(syn.make_label_map(cfg, 0, 3, size=(30, 40)).shape) == (30, 40)
