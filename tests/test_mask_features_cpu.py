"""No-GPU checks of mask-pooled features (gwbp_scatter_mask_features, create_mask_feature_field, the CLI's --mask-features): the
C ABI and its argument validation, the synthetic generator, the CLI flags and the file loader."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib
from gsbp_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scatter_mask_features_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "gwbp.h")).read()
    assert re.search(r"#define GWBP_MASK_SLOT_BYTES 32\b", hdr)
    assert "GWBP_API int gwbp_scatter_mask_features(" in hdr
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "gwbp_scatter_mask_features" in exported and "gwbp_scatter_mask_features" in _lib.EXPORTS
    assert _lib.MASK_SLOT_BYTES == 32
    assert callable(gsbp_amd.create_mask_feature_field)


def test_header_is_c99_clean(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "gwbp.h"\nint main(void) { return (int)sizeof(&gwbp_scatter_mask_features); }\n')
    r = subprocess.run(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _call(label_type=_lib.LABEL_I32, table_type=_lib.MAP_F32, M=4, D=8, ts_row=8, F=True, ymap=False, xmap=False, table=True,
          labels=True, slots=True, slots_bytes=1 << 20, caps=None, misalign=0):
    """gwbp_scatter_mask_features with a NULL workspace and view: only the map, table and slot arguments (and the caps, for the
    slot size) can be looked at before the workspace."""
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 255) & ~255
    fake = C.c_void_p(base)
    tab = C.c_void_p(base + misalign) if table else None
    return _lib.lib().gwbp_scatter_mask_features(
        C.byref(caps) if caps is not None else None, None, 0, None, fake if labels else None, label_type, 1, 1,
        fake if ymap else None, fake if xmap else None, tab, table_type, ts_row, M, D, 1.0, 1.0, fake if F else None, None,
        fake if slots else None, slots_bytes, None, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(label_type=3), b"unknown label type"),
    (dict(table_type=3), b"unknown table type"),
    (dict(M=0), b"num_masks must be positive"),
    (dict(D=6, ts_row=8), b"multiple of 4"),
    (dict(D=0), b"multiple of 4"),
    (dict(labels=False), b"bad label map"),
    (dict(ymap=True), b"both index maps or neither"),
    (dict(xmap=True), b"both index maps or neither"),
    (dict(table=False), b"table rows"),
    (dict(ts_row=4), b"table rows"),
    (dict(ts_row=10), b"table rows"),
    (dict(misalign=8), b"table rows"),
    (dict(F=False), b"F must be"),
    (dict(slots=False), b"slots"),
])
def test_mask_arguments_are_einval_before_any_device_call(kw, msg):
    assert _call(**kw) == -1  # GWBP_EINVAL
    assert msg in _lib.lib().gwbp_last_error_string()


def test_half_table_needs_8_byte_alignment_only():
    """An fp16 table 8 B off a 16-B boundary passes the table check and goes on to the caps (NULL here)."""
    assert _call(table_type=_lib.MAP_F16, misalign=8) == -1
    assert b"null caps" in _lib.lib().gwbp_last_error_string()


def test_short_slot_store_is_einval():
    caps = _lib.Caps(1000, 5000, 1 << 16, 64, 64, 0, 0)
    assert _call(caps=caps, slots_bytes=32 * 5000 - 1) == -1
    assert b"slots" in _lib.lib().gwbp_last_error_string()
    assert _call(caps=caps, slots_bytes=32 * 5000) == -1  # long enough: on to the workspace (NULL)
    assert b"null workspace" in _lib.lib().gwbp_last_error_string()


def test_make_mask_features_is_seeded_voronoi():
    cfg = syn.CONFIGS["T1"]
    L, t = syn.make_mask_features(cfg, 1, 30, 20)
    L2, t2 = syn.make_mask_features(cfg, 1, 30, 20)
    assert torch.equal(L, L2) and torch.equal(t, t2)
    assert L.shape == (cfg.height, cfg.width) and L.dtype == torch.int32
    assert t.shape == (30, 20) and t.dtype == torch.float32
    assert int(L.min()) >= 0 and int(L.max()) < 30
    assert torch.allclose(t.norm(dim=1), torch.ones(30), atol=1e-5)
    # piecewise constant: most horizontal neighbours share their mask
    assert float((L[:, 1:] == L[:, :-1]).float().mean()) > 0.9
    assert torch.equal(L, syn.make_label_map(cfg, 1, 30, n_seeds=30))
    L3, t3 = syn.make_mask_features(cfg, 2, 30, 20)
    assert not torch.equal(t, t3)
    Lp, _ = syn.make_mask_features(cfg, 1, 30, 20, per_pixel=True)
    assert float((Lp[:, 1:] == Lp[:, :-1]).float().mean()) < 0.2
    Ll, _ = syn.make_mask_features(cfg, 1, 30, 20, size=(9, 13))
    assert Ll.shape == (9, 13)


def _parser():
    sys.path.insert(0, ROOT)
    try:
        import run_backproject
    finally:
        sys.path.remove(ROOT)
    return run_backproject


def test_cli_parser_takes_mask_features():
    rb = _parser()
    a = rb.build_parser().parse_args(["--synthetic", "C1", "--mask-features", "synthetic"])
    assert a.mask_features == "synthetic" and a.num_masks == 200
    a = rb.build_parser().parse_args(["--mask-features", "/some/dir", "--num-masks", "12"])
    assert a.mask_features == "/some/dir" and a.num_masks == 12
    for bad in (["--mask-features", "x", "--feature-maps", "y"], ["--mask-features", "x", "--label-maps", "y"]):
        with pytest.raises(SystemExit):
            rb.build_parser().parse_args(bad)


@pytest.mark.parametrize("argv", [
    ["--synthetic", "C1", "--mask-features", "synthetic", "--num-classes", "4"],
    ["--synthetic", "C1", "--mask-features", "somewhere"],
    ["--synthetic", "C1", "--mask-features", "synthetic", "--num-masks", "0"],
    ["--mask-features", "x", "--encoder", "e.pt"],
])
def test_cli_rejects_bad_mask_combinations(argv):
    with pytest.raises(SystemExit):
        _parser().main(argv)


def test_mask_file_loader(tmp_path):
    rb = _parser()
    torch.save({"labels": torch.zeros(4, 5, dtype=torch.int64), "table": torch.ones(3, 8, dtype=torch.float16)}, tmp_path / "a.png.pt")
    lab, tab = rb.load_mask_features(str(tmp_path), "a.png")
    assert lab.shape == (4, 5) and tab.dtype == torch.float16
    for bad in ({"labels": torch.zeros(4, 5), "table": torch.ones(3, 8)}, {"labels": torch.zeros(4, 5, dtype=torch.int32)},
                {"labels": torch.zeros(4, 5, dtype=torch.int32), "table": torch.ones(3, 8, dtype=torch.float64)},
                torch.zeros(4, 5, dtype=torch.int32)):
        torch.save(bad, tmp_path / "b.png.pt")
        with pytest.raises(SystemExit):
            rb.load_mask_features(str(tmp_path), "b.png")


def test_field_argument_checks_need_no_device():
    cfg = syn.CONFIGS["T0"]
    args = (torch.zeros(4, 3), torch.zeros(4, 4), torch.zeros(4, 3), torch.zeros(4), torch.zeros(1, 4, 4), torch.eye(3),
            cfg.width, cfg.height, lambda v: None, 8)
    with pytest.raises(ValueError):
        gsbp_amd.create_mask_feature_field(*args, upsample="bilinear")
    with pytest.raises(ValueError):
        gsbp_amd.create_mask_feature_field(*args, reduction="max")
    with pytest.raises(ValueError):
        gsbp_amd.create_mask_feature_field(*args[:-1], 0)
