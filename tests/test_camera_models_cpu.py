"""No-GPU checks of the camera models / rasterize modes: the C ABI entry point and its argument validation, the float64
restatement the GPU tests compare with (tests/ref_camera_np.py), the COLMAP -> gsplat camera mapping, the CLI flags and the
drop-in's refusals."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib, scene_io
from ref_camera_np import compensation, fisheye_jacobian, fisheye_uv
from test_capi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_project_camera():
    import subprocess
    assert "gwbp_project_camera" in declared_symbols()
    gsbp_amd.build()
    assert getattr(_lib.lib(), "gwbp_project_camera") is not None
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "gwbp_project_camera" in out.split()
    hdr = open(os.path.join(ROOT, "include", "gwbp.h")).read()
    for name, val in (("GWBP_CAMERA_PINHOLE", 0), ("GWBP_CAMERA_ORTHO", 1), ("GWBP_CAMERA_FISHEYE", 2),
                      ("GWBP_RASTERIZE_CLASSIC", 0), ("GWBP_RASTERIZE_ANTIALIASED", 1)):
        assert f"#define {name} {val}" in hdr
    assert _lib.CAMERA_MODELS == {"pinhole": 0, "ortho": 1, "fisheye": 2}
    assert _lib.RASTERIZE_MODES == {"classic": 0, "antialiased": 1}


@pytest.mark.parametrize("model,mode,what", [(3, 0, b"unknown camera model 3"), (-1, 0, b"unknown camera model -1"),
                                             (0, 2, b"unknown rasterize mode 2"), (2, -1, b"unknown rasterize mode -1")])
def test_unknown_model_or_mode_is_einval_before_any_device_call(model, mode, what):
    lib = _lib.lib()
    # every other argument is null: the check must come first (nothing reaches the HIP runtime on this GPU-less machine)
    rc = lib.gwbp_project_camera(None, None, 0, None, model, mode, None, None, None, None, None, None, None, None, None, None)
    assert rc == -1
    assert what in lib.gwbp_last_error_string()


def test_project_camera_validates_the_rest_like_project():
    lib = _lib.lib()
    caps = _lib.Caps(10, 1 << 16, 1 << 20, 64, 64)
    rc = lib.gwbp_project_camera(C.byref(caps), None, 0, None, 2, 1, None, None, None, None, None, None, None, None, None,
                                 None)
    assert rc in (-1, -2)


def _angles():
    for r in (1.0, 3.0):
        for deg in (0, 1, 5, 15, 30, 45, 60, 75, 80, 85):
            for phi in (0.0, 0.7, 2.0, -2.5):
                th = np.radians(deg)
                p = np.array([r * np.sin(th) * np.cos(phi), r * np.sin(th) * np.sin(phi), r * np.cos(th)])
                if deg == 0:
                    p[:2] = 0.0  # rho = 0 exactly: the optical axis
                yield p


def test_fisheye_jacobian_matches_finite_differences():
    """The restatement's J is the derivative of its own (u, v) map, from the optical axis to 85 degrees off it -- this pins the
    maths independently of anyone's memory of gsplat."""
    fx, fy, cx, cy = 523.0, 481.0, 100.0, 68.0
    worst = 0.0
    for p in _angles():
        J = fisheye_jacobian(p, fx, fy)
        h = 1e-6 * np.linalg.norm(p)
        Jn = np.zeros((2, 3))
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            Jn[:, k] = (fisheye_uv(p + e, fx, fy, cx, cy) - fisheye_uv(p - e, fx, fy, cx, cy)) / (2 * h)
        err = np.abs(J - Jn).max() / np.abs(J).max()
        worst = max(worst, err)
        assert np.isfinite(J).all()
    assert worst < 1e-6, worst
    # on the axis the model is the pinhole's: J = [[fx/z, 0, 0], [0, fy/z, 0]], (u, v) = (cx, cy)
    J0 = fisheye_jacobian(np.array([0.0, 0.0, 2.0]), fx, fy)
    np.testing.assert_allclose(J0, [[fx / 2, 0, 0], [0, fy / 2, 0]], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(fisheye_uv(np.array([0.0, 0.0, 2.0]), fx, fy, cx, cy), [cx, cy])


def test_compensation_without_low_pass_is_one():
    rng = np.random.default_rng(3)
    for _ in range(100):
        A = rng.normal(size=(2, 2))
        S2 = A @ A.T + 1e-3 * np.eye(2)
        assert compensation(S2, 0.0) == 1.0
        assert 0.0 < compensation(S2, 0.3) < 1.0


def _write_cameras_bin(path, models):
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(models)))
        for cid, mid in enumerate(models, start=1):
            _, npar = scene_io._CAMERA_MODELS[mid]
            f.write(struct.pack("<iiQQ", cid, mid, 640, 480))
            params = [500.0, 480.0, 320.0, 240.0, 0.1, -0.02, 0.0, 0.001, 0.0, 0.0, 0.0, 0.0][:npar]
            f.write(struct.pack("<" + "d" * npar, *params))


def test_gsplat_camera_model_of_every_colmap_model(tmp_path):
    sparse = tmp_path / "sparse" / "0"
    sparse.mkdir(parents=True)
    ids = sorted(scene_io._CAMERA_MODELS)
    assert ids == list(range(11))
    _write_cameras_bin(sparse / "cameras.bin", ids)
    (sparse / "images.bin").write_bytes(struct.pack("<Q", 0))
    proj = scene_io.read_colmap_model(str(sparse))
    fisheye = {"SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "OPENCV_FISHEYE", "THIN_PRISM_FISHEYE"}
    got = {cam.model: cam.gsplat_camera_model for cam in proj.cameras.values()}
    assert len(got) == 11
    for name, model in got.items():
        assert model == ("fisheye" if name in fisheye else "pinhole"), name
    # distortion = the parameters after focal length(s) and principal point
    by_name = {cam.model: cam for cam in proj.cameras.values()}
    assert by_name["PINHOLE"].distortion.size == 0 and by_name["SIMPLE_PINHOLE"].distortion.size == 0
    assert list(by_name["OPENCV_FISHEYE"].distortion) == [0.1, -0.02, 0.0, 0.001]
    assert list(by_name["SIMPLE_RADIAL_FISHEYE"].distortion) == [240.0]  # (f, cx, cy, k) -- the 4th value of the fixture


def _cli():
    sys.path.insert(0, ROOT)
    import run_backproject
    return run_backproject


def test_cli_camera_flags():
    rb = _cli()
    ap = rb.build_parser()
    a = ap.parse_args([])
    assert a.camera_model is None and a.rasterize_mode == "classic"  # nothing changes for existing runs
    a = ap.parse_args(["--camera-model", "fisheye", "--rasterize-mode", "antialiased"])
    assert a.camera_model == "fisheye" and a.rasterize_mode == "antialiased"
    assert ap.parse_args(["--camera-model", "ortho"]).camera_model == "ortho"
    for bad in (["--camera-model", "ftheta"], ["--rasterize-mode", "fancy"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_cli_fisheye_warnings():
    rb = _cli()
    Cam = scene_io.Camera
    fish = Cam(1, "OPENCV_FISHEYE", 640, 480, np.array([500.0, 480.0, 320.0, 240.0, 0.1, 0.0, 0.0, 0.0]))
    ideal = Cam(1, "OPENCV_FISHEYE", 640, 480, np.array([500.0, 480.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0]))
    pin = Cam(1, "OPENCV", 640, 480, np.array([500.0, 480.0, 320.0, 240.0, 0.1, 0.0, 0.0, 0.0]))
    w = rb.camera_warnings(fish, None)
    assert len(w) == 2 and all(line.startswith("warning:") and "\n" not in line for line in w)
    assert "--camera-model" in w[0] and "distortion" in w[1]
    assert len(rb.camera_warnings(fish, "fisheye")) == 1  # the coefficients are still ignored
    assert rb.camera_warnings(ideal, "fisheye") == []
    assert len(rb.camera_warnings(ideal, None)) == 1
    assert rb.camera_warnings(pin, None) == []  # pinhole-family distortion is not this feature's concern


def test_view_carries_camera_settings_and_keeps_its_size():
    vm, K = torch.eye(4), torch.tensor([[100.0, 0, 32], [0, 100.0, 32], [0, 0, 1]])
    v = _lib.make_view(vm, K, 64, 64)
    assert _lib.camera_of(v) == ("pinhole", "classic") and _lib.is_default_camera(v)
    v2 = _lib.make_view(vm, K, 64, 64, camera_model="fisheye", rasterize_mode="antialiased")
    assert _lib.camera_of(v2) == ("fisheye", "antialiased") and not _lib.is_default_camera(v2)
    assert bytes(v) == bytes(v2) and C.sizeof(v2) == C.sizeof(_lib.View)
    assert _lib.camera_of(_lib.View()) == ("pinhole", "classic")
    with pytest.raises(ValueError):
        _lib.make_view(vm, K, 64, 64, camera_model="ftheta")
    with pytest.raises(ValueError):
        _lib.make_view(vm, K, 64, 64, rasterize_mode="antialias")


def test_dropin_still_refuses_what_is_not_implemented():
    from gsbp_amd.rasterization import rasterization
    n = 4
    args = (torch.zeros(n, 3), torch.tensor([[1.0, 0, 0, 0]] * n), torch.ones(n, 3), torch.ones(n), torch.zeros(n, 3),
            torch.eye(4)[None], torch.eye(3)[None], 16, 16)
    with pytest.raises(NotImplementedError):
        rasterization(*args, camera_model="ftheta")
    with pytest.raises(NotImplementedError):
        rasterization(*args, rasterize_mode="fancy")
    with pytest.raises(NotImplementedError):
        rasterization(*args, covars=torch.zeros(n, 6))
    with pytest.raises(NotImplementedError):
        rasterization(*args, absgrad=True)
    with pytest.raises(NotImplementedError):
        rasterization(*args, distributed=True)
    # the accepted settings get past the check (and then want HIP tensors)
    for model in ("pinhole", "ortho", "fisheye"):
        for mode in ("classic", "antialiased"):
            with pytest.raises(_lib.GwbpError):
                rasterization(*args, camera_model=model, rasterize_mode=mode)
