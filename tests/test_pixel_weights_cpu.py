"""No-GPU checks of the per-pixel weight maps (gwbp_pixel_weights, the gwbp_*_ex blends, Engine.pixel_weights): the struct layout,
argument validation before any device call, the Python validator, and the assembly of the weighted producer / consumer kernel."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib
from gsbp_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below fails validation first


def test_pixel_weights_struct_layout():
    assert C.sizeof(_lib.PixelWeights) == 32
    offs = {name: getattr(_lib.PixelWeights, name).offset for name, _ in _lib.PixelWeights._fields_}
    assert offs == {"data": 0, "ws_y": 8, "ws_x": 16, "dtype": 24, "reserved": 28}
    hdr = open(os.path.join(ROOT, "include", "gwbp.h")).read()
    body = re.search(r"typedef struct gwbp_pixel_weights \{(.*?)\} gwbp_pixel_weights;", hdr, re.S).group(1)
    assert [ln.split("/*")[0].strip() for ln in body.strip().splitlines()] == [
        "const void *data;", "int64_t ws_y, ws_x;", "int32_t dtype;", "int32_t reserved;"]
    codes = {k: int(v) for k, v in re.findall(r"#define GWBP_PIXW_(\w+) (\d+)", hdr)}
    assert codes == {"F32": _lib.PIXW_F32, "F16": _lib.PIXW_F16, "BF16": _lib.PIXW_BF16, "U8": _lib.PIXW_U8}


def test_ex_entry_points_are_exported():
    gsbp_amd.build()
    for name in ("gwbp_blend_weights_ex", "gwbp_blend_weights_d_ex", "gwbp_blend_tokens_ex", "gwbp_blend_scatter_ex",
                 "gwbp_blend_scatter_encoded_ex"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib(), name) is not None


def _ex_calls(pw):
    """Each _ex entry point with a null caps / workspace / view and the given weight map."""
    L = _lib.lib()
    ref = C.byref(pw)
    return {
        "gwbp_blend_weights_ex": lambda: L.gwbp_blend_weights_ex(None, None, 0, None, None, ref, None),
        "gwbp_blend_weights_d_ex": lambda: L.gwbp_blend_weights_d_ex(None, None, 0, None, None, 1.0, FAKE, ref, None),
        "gwbp_blend_tokens_ex": lambda: L.gwbp_blend_tokens_ex(None, None, 0, None, FAKE, FAKE, None, ref, None),
        "gwbp_blend_scatter_ex": lambda: L.gwbp_blend_scatter_ex(None, None, 0, None, FAKE, 16, 16, 16, 1.0, 1.0, FAKE, FAKE,
                                                                None, ref, None),
        "gwbp_blend_scatter_encoded_ex": lambda: L.gwbp_blend_scatter_encoded_ex(None, None, 0, None, FAKE, 16, 16, 16, FAKE, 8,
                                                                                1.0, 1.0, FAKE, FAKE, None, ref, None),
    }


def _pw(data=0x2000, ws_y=200, ws_x=1, dtype=_lib.PIXW_F32, reserved=0):
    pw = _lib.PixelWeights()
    pw.data, pw.ws_y, pw.ws_x, pw.dtype, pw.reserved = data, ws_y, ws_x, dtype, reserved
    return pw


@pytest.mark.parametrize("bad, msg", [(dict(dtype=4), "unknown pixel weight type"), (dict(dtype=-1), "unknown pixel weight type"),
                                      (dict(data=None), "null pixel weight map"), (dict(ws_y=-1), "negative"),
                                      (dict(ws_x=-200), "negative"), (dict(reserved=1), "reserved")])
def test_ex_entry_points_reject_bad_weight_maps_first(bad, msg):
    """Checked before the caps, the workspace or the view are looked at (all NULL here), so no device is involved."""
    gsbp_amd.build()
    for name, call in _ex_calls(_pw(**bad)).items():
        assert call() == -1, name
        assert msg in _lib.lib().gwbp_last_error_string().decode(), name


def test_ex_entry_points_with_a_valid_map_go_on_to_the_other_arguments():
    gsbp_amd.build()
    for name, call in _ex_calls(_pw(dtype=_lib.PIXW_U8)).items():
        assert call() == -1, name  # the NULL caps
        assert "pixel weight" not in _lib.lib().gwbp_last_error_string().decode(), name


def _engine_stub():
    """An Engine without a workspace: enough for the validator, which touches no device."""
    e = gsbp_amd.Engine.__new__(gsbp_amd.Engine)
    e.device, e._dev_index = torch.device("cuda:0"), 0
    return e


class _View:
    width, height = 20, 10


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.float64, torch.int8, torch.complex64])
def test_validator_rejects_unsupported_types(dtype):
    with pytest.raises(gsbp_amd.GwbpError, match="bool, uint8, float16, bfloat16 or float32"):
        _engine_stub().pixel_weights(torch.zeros(10, 20, dtype=dtype), _View())


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.float16, torch.bfloat16, torch.float32])
def test_validator_rejects_host_tensors(dtype):
    with pytest.raises(gsbp_amd.GwbpError, match="device"):
        _engine_stub().pixel_weights(torch.ones(10, 20, dtype=dtype), _View())


def test_validator_rejects_non_tensors():
    with pytest.raises(gsbp_amd.GwbpError, match="tensor"):
        _engine_stub().pixel_weights([[1.0] * 20] * 10, _View())


def test_view_fn_cannot_take_pixel_weights():
    cfg = syn.CONFIGS["T0"]
    means, quats, scales, opac = syn.activate(syn.make_scene(cfg))
    with pytest.raises(ValueError, match="pixel_weight_fn"):
        gsbp_amd.create_feature_field(means, quats, scales, opac, syn.make_cameras(cfg), syn.intrinsics(cfg), cfg.width,
                                      cfg.height, lambda v: torch.zeros(cfg.height, cfg.width, 4), 4,
                                      view_fn=lambda v, f: None, pixel_weight_fn=lambda v: torch.ones(cfg.height, cfg.width))


def test_synthetic_weight_maps_are_seeded():
    cfg = syn.CONFIGS["T1"]
    m = syn.make_pixel_weights(cfg, 0)
    assert m.dtype == torch.bool and tuple(m.shape) == (cfg.height, cfg.width)
    assert not m[0].any() and not m[:, 0].any() and 0.5 < float(m.float().mean()) < 1.0
    assert torch.equal(m, syn.make_pixel_weights(cfg, 0))
    c = syn.make_pixel_weights(cfg, 1, kind="confidence")
    assert c.dtype == torch.float32 and float(c.max()) < 1.0 and torch.equal(c > 0, syn.make_pixel_weights(cfg, 1))


def test_weighted_producer_consumer_kernel_has_no_lane_masked_loops(tmp_path):
    """tests/test_capi_cpu.py::test_producer_consumer_kernel_has_no_lane_masked_loops on the WEIGHTED instantiation
    k_blend<kFusedPC, WAVES, true>: every ring loop stays wave-uniform and bounded."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-munsafe-fp-atomics", "-fvisibility=hidden", "-S", "--cuda-device-only"]
    out = tmp_path / "blend.s"
    subprocess.check_call([hipcc, *flags, "-o", str(out), os.path.join(_lib.CSRC, "blend.hip")], stderr=subprocess.DEVNULL)
    body, on, seen = [], False, False
    for line in out.read_text().splitlines():
        if re.match(r"_ZN4gwbp7k_blendILi5ELi\d+ELb1E\S*:", line):
            on = seen = True
        elif on and line.startswith(".Lfunc_end"):
            break
        elif on:
            body.append(line)
    assert seen and len(body) > 500, "k_blend<kFusedPC, 16, true> not found in the assembly"
    masked = [ln.strip() for ln in body if "s_andn2_b64 exec, exec" in ln]
    assert len(masked) <= 1, masked
    assert sum("s_sleep" in ln for ln in body) == 2


@pytest.mark.parametrize("maps", [["--feature-maps", "fm"], ["--label-maps", "lm", "--num-classes", "4"],
                                  ["--synthetic", "C1", "--num-classes", "4"], ["--synthetic", "C1"]])
def test_cli_parser_accepts_pixel_weights(maps):
    import sys
    sys.path.insert(0, ROOT)
    import run_backproject
    a = run_backproject.build_parser().parse_args([*maps, "--pixel-weights", "weights"])
    assert a.pixel_weights == "weights"
    assert run_backproject.build_parser().parse_args(maps).pixel_weights is None
