"""No-GPU checks of the render-fed drivers (create_feature_field / create_label_field / create_mask_feature_field(render_colors=,
sh_degree=)) and the gwbp_blend_*_rgb entry points: argument validation before any GPU work, the header declarations, EINVAL on
bad arguments without a device, and the register budget of the RENDER instantiations of k_blend."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gwbp.h")
FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below fails validation first
RGB = ("gwbp_blend_weights_rgb", "gwbp_blend_weights_d_rgb", "gwbp_blend_tokens_rgb")
N, H, W = 16, 8, 12


def _scene():
    g = torch.Generator().manual_seed(0)
    return (torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g), torch.rand(N, 3, generator=g),
            torch.rand(N, generator=g), torch.eye(4)[None].repeat(2, 1, 1), torch.eye(3))


def _drivers():
    means, quats, scales, opac, vms, K = _scene()
    common = (means, quats, scales, opac, vms, K, W, H)
    return {
        "feature": lambda **kw: gsbp_amd.create_feature_field(*common, lambda v, img=None: None, 8, **kw),
        "label": lambda **kw: gsbp_amd.create_label_field(*common, lambda v, img=None: None, 4, **kw),
        "mask": lambda **kw: gsbp_amd.create_mask_feature_field(*common, lambda v, img=None: None, 8, **kw),
    }


BAD = [
    (dict(sh_degree=3), "sh_degree needs render_colors"),
    (dict(render_colors=torch.zeros(N, 3), sh_degree=4), "sh_degree must be an int in 0..3"),
    (dict(render_colors=torch.zeros(N, 16, 3), sh_degree=-1), "sh_degree must be an int in 0..3"),
    (dict(render_colors=torch.zeros(N, 16, 3), sh_degree=1.0), "sh_degree must be an int in 0..3"),
    (dict(render_colors=torch.zeros(N, 16, 3), sh_degree=True), "sh_degree must be an int in 0..3"),
    (dict(render_colors=torch.zeros(N, 4)), r"must be \[N, 3\]"),
    (dict(render_colors=torch.zeros(N + 1, 3)), r"must be \[N, 3\]"),
    (dict(render_colors=torch.zeros(N, 16, 3)), r"must be \[N, 3\]"),
    (dict(render_colors=torch.zeros(N, 3), sh_degree=0), r"\[N, K, 3\] SH coefficients"),
    (dict(render_colors=torch.zeros(N, 9, 3), sh_degree=3), r"K >= 16"),
    (dict(render_colors=torch.zeros(N, 16, 4), sh_degree=3), r"\[N, K, 3\] SH coefficients"),
    (dict(render_colors=torch.zeros(N, 3, dtype=torch.float64)), "must be float32"),
    (dict(render_colors=[[0.0, 0.0, 0.0]] * N), "must be a tensor"),
]


@pytest.mark.parametrize("driver", ["feature", "label", "mask"])
@pytest.mark.parametrize("kw, msg", BAD)
def test_drivers_reject_bad_render_arguments_before_any_gpu_work(driver, kw, msg):
    """CPU tensors throughout: a ValueError must come before anything reaches the device (which would raise otherwise)."""
    with pytest.raises(ValueError, match=msg):
        _drivers()[driver](**kw)


def test_render_colors_on_another_device_are_rejected():
    means, quats, scales, opac, vms, K = _scene()
    with pytest.raises(ValueError, match="Gaussians' device"):
        gsbp_amd.create_feature_field(means, quats, scales, opac, vms, K, W, H, lambda v, i: None, 8,
                                      render_colors=torch.zeros(N, 3, dtype=torch.float32, device="meta"))


def test_render_colors_cannot_go_with_view_fn():
    means, quats, scales, opac, vms, K = _scene()
    with pytest.raises(ValueError, match="view_fn"):
        gsbp_amd.create_feature_field(means, quats, scales, opac, vms, K, W, H, lambda v, i: None, 8,
                                      view_fn=lambda v, f: None, render_colors=torch.zeros(N, 3))


def test_without_render_colors_the_callback_takes_one_argument():
    """Regression guard, not evidence for the feature (it passes without it too): without render_colors, view_fn's CPU path still
    calls feature_fn(v) with one argument."""
    means, quats, scales, opac, vms, K = _scene()
    calls = []

    def feature_fn(v):
        calls.append(v)
        return torch.ones(H, W, 8)

    gsbp_amd.create_feature_field(means, quats, scales, opac, vms, K, W, H, feature_fn, 8,
                                  view_fn=lambda v, f: None, views=[0, 1])
    assert calls == [0, 1]


def test_new_header_declarations_are_plain_c(tmp_path):
    """The three _rgb prototypes are in include/gwbp.h and a C99 translation unit can take their addresses with the argument
    list the ctypes binding uses."""
    code = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in RGB:
        assert re.search(r"GWBP_API int %s\(" % name, code), name
        assert name in _lib.EXPORTS and name in _lib.ARGTYPES
    src = tmp_path / "rgb.c"
    src.write_text('#include "gwbp.h"\n'
                   "typedef int (*w_t)(const gwbp_caps *, void *, size_t, const gwbp_view *, float *, const gwbp_pixel_weights *,"
                   " const float *, float *, void *);\n"
                   "typedef int (*wd_t)(const gwbp_caps *, void *, size_t, const gwbp_view *, float *, float, float *,"
                   " const gwbp_pixel_weights *, const float *, float *, void *);\n"
                   "typedef int (*t_t)(const gwbp_caps *, void *, size_t, const gwbp_view *, const int32_t *, const int32_t *,"
                   " float *, const gwbp_pixel_weights *, const float *, float *, void *);\n"
                   "w_t a = gwbp_blend_weights_rgb; wd_t b = gwbp_blend_weights_d_rgb; t_t c = gwbp_blend_tokens_rgb;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I",
                           os.path.dirname(HDR), str(src)])


def _rgb_calls(colors, image, pw=None):
    """Each _rgb entry point with a null caps / workspace / view."""
    L = _lib.lib()
    ref = C.byref(pw) if pw is not None else None
    return {
        "gwbp_blend_weights_rgb": lambda: L.gwbp_blend_weights_rgb(None, None, 0, None, None, ref, colors, image, None),
        "gwbp_blend_weights_d_rgb": lambda: L.gwbp_blend_weights_d_rgb(None, None, 0, None, None, 1.0, FAKE, ref, colors, image,
                                                                       None),
        "gwbp_blend_tokens_rgb": lambda: L.gwbp_blend_tokens_rgb(None, None, 0, None, FAKE, FAKE, None, ref, colors, image, None),
    }


@pytest.mark.parametrize("colors, image", [(FAKE, None), (None, FAKE)])
def test_rgb_entry_points_need_both_colors_and_image(colors, image):
    gsbp_amd.build()
    for name, call in _rgb_calls(colors, image).items():
        assert call() == _lib_einval(), name
        assert "RGB composite needs both" in _lib.lib().gwbp_last_error_string().decode(), name


def test_rgb_entry_points_check_the_pixel_weights_first():
    gsbp_amd.build()
    pw = _lib.PixelWeights()
    pw.data, pw.ws_y, pw.ws_x, pw.dtype, pw.reserved = 0x2000, 12, 1, 9, 0
    for name, call in _rgb_calls(FAKE, None, pw).items():
        assert call() == _lib_einval(), name
        assert "unknown pixel weight type" in _lib.lib().gwbp_last_error_string().decode(), name


@pytest.mark.parametrize("colors, image", [(FAKE, FAKE), (None, None)])
def test_rgb_entry_points_with_valid_render_arguments_go_on_to_the_workspace(colors, image):
    gsbp_amd.build()
    for name, call in _rgb_calls(colors, image).items():
        assert call() == _lib_einval(), name  # the NULL caps
        assert "RGB composite" not in _lib.lib().gwbp_last_error_string().decode(), name


def _lib_einval():
    return -1  # GWBP_EINVAL


# k_blend<MODE, 1, PIXW, RENDER = true>: (mode, weighted) -> the allocation limit the design keeps to
RENDER_KERNELS = {(0, False): 80, (0, True): 80, (1, False): 80, (1, True): 88, (4, False): 80, (4, True): 80}


def test_render_instantiations_compile_without_scratch_and_within_the_register_budget(tmp_path):
    """The RENDER instantiations of k_blend (kStore = 0, kHalves = 1, kToken = 4; unweighted and weighted) compile for gfx950
    with zero scratch and at most the VGPRs their wave count allows (80 = 6 waves per SIMD; the weighted kHalves composite 88);
    the counts are in the failure message."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-munsafe-fp-atomics", "-fvisibility=hidden", "-S", "--cuda-device-only",
             "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run([hipcc, *flags, "-o", str(tmp_path / "blend.s"), os.path.join(_lib.CSRC, "blend.hip")],
                       capture_output=True, text=True, check=True)
    found, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: _ZN4gwbp7k_blendILi(\d)ELi1ELb([01])ELb1E", line)
        if m:
            cur = (int(m.group(1)), m.group(2) == "1")
            found[cur] = {}
            continue
        if "Function Name:" in line:
            cur = None
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            found[cur][m.group(1)] = int(m.group(2))
    report = "; ".join(f"k_blend<{k[0]}, 1, {k[1]}, true>: {v}" for k, v in sorted(found.items()))
    assert set(found) == set(RENDER_KERNELS), report
    for k, limit in RENDER_KERNELS.items():
        assert found[k]["ScratchSize [bytes/lane]"] == 0, report
        assert found[k]["VGPRs"] <= limit, report
