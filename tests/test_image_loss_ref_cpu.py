"""No-GPU checks behind the photometric loss (csrc/ssim.hip, gsbp_amd.photometric): the torch restatement of its contract
(tests/image_loss_ref.py) against itself -- the stored-map backward the kernels use against autograd and finite differences --, the
window's bits, the header's constants, csrc/ssim_math.h compiled for the host (tests/ssim_host.cpp), the argument checks of the C ABI,
and the proof that the floor rule of tests/test_gpu_image_loss.py is not blind: four broken variants of the contract fail it.

ssim_host.cpp's bound: the float32 results of ssim_point within RATIO x 2^-24 x kappa x scale of float64 on the same moments (kappa =
1 + (m2 + m3 + |m4|) / Dn is the amplification of the cancelling variances; its header gives the scales).  Measured: ssim 1.21, d12
1.58, d1 1.62, dmu 1.14, ssim_grad 3.17 (of 2^-24 x the sum of its terms' magnitudes); RATIO = 8.  x = y gives exactly 1.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import image_loss_ref as ref
from gsbp_amd import _lib, photometric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(padding, weighted) for padding in ("valid", "same") for weighted in (False, True)]


def case(H=19, W=23, D=2, weighted=False, seed=0):
    x, y = ref.smooth_pair(H, W, D, seed)
    return x, y, ref.smooth_weights(H, W, seed) if weighted else None


@pytest.mark.parametrize("padding,weighted", CASES)
@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
def test_stored_map_backward_is_autograd(padding, weighted, lam):
    x, y, w = case(weighted=weighted)
    loss_a, grad_a = ref.autograd_gradient(x, y, lam, padding, w)
    loss_s, grad_s = ref.stored_map_backward(x, y, lam, padding, w)
    err = float((grad_a - grad_s).norm() / grad_a.norm())
    print(f"{padding} weighted={weighted} lambda={lam}: |stored - autograd| / |autograd| = {err:.2e}")
    assert err <= 1e-12 and abs(float(loss_a) - float(loss_s)) <= 1e-12


@pytest.mark.parametrize("padding,weighted", CASES)
def test_stored_map_backward_is_the_slope_of_its_loss(padding, weighted):
    """Central differences of the float64 loss along seeded directions; the ties (x = y, where |x - y| has a kink) stay out of them."""
    x, y, w = case(H=15, W=17, weighted=weighted, seed=1)
    _, grad = ref.stored_map_backward(x, y, 0.2, padding, w)
    gen = torch.Generator().manual_seed(5)
    x64 = x.double()
    for _ in range(4):
        d = torch.randn(x.shape, generator=gen, dtype=torch.float64) * (x != y)
        h = 1e-6
        slope = (ref.loss_of(x64 + h * d, y, 0.2, padding, w) - ref.loss_of(x64 - h * d, y, 0.2, padding, w)) / (2 * h)
        want = float((grad * d).sum())
        assert abs(float(slope) - want) <= 1e-6 * max(abs(want), float(grad.norm() * d.norm()) * 1e-3), (float(slope), want)


def test_window_bits():
    g = photometric.gaussian_window()
    assert g.dtype == torch.float32 and g.shape == (11,)
    bits = [0x3a86cab6, 0x3bf8ff01, 0x3d13758c, 0x3ddff87f, 0x3e5a1e20, 0x3e8832b0, 0x3e5a1e20, 0x3ddff87f, 0x3d13758c, 0x3bf8ff01,
            0x3a86cab6]
    assert g.view(torch.int32).tolist() == bits
    assert torch.equal(g, ref.window(torch.float32))
    hdr = open(os.path.join(_lib.CSRC, "ssim_math.h")).read()
    taps = re.search(r"#define GWBP_SSIM_WINDOW(.*?)\}", hdr, flags=re.S).group(1)
    assert [float.fromhex(t.rstrip("f")) for t in re.findall(r"0x[0-9a-f.]+p-?\d+f", taps)] == g.double().tolist()
    c1, c2 = (float.fromhex(re.search(rf"{name} = (0x[0-9a-f.]+p-?\d+)f", hdr).group(1)) for name in ("kSsimC1", "kSsimC2"))
    assert c1 == ref.C1 and c2 == ref.C2


def test_tile_and_limits_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "gwbp.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert photometric.SSIM_TILE == (define("GWBP_SSIM_TILE_Y"), define("GWBP_SSIM_TILE_X"))
    assert _lib.IMAGE_LOSS_MAX_D == define("GWBP_IMAGE_LOSS_MAX_D")
    assert _lib.SSIM_PADDINGS == {"valid": define("GWBP_SSIM_VALID"), "same": define("GWBP_SSIM_SAME")}
    stripped = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    for name in ("gwbp_image_loss", "gwbp_image_loss_workspace_size"):
        assert f"GWBP_API int {name}(" in stripped and name in _lib.ARGTYPES and name in _lib.EXPORTS
    assert "ssim.hip" in mk and "ssim$(SUF): ssim_math.h" in mk


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_the_floor_rule_sees_a_broken_contract(mutant):
    """A float64 evaluation of a contract with one thing broken, held to the rule of the GPU test at its ceiling FACTOR = 16: it must
    fail for the gradient (and, where the map or the loss changes, there too)."""
    padding = "same" if mutant == "same_over_valid_count" else "valid"
    x, y, w = case(H=27, W=31, D=3, weighted=True, seed=2)
    _, truth = ref.stored_map_backward(x, y, 0.2, padding, w)
    _, floor32 = ref.stored_map_backward(x, y, 0.2, padding, w, dtype=torch.float32)
    _, broken = ref.stored_map_backward(x, y, 0.2, padding, w, mutant=mutant)
    ok = ref.floor_ratios(floor32, truth, floor32)
    ratios = ref.floor_ratios(broken, truth, floor32)
    print(f"{mutant}: ratios {ratios[0]:.3g} (Frobenius) {ratios[1]:.3g} (max-abs); the float32 restatement itself: {ok}")
    assert min(ratios) > 16 and max(ok) <= 1.0


def test_the_float32_restatement_is_close_to_float64():
    x, y, w = case(H=40, W=45, D=3, weighted=True, seed=3)
    _, truth = ref.stored_map_backward(x, y, 0.2, "valid", w)
    _, floor32 = ref.stored_map_backward(x, y, 0.2, "valid", w, dtype=torch.float32)
    m64, m32 = ref.ssim_map(x, y, "valid"), ref.ssim_map(x, y, "valid", torch.float32)
    rel = float((floor32.double() - truth).norm() / truth.norm())
    print(f"float32 restatement: gradient {rel:.2e} (relative, Frobenius), map {float((m32.double() - m64).abs().max()):.2e} (max-abs)")
    assert rel < 1e-4 and float((m32.double() - m64).abs().max()) < 1e-4
    assert torch.equal(ref.ssim_map(x, x, "same", torch.float32), torch.ones(40, 45, 3))


def test_ssim_math_on_the_host(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) found")
    exe = str(tmp_path / "ssim_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-o", exe,
                           os.path.join(ROOT, "tests", "ssim_host.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr


# ---- the C ABI's argument checks: nothing here reaches a kernel ---------------------------------------------------------------------
def call(lib, **over):
    buf = (C.c_double * 64)()
    addr = C.addressof(buf)
    a = dict(height=16, width=16, D=3, x=addr, xs=3, y=addr, ys=3, pw=None, padding=0, lam=0.2, map=None, grad=None, gs=3, table=addr,
             ws=addr, ws_bytes=0, stream=None)
    a.update(over)
    return lib.gwbp_image_loss(a["height"], a["width"], a["D"], a["x"], a["xs"], a["y"], a["ys"], a["pw"], a["padding"], a["lam"],
                               a["map"], a["grad"], a["gs"], a["table"], a["ws"], a["ws_bytes"], a["stream"]), buf


def test_capi_rejects_without_a_launch():
    lib = _lib.lib()

    def message():
        return lib.gwbp_last_error_string().decode()
    for h, w in ((10, 16), (16, 10), (1, 1)):
        assert call(lib, height=h, width=w)[0] == -1
        assert f"{w} x {h}" in message() and "11" in message()
    for D in (0, 33, -1):
        assert call(lib, D=D)[0] == -1 and str(D) in message()
    assert call(lib, padding=2)[0] == -1 and "padding" in message()
    assert call(lib, height=0)[0] == -1 and call(lib, width=-3, padding=1)[0] == -1
    for null in ("x", "y", "table", "ws"):
        assert call(lib, **{null: None})[0] == -1 and "null" in message()
    assert call(lib, xs=2)[0] == -1 and call(lib, ys=2)[0] == -1 and "strides" in message()
    buf = (C.c_double * 4)()
    assert call(lib, grad=C.addressof(buf), gs=2)[0] == -1
    assert call(lib, x=C.addressof(buf) + 2)[0] == -1 and "aligned" in message()
    assert call(lib, table=C.addressof(buf) + 4)[0] == -1 and "8-B" in message()
    # everything valid but the workspace: too small by one byte, with and without the gradient's planes
    for grad in (None, C.addressof(buf)):
        need = C.c_size_t(0)
        assert lib.gwbp_image_loss_workspace_size(16, 16, 3, int(grad is not None), C.byref(need)) == 0
        assert call(lib, grad=grad, ws_bytes=need.value - 1)[0] == -2 and str(need.value) in message()


def test_workspace_size_is_its_documented_formula():
    lib = _lib.lib()
    ty, tx = photometric.SSIM_TILE
    n = C.c_size_t(0)
    for h, w, d in ((1, 1, 1), (11, 11, 3), (ty, tx, 4), (ty + 1, tx + 1, 32), (1060, 1600, 3)):
        tiles = -(-h // ty) * -(-w // tx)
        for want_grad in (0, 1):
            assert lib.gwbp_image_loss_workspace_size(h, w, d, want_grad, C.byref(n)) == 0
            assert n.value == 40 * tiles + (12 * h * w * d if want_grad else 0), (h, w, d, want_grad)
    assert lib.gwbp_image_loss_workspace_size(16, 16, 3, 1, None) == -1
    assert lib.gwbp_image_loss_workspace_size(16, 16, 0, 1, C.byref(n)) == -1
    assert lib.gwbp_image_loss_workspace_size(0, 16, 3, 1, C.byref(n)) == -1
    assert lib.gwbp_image_loss_workspace_size(1 << 14, 1 << 13, 3, 1, C.byref(n)) == -1  # more than GWBP_IMAGE_LOSS_MAX_PIXELS


def test_cpu_tensors_raise():
    x, y, _ = case()
    with pytest.raises(_lib.GwbpError, match="no CPU path"):
        photometric.photometric_loss(x, y)
    with pytest.raises(_lib.GwbpError, match="no CPU path"):
        photometric.ssim_map(x, y)
    with pytest.raises(_lib.GwbpError, match="padding"):
        photometric.photometric_loss(x, y, padding="reflect")
