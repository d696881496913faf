"""No-GPU checks of the SH colours' backward: csrc/sh_math.h compiled for the host -- plainly and under
-fsanitize=address,undefined, a stand-alone program both times -- against sh_colors_torch under autograd in float64 by the floor rule
of tests/sh_grad_ref.py; the Gaussian at the camera centre on its own; the mutants the comparison must catch; the C ABI's argument
checks; header, map and _lib in agreement; what the Python layer refuses without a device.

FACTOR.  The host's forward and backward differ from the float32 run of sh_colors_torch by the order of a handful of sums and by the
basis derivatives being written out instead of chained through autograd, ulp-level effects of the floor's own size.  Measured here over
the 7 cases x 3 tensors x 2 figures below (each test prints its largest): ratios 1.00 .. 1.44, the largest on the max-abs figure of
v_means at degree 3; HOST_FACTOR = ceil(2 x 1.44) = 3.  A mutant is off by 1e6 floors or more.
"""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import sh_grad_ref as ref
import gsbp_amd
from gsbp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_FACTOR = 3.0
N = 600
CASES = [(d, k) for d in range(4) for k in sorted({(d + 1) ** 2, 16})]


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) found")
    d = tmp_path_factory.mktemp("sh_host")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
    src = os.path.join(ROOT, "tests", "sh_host.cpp")
    plain, checked = str(d / "sh_host"), str(d / "sh_host_san")
    subprocess.check_call(base + ["-O2", "-o", plain, src])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", checked, src])
    return plain, checked, d


@pytest.fixture(scope="module")
def cases():
    """One case per (degree, K), with its float64 truth and float32 floor, computed once."""
    out = {}
    for degree, k in CASES:
        case = ref.make_case(N, degree, k)
        out[(degree, k)] = (case, ref.autograd(case, torch.float64), ref.autograd(case, torch.float32))
    return out


def run_host(exe, tmp, case):
    n, k = case["coeffs"].shape[:2]
    src, dst = os.path.join(str(tmp), "sh_in.bin"), os.path.join(str(tmp), "sh_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<qii3f", n, case["degree"], k, *case["campos"].tolist()))
        f.write(case["means"].tobytes() + case["coeffs"].tobytes() + case["v_colors"].tobytes())
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    assert len(raw) == 4 * (3 * n + 3 * k * n + 3 * n)
    a = np.frombuffer(raw, np.float32)
    return dict(colors=a[:3 * n].reshape(n, 3), v_coeffs=a[3 * n:3 * n + 3 * k * n].reshape(n, k, 3), v_means=a[-3 * n:].reshape(n, 3)), raw


@pytest.mark.parametrize("degree,k", CASES)
def test_the_inputs_keep_their_promises(cases, degree, k):
    case, truth, _ = cases[(degree, k)]
    clamped, edge = ref.case_facts(case)
    assert clamped >= 0.2, clamped
    assert edge >= ref.EDGE, edge
    d = np.linalg.norm(case["means"].astype(np.float64) - case["campos"], axis=1)
    assert d[0] == 0.0 and d[1:].min() >= 0.5
    ref.check_row0(case, truth)  # sh_colors_torch itself: finite, v_dir 1e12, no projection term
    if degree > 0:
        assert np.abs(truth["v_means"][0]).max() > 1e9
    assert not truth["v_coeffs"][:, (degree + 1) ** 2:].any()


@pytest.mark.parametrize("degree,k", CASES)
def test_sh_math_on_the_host_against_float64(host_programs, cases, degree, k):
    plain, checked, tmp = host_programs
    case, truth, floor = cases[(degree, k)]
    got, raw = run_host(plain, tmp, case)
    r = ref.ratios(got, truth, floor)
    worst = max(r, key=r.get)
    print(f"degree {degree}, K {k}: host / floor, largest {r[worst]:.3f} at {worst}")
    assert r[worst] <= HOST_FACTOR, r
    ref.check_row0(case, got)
    # the forward is the float32 chain of k_sh_colors: where torch's float32 run clamps, so does it (no value sits at the edge)
    assert np.array_equal(got["colors"] == 0, truth["colors"] == 0)
    # rows the degree does not use: exact +0, not -0, not what was there
    rest = got["v_coeffs"][:, (degree + 1) ** 2:]
    assert not rest.view(np.uint32).any()
    if degree == 0:
        assert not got["v_means"].view(np.uint32).any()
    # the same text under the address and undefined-behaviour sanitizers: a clean run and the same bytes
    _, raw_checked = run_host(checked, tmp, case)
    assert raw_checked == raw


def test_the_restatement_is_inside_the_rule_and_the_mutants_are_not(cases):
    case, truth, floor = cases[(3, 16)]
    r = ref.ratios(ref.restate(case), truth, floor)
    assert max(r.values()) <= HOST_FACTOR, r
    low, low_truth, low_floor = cases[(1, 16)]
    for mutant, subject, key in (("sign_deg3", (case, truth, floor), ("v_means", "fro")),
                                 ("no_projection", (case, truth, floor), ("v_means", "fro")),
                                 ("no_mask", (case, truth, floor), ("v_coeffs", "fro")),
                                 ("no_zero_rows", (low, low_truth, low_floor), ("v_coeffs", "fro"))):
        c, t, f = subject
        bad = ref.ratios(ref.restate(c, mutant=mutant), t, f)
        print(f"mutant {mutant}: {key} ratio {bad[key]:.3g}")
        assert bad[key] > 1000.0 * HOST_FACTOR, (mutant, bad)


# ---- the C ABI: nothing here reaches a kernel --------------------------------------------------------------------------------------
NAMES = ("gwbp_sh_eval", "gwbp_sh_eval_backward")


def test_header_declares_the_entry_points_and_the_library_exports_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gwbp.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"GWBP_API int {name}\s*\(", src), name
        assert name in _lib.ARGTYPES and name in _lib.EXPORTS
    assert re.search(r"#define GWBP_SH_MAX_K 16\b", src) and _lib.SH_MAX_K == 16
    assert "gwbp_*" in open(os.path.join(ROOT, "3dgs-gradient-backprojection_amd", "csrc", "gwbp.map")).read()
    gsbp_amd.build()
    assert all(hasattr(_lib.lib(), n) for n in NAMES)
    for name in ("sh_colors", "sh_colors_torch"):
        assert callable(getattr(gsbp_amd, name)), name
    for name in ("sh_eval", "sh_eval_backward"):
        assert callable(getattr(gsbp_amd.Engine, name)), name
    assert callable(gsbp_amd.rasterization.__globals__["set_sh_kernel"])


def test_capi_rejects_without_a_launch():
    lib = _lib.lib()
    buf = (C.c_float * 4096)()
    a = C.addressof(buf)
    cp = (C.c_float * 3)(0.0, 0.0, 0.0)

    def message():
        return lib.gwbp_last_error_string().decode()

    def ev(n=4, degree=3, kh=1, kt=15, means=a, head=a + 256, tail=a + 1024, campos=cp, out=a + 8192):
        return lib.gwbp_sh_eval(n, degree, kh, kt, means, head, tail, campos, out, None)

    def bw(n=4, degree=3, kh=1, kt=15, means=a, head=a + 256, tail=a + 1024, campos=cp, v=a + 8192, vh=a + 9216, vt=a + 10240,
           vm=a + 12288):
        return lib.gwbp_sh_eval_backward(n, degree, kh, kt, means, head, tail, campos, v, vh, vt, vm, None)

    for fn in (ev, bw):
        assert fn(n=-1) == -1 and "Gaussians" in message()
        assert fn(n=1 << 31) == -1
        for degree in (-1, 4):
            assert fn(degree=degree) == -1 and "degree" in message()
        assert fn(kh=0, kt=16) == -1 and "K_head" in message()
        assert fn(kt=-1) == -1
        assert fn(kt=14) == -1 and "fewer" in message()
        assert fn(degree=1, kh=1, kt=2) == -1 and "fewer" in message()
        assert fn(kt=16) == -1 and "GWBP_SH_MAX_K" in message()
        assert fn(tail=None) == -1 and "null tail" in message()
        assert fn(kh=16, kt=0) == -1 and "K_tail = 0" in message()
        assert fn(campos=None) == -1 and "campos" in message()
        for null in ("means", "head"):
            assert fn(**{null: None}) == -1 and "null" in message(), null
        assert fn(means=a + 2) == -1 and fn(head=a + 257) == -1 and fn(tail=a + 1026) == -1 and "4-B" in message()
    assert ev(out=None) == -1 and "null out" in message()
    assert ev(out=a + 8193) == -1 and "4-B" in message()
    assert ev(out=a) == -1 and "input" in message()
    assert bw(vh=None, vt=None, vm=None) == -1 and "every output" in message()
    assert bw(v=None) == -1 and "v_colors" in message()
    assert bw(kh=16, kt=0, tail=None) == -1 and "v_tail" in message()
    for k in ("v", "vh", "vt", "vm"):
        assert bw(**{k: a + 8193 + 1024 * "v vh vt vm".split().index(k)}) == -1 and "4-B" in message(), k
    assert bw(vh=a + 256) == -1 and "input" in message()       # v_head is head
    assert bw(vt=a + 1024) == -1 and "input" in message()      # v_tail is tail
    assert bw(vm=a) == -1 and bw(vh=a + 8192) == -1            # v_means is means, v_head is v_colors
    assert bw(vh=a + 9216, vt=a + 9216) == -1 and "same array" in message()
    # nothing to do: no launch, no device
    assert ev(n=0, means=None, head=None, tail=None, kt=15, out=None) == -1  # (a null tail with K_tail > 0 stays an error)
    assert ev(n=0, kh=16, kt=0, means=None, head=None, tail=None, out=None) == 0
    assert bw(n=0, kh=16, kt=0, means=None, head=None, tail=None, v=None, vt=None) == 0
    del buf


# ---- the Python layer without a device ---------------------------------------------------------------------------------------------
def test_cpu_tensors_and_bad_arguments_raise():
    m, c = torch.zeros(5, 3), torch.zeros(5, 16, 3)
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.sh_colors(3, m, c, (0.0, 0.0, 0.0))
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.sh_colors(0, m, c[:, :1], (0.0, 0.0, 0.0), rest=c[:, 1:])
    sc = gsbp_amd.synthetic.make_scene(gsbp_amd.synthetic.CONFIGS["T0"])
    sc["features_dc"], sc["features_rest"] = torch.zeros(512, 1, 3), torch.zeros(512, 15, 3)
    eye, K = torch.eye(4)[None], torch.eye(3)
    for interval in (0, -5, 2.5, True, "1000"):
        for fn in (lambda **kw: gsbp_amd.polish_scene(sc, eye, K, 96, 64, lambda v: None, **kw),
                   lambda **kw: gsbp_amd.train_scene(sc, eye, K, 96, 64, lambda v: None, 10, **kw)):
            with pytest.raises(gsbp_amd.GwbpError, match="sh_degree_interval"):
                fn(sh_degree_interval=interval)
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.polish_scene(sc, eye, K, 96, 64, lambda v: None, sh_degree_interval=1000)
    from gsbp_amd.polish import render_splats, scheduled_sh_degree, table_sh_degree
    assert table_sh_degree(sc) == 3
    assert [scheduled_sh_degree(s, 5, 3) for s in (0, 4, 5, 9, 10, 15, 16, 400)] == [0, 0, 1, 1, 2, 3, 3, 3]
    assert scheduled_sh_degree(7, None, 3) is None
    for bad in (4, -1, 1.0, True):
        with pytest.raises(gsbp_amd.GwbpError, match="sh_degree must be"):
            render_splats(sc, eye[0], K, 96, 64, sh_degree=bad)
    sc["features_rest"] = torch.zeros(512, 14, 3)
    with pytest.raises(gsbp_amd.GwbpError, match="no full degree"):
        render_splats(sc, eye[0], K, 96, 64)
