"""No-GPU checks of the fused Adam step: csrc/adam_math.h compiled for the host -- plainly and under
-fsanitize=address,undefined, a stand-alone program both times -- gives the bytes of the numpy float32 restatement (tests/adam_ref.py);
that chain against torch.optim.Adam on the CPU by the floor rule, with the float64 chain as the truth and torch's float32 result as the
floor; the zero gradient on zero moments; the mutants the comparison must catch; the C ABI's argument checks; header, map and _lib in
agreement; the command lines' namespaces; what SplatAdam and the adam= keyword refuse without a device.

FACTOR.  The header's chain and torch's single-tensor Adam are the same expressions; what differs is whether lerp_ and addcmul_ fuse a
multiply-add and the order in which addcdiv_ applies the step size.  Measured here over 1 and 25 steps x 3 tensors x 2 figures (the
test prints its largest): ratios 1.000 after 1 step and up to 1.056 after 25, the largest on the Frobenius figure of exp_avg;
HOST_FACTOR = ceil(2 x 1.056) = 3.  A mutant is off by 7e4 floors or more.
"""
import argparse
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import adam_ref as ref
import gsbp_amd
from gsbp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_FACTOR = 3.0
N, W, LR = 257, 45, 1e-2
STEPS = (1, 25)


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++) found")
    d = tmp_path_factory.mktemp("adam_host")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
    src = os.path.join(ROOT, "tests", "adam_host.cpp")
    plain, checked = str(d / "adam_host"), str(d / "adam_host_san")
    subprocess.check_call(base + ["-O2", "-o", plain, src])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", checked, src])
    return plain, checked, d


@pytest.fixture(scope="module")
def sequence():
    """A table and 25 gradients (a fresh draw per step, zeros mixed in), with the truth, the restatement and torch's floor after 1 and
    after 25 steps, computed once.  The optimiser starts as torch's does: zero moments."""
    start = ref.make_tables(N, W, seed=1, zero_moments=True)
    grads = [ref.make_tables(N, W, seed=100 + s)["g"] for s in range(max(STEPS))]
    out = {}
    for steps in STEPS:
        out[steps] = dict(truth=ref.run_steps(ref.chain64, start["p"], start["m"], start["v"], grads[:steps], LR),
                          restated=ref.run_steps(ref.chain32, start["p"], start["m"], start["v"], grads[:steps], LR),
                          floor=ref.torch_adam(start["p"], grads[:steps], LR))
    return start, grads, out


def run_host(exe, tmp, start, grads, lr=LR, first_step=1):
    n, steps = start["p"].size, len(grads)
    src, dst = os.path.join(str(tmp), "adam_in.bin"), os.path.join(str(tmp), "adam_out.bin")
    sc = [ref.scalars32(first_step + s, lr) for s in range(steps)]
    with open(src, "wb") as f:
        f.write(struct.pack("<qiiddff", n, steps, 0, ref.B1, ref.B2, ref.EPS, 0.0))
        f.write(np.array([s["step_size"] for s in sc], np.float32).tobytes() + np.array([s["sqrt_bc2"] for s in sc], np.float32).tobytes())
        f.write(b"".join(np.ascontiguousarray(start[k], np.float32).tobytes() for k in ("p", "m", "v")))
        f.write(b"".join(np.ascontiguousarray(g, np.float32).tobytes() for g in grads))
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    assert len(raw) == 12 * n
    a = np.frombuffer(raw, np.float32).reshape(3, *start["p"].shape)
    return dict(p=a[0], m=a[1], v=a[2]), raw


@pytest.mark.parametrize("steps", STEPS)
def test_the_header_on_the_host_gives_the_restatements_bytes(host_programs, sequence, steps):
    plain, checked, tmp = host_programs
    start, grads, runs = sequence
    got, raw = run_host(plain, tmp, start, grads[:steps])
    want = runs[steps]["restated"]
    for k in ref.TENSORS:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    # the same text under the address and undefined-behaviour sanitizers: a clean run and the same bytes
    assert run_host(checked, tmp, start, grads[:steps])[1] == raw
    # ... and from moments that are not zero, one step at a later count
    warm = ref.make_tables(N, W, seed=2)
    got, raw = run_host(plain, tmp, warm, [warm["g"]], first_step=7)
    want = ref.chain32(warm["p"], warm["g"], warm["m"], warm["v"], 7, LR)
    assert all(np.array_equal(got[k].view(np.uint32), w.view(np.uint32)) for k, w in zip(ref.TENSORS, want))
    assert run_host(checked, tmp, warm, [warm["g"]], first_step=7)[1] == raw


def test_the_inputs_keep_their_promises():
    for zero_moments in (False, True):
        t = ref.make_tables(N, W, seed=2, zero_moments=zero_moments)
        mag = np.abs(t["g"][t["g"] != 0])
        assert mag.min() >= 1e-12 and mag.max() <= 1e2 and mag.min() < 1e-10 and mag.max() > 1.0
        assert 0.05 < (t["g"] == 0).mean() < 0.25 and np.signbit(t["g"][t["g"] == 0]).any()
        assert (t["m"] == 0).any() and (t["v"] == 0).any() and (zero_moments or ((t["m"] != 0).any() and (t["v"] != 0).any()))
        for step in (1, 25):
            ref.check_normal(ref.chain32(t["p"], t["g"], t["m"], t["v"], step, LR, want_parts=True)[1])


@pytest.mark.parametrize("steps", STEPS)
def test_the_chain_against_torch_adam_by_the_floor_rule(sequence, steps):
    _, _, runs = sequence
    r = ref.ratios(runs[steps]["restated"], runs[steps]["truth"], runs[steps]["floor"])
    worst = max(r, key=r.get)
    print(f"{steps} steps: restatement / floor, largest {r[worst]:.3f} at {worst}")
    assert r[worst] <= HOST_FACTOR, r


def test_a_zero_gradient_on_zero_moments_leaves_the_bits():
    p = np.array([1.5, -0.0, 0.0, -3.25e-20, 7e30, 1.0], np.float32)
    g = np.array([0.0, 0.0, -0.0, -0.0, 0.0, -0.0], np.float32)
    z = np.zeros_like(p)
    for step in (1, 2, 1000):
        p1, m1, v1 = ref.chain32(p, g, z, z, step, 0.05)
        assert np.array_equal(p1.view(np.uint32), p.view(np.uint32))
        assert not m1.view(np.uint32).any() and not v1.view(np.uint32).any()
    # with a mask, a row that is not visible keeps its bits whatever its gradient and moments are
    t = ref.make_tables(6, 3, seed=3)
    keep = np.array([1, 0, 0, 1, 0, 1], np.uint8)
    out = ref.masked32(t["p"], t["g"], t["m"], t["v"], keep, 3, LR)
    for old, new in zip((t["p"], t["m"], t["v"]), out):
        assert np.array_equal(old[keep == 0].view(np.uint32), new[keep == 0].view(np.uint32))
        assert (old[keep == 1] != new[keep == 1]).any()


@pytest.mark.parametrize("mutant", ["no_bias_correction", "eps_in_sqrt", "b2_for_m"])
def test_the_comparison_catches_the_mutants(sequence, mutant):
    """(eps inside the root shows on the gradients below sqrt(eps / (1 - b2)) = 1e-6, a third of the draw: there v' is below eps.)"""
    start, grads, runs = sequence
    for steps in STEPS:
        bad = ref.ratios(ref.run_steps(ref.chain32, start["p"], start["m"], start["v"], grads[:steps], LR, mutant=mutant),
                         runs[steps]["truth"], runs[steps]["floor"])
        worst = max(bad, key=bad.get)
        print(f"mutant {mutant}, {steps} steps: largest ratio {bad[worst]:.3g} at {worst}")
        assert bad[worst] > 1000.0 * HOST_FACTOR, (mutant, bad)


# ---- the C ABI: nothing here reaches a kernel --------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_library_exports_it():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gwbp.h")).read(), flags=re.S)
    assert re.search(r"GWBP_API int gwbp_adam_step\s*\(", src)
    assert "gwbp_adam_step" in _lib.ARGTYPES and "gwbp_adam_step" in _lib.EXPORTS
    assert _lib.ARGTYPES["gwbp_adam_step"][9:11] == [C.c_double, C.c_double]
    text = open(os.path.join(ROOT, "3dgs-gradient-backprojection_amd", "csrc", "gwbp.map")).read()
    assert "gwbp_*" in text and "gwbp_adam_step" in text
    assert "adam.hip" in open(os.path.join(ROOT, "3dgs-gradient-backprojection_amd", "csrc", "Makefile")).read()
    gsbp_amd.build()
    assert hasattr(_lib.lib(), "gwbp_adam_step")
    assert callable(gsbp_amd.Engine.adam_step) and issubclass(gsbp_amd.SplatAdam, torch.optim.Adam)


def test_capi_rejects_without_a_launch():
    lib = _lib.lib()
    buf = (C.c_float * 8192)()
    a = (C.addressof(buf) + 15) & ~15  # 16-B aligned; the tables below are 4 KB apart

    def message():
        return lib.gwbp_last_error_string().decode()

    def call(n=4, w=3, p=a, g=a + 4096, m=a + 8192, v=a + 12288, visible=a + 16384, step_size=1e-3, sqrt_bc2=0.5, b1=0.9, b2=0.999,
             eps=1e-15):
        return lib.gwbp_adam_step(n, w, p, g, m, v, visible, step_size, sqrt_bc2, b1, b2, eps, None)

    assert call(n=-1) == -1 and "Gaussians" in message()
    assert call(n=1 << 31) == -1
    for w in (0, -3):
        assert call(w=w) == -1 and "w must be" in message()
    for null in ("p", "g", "m", "v"):
        assert call(**{null: None}) == -1 and "null" in message(), null
    for k in ("p", "g", "m", "v"):
        for off in (4, 8):
            assert call(**{k: a + 4096 * "p g m v".split().index(k) + off}) == -1 and "16-B" in message(), (k, off)
    assert call(m=a) == -1 and "same array" in message()               # m is p
    assert call(v=a + 8192) == -1 and "same array" in message()        # v is m
    assert call(g=a) == -1 and "input" in message()                    # g is p
    assert call(g=a + 12288) == -1 and "input" in message()            # g is v
    assert call(visible=a + 8192) == -1 and "input" in message()       # the mask is m
    for bad in (dict(sqrt_bc2=0.0), dict(sqrt_bc2=float("nan")), dict(step_size=float("nan")), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0)):
        assert call(**bad) == -1 and "scalars" in message(), bad
    # nothing to do: no launch, no device
    assert call(n=0, p=None, g=None, m=None, v=None, visible=None) == 0
    assert call(n=0) == 0
    del buf


# ---- the command lines and the Python layer without a device -----------------------------------------------------------------------
def test_the_command_lines_namespaces_are_unchanged_without_the_options():
    import run_polish
    import run_train
    for tool in (run_train, run_polish):
        ap = tool.build_parser()
        plain = vars(ap.parse_args(["--synthetic", "T0"]))
        assert "adam" not in plain and "means_lr_final" not in plain
        for action in ap._actions:
            if action.dest in ("adam", "means_lr_final"):
                assert action.default is argparse.SUPPRESS
        given = vars(ap.parse_args(["--synthetic", "T0", "--adam", "visible", "--means-lr-final", "0.01"]))
        assert given["adam"] == "visible" and given["means_lr_final"] == 0.01
        assert {k: v for k, v in given.items() if k not in ("adam", "means_lr_final")} == plain
        with pytest.raises(SystemExit):
            ap.parse_args(["--synthetic", "T0", "--adam", "sparse"])


def test_splat_adam_and_the_keywords_refuse_without_a_device():
    p = torch.zeros(5, 3, requires_grad=True)
    for kw in (dict(amsgrad=True), dict(weight_decay=0.1), dict(maximize=True), dict(fused=True), dict(foreach=True), dict(capturable=True)):
        with pytest.raises(gsbp_amd.GwbpError, match="SplatAdam"):
            gsbp_amd.SplatAdam([p], **kw)
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.SplatAdam([p])
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.SplatAdam([dict(params=[p], lr=0.1)], eps=1e-15)
    with pytest.raises(gsbp_amd.GwbpError, match="float32"):
        gsbp_amd.SplatAdam([torch.zeros(5, 3, dtype=torch.float64, requires_grad=True)])
    with pytest.raises(gsbp_amd.GwbpError, match="contiguous"):
        gsbp_amd.SplatAdam([torch.zeros(3, 5).t().requires_grad_(True)])
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.adam.visible_rows(torch.ones(5, dtype=torch.bool))
    from gsbp_amd.engine import adam_scalars, adam_step_tables
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        adam_step_tables(None, None, p.detach(), p.detach(), p.detach(), p.detach(), None, 1, 0.1, 0.9, 0.999, 1e-8)
    assert adam_scalars(3, 0.5, 0.9, 0.999) == ref.scalars64(3, 0.5)
    sc = gsbp_amd.synthetic.make_scene(gsbp_amd.synthetic.CONFIGS["T0"])
    sc["features_dc"], sc["features_rest"] = torch.zeros(512, 1, 3), torch.zeros(512, 15, 3)
    eye, K = torch.eye(4)[None], torch.eye(3)
    calls = (lambda **kw: gsbp_amd.polish_scene(sc, eye, K, 96, 64, lambda v: None, **kw),
             lambda **kw: gsbp_amd.train_scene(sc, eye, K, 96, 64, lambda v: None, 10, **kw))
    for fn in calls:
        for adam in ("sparse", None, True, "Fused"):
            with pytest.raises(gsbp_amd.GwbpError, match="adam must be"):
                fn(adam=adam)
        for final in (0.0, -0.01, float("inf"), float("nan"), True, "0.01"):
            with pytest.raises(gsbp_amd.GwbpError, match="means_lr_final"):
                fn(means_lr_final=final)
        for adam in ("torch", "fused", "visible"):  # a good keyword goes on to the next check: the tensors' device
            with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
                fn(adam=adam, means_lr_final=0.01)
    from gsbp_amd.polish import means_lr_at
    assert means_lr_at(1.6e-4, 0.01, 0, 7000) == 1.6e-4
    assert abs(means_lr_at(1.6e-4, 0.01, 3500, 7000) / 1.6e-5 - 1.0) < 1e-12 and abs(means_lr_at(1.6e-4, 0.01, 7000, 7000) / 1.6e-6 - 1.0) < 1e-12
