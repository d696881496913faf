"""No-GPU checks of the SH colours with the camera centre on the device and of pose.PoseAdjust: header, map and _lib
in agreement on the three new entry points; the C ABI's argument checks, none of which reaches a kernel; PoseAdjust.apply against
inverse(c2w @ T) in float64; what the Python layer refuses without a device.  (No per-row arithmetic was added to csrc/sh_math.h: the
new kernels call sh_forward_row and sh_backward_row, which tests/test_sh_grad_cpu.py checks on the host.)
"""
import ctypes as C
import os
import re

import pytest
import torch

import gsbp_amd
from gsbp_amd import _lib
from gsbp_amd.pose import PoseAdjust, PoseTraining, rigid_inverse, rotation_6d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gwbp_sh_eval_dev", "gwbp_sh_eval_backward_dev", "gwbp_sh_eval_backward_blocks")


def test_header_declares_the_entry_points_and_the_library_exports_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gwbp.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"GWBP_API int {name}\s*\(", src), name
        assert name in _lib.ARGTYPES and name in _lib.EXPORTS
    assert "gwbp_*" in open(os.path.join(ROOT, "3dgs-gradient-backprojection_amd", "csrc", "gwbp.map")).read()
    gsbp_amd.build()
    assert all(hasattr(_lib.lib(), n) for n in NAMES)
    for name in ("sh_eval_dev", "sh_eval_backward_dev"):
        assert callable(getattr(gsbp_amd.Engine, name)), name
    assert gsbp_amd.PoseAdjust is PoseAdjust


def test_blocks_are_the_workgroups_of_256():
    lib = _lib.lib()
    assert [lib.gwbp_sh_eval_backward_blocks(n) for n in (0, 1, 255, 256, 257, 1000, 1_000_000)] == [0, 1, 1, 1, 2, 4, 3907]
    assert lib.gwbp_sh_eval_backward_blocks((1 << 31) - 1) == 1 << 23
    assert lib.gwbp_sh_eval_backward_blocks(-1) == -1 and "Gaussians" in lib.gwbp_last_error_string().decode()
    assert lib.gwbp_sh_eval_backward_blocks(1 << 31) == -1


def test_capi_rejects_without_a_launch():
    """Host memory stands in for every array: a call that got as far as a launch would fault or report a HIP error, not -1 with the
    message that is checked."""
    lib = _lib.lib()
    buf = (C.c_float * 8192)()
    a = C.addressof(buf)
    assert a % 8 == 0

    def message():
        return lib.gwbp_last_error_string().decode()

    def ev(n=4, degree=3, kh=1, kt=15, means=a, head=a + 256, tail=a + 1024, campos=a + 4096, out=a + 8192):
        return lib.gwbp_sh_eval_dev(n, degree, kh, kt, means, head, tail, campos, out, None)

    def bw(n=4, degree=3, kh=1, kt=15, means=a, head=a + 256, tail=a + 1024, campos=a + 4096, v=a + 8192, vh=a + 9216, vt=a + 10240,
           vm=a + 12288, vc=a + 16384, scratch=a + 20480):
        return lib.gwbp_sh_eval_backward_dev(n, degree, kh, kt, means, head, tail, campos, v, vh, vt, vm, vc, scratch, None)

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
        assert fn(campos=a + 4098) == -1 and "4-B" in message()
        for null in ("means", "head"):
            assert fn(**{null: None}) == -1 and "null" in message(), null
        assert fn(means=a + 2) == -1 and fn(head=a + 257) == -1 and fn(tail=a + 1026) == -1 and "4-B" in message()
    assert ev(out=None) == -1 and "null out" in message()
    assert ev(out=a + 8193) == -1 and "4-B" in message()
    assert ev(out=a) == -1 and "input" in message()
    assert ev(out=a + 4096) == -1 and "input" in message()      # out is campos
    assert bw(vh=None, vt=None, vm=None, vc=None) == -1 and "every output" in message()
    assert bw(v=None) == -1 and "v_colors" in message()
    assert bw(kh=16, kt=0, tail=None) == -1 and "v_tail" in message()
    assert bw(scratch=None) == -1 and "scratch" in message()
    for i, k in enumerate(("v", "vh", "vt", "vm")):
        assert bw(**{k: a + 8193 + 1024 * i}) == -1 and "4-B" in message(), k
    assert bw(vc=a + 16388) == -1 and "8-B" in message()
    assert bw(scratch=a + 20484) == -1 and "8-B" in message()
    assert bw(vh=a + 256) == -1 and "input" in message()        # v_head is head
    assert bw(vt=a + 1024) == -1 and "input" in message()       # v_tail is tail
    assert bw(vm=a) == -1 and bw(vh=a + 8192) == -1             # v_means is means, v_head is v_colors
    assert bw(vc=a + 4096) == -1 and "input" in message()       # v_campos is campos
    assert bw(scratch=a + 8192) == -1 and "input" in message()  # the scratch is v_colors
    assert bw(vh=a + 9216, vt=a + 9216) == -1 and "same array" in message()
    assert bw(vc=a + 20480) == -1 and "same array" in message()  # v_campos is the scratch
    # nothing to do: no launch (without v_campos not even a HIP call)
    assert ev(n=0, kh=16, kt=0, means=None, head=None, tail=None, out=None) == 0
    assert bw(n=0, kh=16, kt=0, means=None, head=None, tail=None, v=None, vt=None, vc=None, scratch=None) == 0
    del buf


def _transform(table_row, identity):
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = rotation_6d(table_row[3:] + identity)
    T[:3, 3] = table_row[:3]
    return T


def test_pose_adjust_is_the_inverse_of_the_reference_product():
    """The reference right-multiplies the camera-to-world matrix by T = [R | dx]; apply() must give that camera's view matrix."""
    gen = torch.Generator().manual_seed(11)
    adj = PoseAdjust(5, dtype=torch.float64).random_init(0.2, seed=4)
    again = PoseAdjust(5, dtype=torch.float64).random_init(0.2, seed=4)
    assert torch.equal(adj.table, again.table) and bool(adj.table.any())
    assert not torch.equal(adj.table, PoseAdjust(5, dtype=torch.float64).random_init(0.2, seed=5).table)
    vms = torch.stack([gsbp_amd.se3_exp(torch.randn(6, generator=gen, dtype=torch.float64)) for _ in range(5)])
    for v in range(5):
        T = _transform(adj.table[v], adj.identity)
        R = T[:3, :3]
        assert (R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-14 and abs(float(torch.det(R)) - 1.0) < 1e-14
        want = torch.linalg.inv(torch.linalg.inv(vms[v]) @ T)
        assert (adj.apply(vms[v], v) - want).abs().max() <= 1e-12
        assert (adj.apply_all(vms)[v] - want).abs().max() <= 1e-12
    assert (rigid_inverse(vms) - torch.linalg.inv(vms)).abs().max() <= 1e-12


def test_pose_adjust_is_the_identity_at_zero():
    gen = torch.Generator().manual_seed(12)
    for dtype in (torch.float64, torch.float32):
        vm = gsbp_amd.se3_exp(torch.randn(6, generator=gen, dtype=torch.float64)).to(dtype)
        adj = PoseAdjust(3, dtype=dtype)
        assert adj.table.shape == (3, 9) and adj.table.dtype == dtype and not adj.table.any()
        assert torch.equal(adj.apply(vm, 1), vm) and torch.equal(adj.apply_all(vm[None].expand(3, 4, 4)), vm[None].expand(3, 4, 4))
        assert torch.equal(adj.random_init(0.1).zero_init().apply(vm, 2), vm)
    # the gradient at zero exists and is finite (Gram-Schmidt of (1, 0, 0), (0, 1, 0))
    adj = PoseAdjust(2, dtype=torch.float64)
    adj.table.requires_grad_(True)
    adj.apply(vm.double(), 0).square().sum().backward()
    assert torch.isfinite(adj.table.grad).all() and bool(adj.table.grad[0].any()) and not adj.table.grad[1].any()
    with pytest.raises(ValueError):
        PoseAdjust(0)


def test_pose_training_schedules_its_rate_and_monitors_the_error():
    """PoseTraining on the CPU (plain torch): the noise alone leaves a constant error; a step toward the truth lowers it; the rate of
    step s is lr * 0.01 ** (s / steps)."""
    gen = torch.Generator().manual_seed(13)
    vms = torch.stack([gsbp_amd.se3_exp(torch.randn(6, generator=gen, dtype=torch.float64)) for _ in range(4)]).float()
    fixed = PoseTraining(vms, 10, 7, False, 1e-5, 1e-6, 0.05)
    assert fixed.view(2) is not None and not fixed.view(2).requires_grad
    for s in range(3):
        fixed.step(s)
    h = fixed.history()
    assert len(set(h["pose_err"])) == 1 and h["pose_err"][0] > 0 and "pose_adjust" not in h and h["viewmats"].shape == (4, 4, 4)
    assert not torch.equal(h["viewmats"], vms)
    both = PoseTraining(vms, 10, 7, True, 1e-2, 0.0, 0.05)
    rates = []
    for s in range(10):
        vm = both.view(s % 4)
        assert vm.requires_grad
        (vm - vms[s % 4]).square().sum().backward()  # pull the used view toward the true one
        both.step(s)
        rates.append(both.opt.param_groups[0]["lr"])
    assert rates == [1e-2 * 0.01 ** (s / 10) for s in range(10)]
    h = both.history()
    assert h["pose_err"][-1] < h["pose_err"][0] == fixed.history()["pose_err"][0]
    assert h["pose_adjust"].shape == (4, 9) and bool(h["pose_adjust"].any()) and not h["pose_adjust"].requires_grad
    plain = PoseTraining(vms, 10, 7, True, 1e-2, 0.0, 0.0).history()
    assert "pose_err" not in plain and torch.equal(plain["viewmats"], vms)


def test_cpu_tensors_and_bad_arguments_raise():
    sc = gsbp_amd.synthetic.make_scene(gsbp_amd.synthetic.CONFIGS["T0"])
    sc["features_dc"], sc["features_rest"] = torch.zeros(512, 1, 3), torch.zeros(512, 15, 3)
    eye, K = torch.eye(4)[None], torch.eye(3)

    def train(views=eye, **kw):
        return gsbp_amd.train_scene(sc, views, K, 96, 64, lambda v: None, 10, **kw)

    for name in ("pose_opt_lr", "pose_opt_reg", "pose_noise"):
        for bad in (-1e-3, float("nan"), float("inf"), "0.1", True, None):
            with pytest.raises(gsbp_amd.GwbpError, match=name):
                train(pose_opt=True, **{name: bad})
    for bad in (1, "yes", None):
        with pytest.raises(gsbp_amd.GwbpError, match="pose_opt must be a bool"):
            train(pose_opt=bad)
    for kw in (dict(pose_opt=True), dict(pose_noise=0.1)):
        with pytest.raises(gsbp_amd.GwbpError, match="at least one view"):
            train(views=eye[:0], **kw)
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):  # (good values get as far as the device check)
        train(pose_opt=True, pose_noise=0.1)
    m, c = torch.zeros(5, 3), torch.zeros(5, 16, 3)
    with pytest.raises(gsbp_amd.GwbpError, match="no CPU path"):
        gsbp_amd.sh_colors(3, m, c, torch.zeros(3), campos_grad=True)
