"""The SH colours with the camera centre on the device, and the centre's gradient (csrc/sh.hip: k_sh_eval_dev, k_sh_eval_bwd_dev,
k_sh_campos_sum).

Bits.  For the same three floats gwbp_sh_eval_dev gives gwbp_sh_eval's bits and gwbp_sh_eval_backward_dev gives
gwbp_sh_eval_backward's v_head, v_tail and v_means bits, on tests/sh_grad_ref.py's cases (the row at the camera centre included).

v_campos.  Floor rule of tests/sh_campos_ref.py, per figure (Frobenius, max-abs) of the three numbers:
|kernel - truth| <= FACTOR x max(|float32 CPU autograd - truth|, 2^-24 |truth|).  FACTOR = ceil(2 x the largest ratio measured on an
MI355X) over every case of cases(); tools/time_sh_campos_grad.py measures them with this file's own functions and writes
profiles/sh_campos_grad.json "errors".
Consistency, a derived bound: the kernel adds the float32 v_means values widened to double, at most 1000 of them, so
|v_campos + sum_i double(v_means_i)| <= 1e-12 x sum_i |v_means_i| per component (a double sum of at most 1000 terms errs by less than
1000 x 2^-53 = 1.1e-13 of sum |.|), the sum taken on the CPU over the kernel's own v_means.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import sh_campos_ref as cref  # noqa: E402
import sh_grad_ref as ref  # noqa: E402
import test_gpu_sh_grad as tsg  # noqa: E402  (its cases' sizes, its placement of inputs and its guarded outputs)

import gsbp_amd  # noqa: E402
from gsbp_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
FACTOR = 6  # ceil(2 x 2.5705), the largest ratio of profiles/sh_campos_grad.json "errors" (max-abs at N = 256, degree 3, K = 16)
SIZES = (1, 255, 256, 257, 1000)  # the workgroup's 256 rows: one row, one short, exact, one over (a second workgroup of one row), several
DEGREE_K = tsg.DEGREE_K
CONSISTENCY = 1e-12


def layouts(k):
    """(name, K_head, whether every array sits 4 B behind a 16-B boundary): one table and the dict's split, each both ways."""
    out = [("single", k, False), ("single-shifted", k, True)]
    if k > 1:
        out += [("split-1", 1, False), ("split-1-shifted", 1, True)]
    return out


def cases():
    return [(n, d, k, name, k_head, shifted) for n in SIZES for d, k in DEGREE_K for name, k_head, shifted in layouts(k)]


@functools.lru_cache(maxsize=None)
def reference(n, degree, k):
    """The case with the centre as a leaf, its float64 truth and float32 floor (CPU): computed once, shared, never modified."""
    case = cref.make_case(n, degree, k, seed=n)
    return case, cref.autograd(case, torch.float64), cref.autograd(case, torch.float32)


class GuardedDouble:
    """tsg.Guarded for a float64 output: PAD guard doubles each side."""

    def __init__(self, shape, dev):
        self.size = int(np.prod(shape))
        self.buf = torch.full((self.size + 2 * tsg.PAD,), 7.0, device=dev, dtype=torch.float64)
        self.view = self.buf[tsg.PAD:tsg.PAD + self.size].view(shape)
        self.ptr = C.c_void_p(self.view.data_ptr())

    def result(self):
        b = self.buf.cpu()
        assert bool((b[:tsg.PAD] == 7.0).all()) and bool((b[tsg.PAD + self.size:] == 7.0).all()), "a guard row was written"
        return b[tsg.PAD:tsg.PAD + self.size].view(self.view.shape).numpy().copy()


def raw_call(dev, case, k_head, shifted, want_means=True, want_tables=True, want_campos=True):
    """gwbp_sh_eval_dev and gwbp_sh_eval_backward_dev through the C ABI on guarded outputs (the scratch guarded too) ->
    dict(colors, v_coeffs, v_means, v_campos) in numpy."""
    n, k = case["coeffs"].shape[:2]
    means, v = tsg.place(case["means"], dev, shifted), tsg.place(case["v_colors"], dev, shifted)
    head = tsg.place(case["coeffs"][:, :k_head], dev, shifted)
    tail = tsg.place(case["coeffs"][:, k_head:], dev, shifted) if k_head < k else None
    cp = tsg.place(case["campos"], dev, shifted)
    colors = tsg.Guarded((n, 3), dev, shifted)
    v_head = tsg.Guarded((n, k_head, 3), dev, shifted) if want_tables else None
    v_tail = tsg.Guarded((n, k - k_head, 3), dev, shifted) if want_tables and tail is not None else None
    v_means = tsg.Guarded((n, 3), dev, shifted) if want_means else None
    lib = _lib.lib()
    blocks = lib.gwbp_sh_eval_backward_blocks(n)
    assert blocks == (n + 255) // 256
    v_campos = GuardedDouble((3,), dev) if want_campos else None
    scratch = GuardedDouble((blocks, 3), dev) if want_campos else None
    p = lambda g: None if g is None else g.ptr  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.gwbp_sh_eval_dev(n, case["degree"], k_head, k - k_head, _lib.ptr(means), _lib.ptr(head), _lib.ptr(tail), _lib.ptr(cp),
                                    colors.ptr, stream), "gwbp_sh_eval_dev")
    _lib.check(lib.gwbp_sh_eval_backward_dev(n, case["degree"], k_head, k - k_head, _lib.ptr(means), _lib.ptr(head), _lib.ptr(tail),
                                             _lib.ptr(cp), _lib.ptr(v), p(v_head), p(v_tail), p(v_means), p(v_campos), p(scratch),
                                             stream), "gwbp_sh_eval_backward_dev")
    torch.cuda.synchronize(dev)
    out = dict(colors=colors.result())
    if want_tables:
        out["v_coeffs"] = np.concatenate([v_head.result()] + ([v_tail.result()] if v_tail is not None else []), axis=1)
    if want_means:
        out["v_means"] = v_means.result()
    if want_campos:
        out["v_campos"] = v_campos.result()
        scratch.result()  # (its guards)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def measure(dev, n, degree, k, k_head, shifted):
    """{figure: ratio} of one case's v_campos, after its exact properties and the consistency bound."""
    case, truth, floor = reference(n, degree, k)
    got = raw_call(dev, case, k_head, shifted)
    if degree == 0:
        assert same_bits(got["v_campos"], np.zeros(3)), "v_campos at degree 0 is not exact +0"
    vm = got["v_means"].astype(np.float64)
    gap, scale = np.abs(got["v_campos"] + vm.sum(axis=0)), np.abs(vm).sum(axis=0)
    assert (gap <= CONSISTENCY * scale).all(), (n, degree, k, gap, scale)
    # v_campos asked for alone has the bits it has beside the others, and the others have theirs without it
    alone = raw_call(dev, case, k_head, shifted, want_means=False, want_tables=False)
    assert same_bits(alone["v_campos"], got["v_campos"])
    without = raw_call(dev, case, k_head, shifted, want_campos=False)
    assert same_bits(without["v_means"], got["v_means"]) and same_bits(without["v_coeffs"], got["v_coeffs"])
    return cref.campos_ratios(got["v_campos"], truth["v_campos"], floor["v_campos"])


@pytest.mark.parametrize("n", SIZES)
def test_v_campos_against_float64_by_the_floor_rule(dev, n):
    worst = (0.0, None)
    for _, d, k, name, k_head, shifted in [c for c in cases() if c[0] == n]:
        r = measure(dev, n, d, k, k_head, shifted)
        for fig, v in r.items():
            worst = (v, (d, k, name, fig)) if v >= worst[0] else worst
            assert v <= FACTOR, (n, d, k, name, fig, v)
    print(f"N = {n}: largest kernel / floor ratio of v_campos {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("n", SIZES)
def test_the_device_centre_gives_the_bits_of_the_host_centre(dev, n):
    """Forward, v_head, v_tail and v_means against gwbp_sh_eval and gwbp_sh_eval_backward, on sh_grad_ref's own cases: the Gaussian at
    the camera centre (row 0) is one of the rows.  v_campos then holds that row's 1e11 and is only checked for consistency."""
    for d, k in DEGREE_K:
        case, _, _ = tsg.reference(n, d, k)
        for name, k_head, shifted in layouts(k):
            want = tsg.raw_call(dev, case, k_head, shifted)
            got = raw_call(dev, case, k_head, shifted)
            for key in ("colors", "v_coeffs", "v_means"):
                assert same_bits(got[key], want[key]), (n, d, k, name, key)
            vm = got["v_means"].astype(np.float64)
            assert np.isfinite(got["v_campos"]).all()
            assert (np.abs(got["v_campos"] + vm.sum(axis=0)) <= CONSISTENCY * np.abs(vm).sum(axis=0)).all(), (n, d, k, name)


def test_two_runs_give_equal_bits(dev):
    case, _, _ = reference(1000, 3, 16)
    a, b = raw_call(dev, case, 1, False), raw_call(dev, case, 1, False)
    for key in a:
        assert same_bits(a[key], b[key]), key
    assert np.abs(a["v_campos"]).min() > 0


def test_sh_colors_autograd_returns_the_kernels_results(dev):
    """sh_colors(campos_grad=True) under autograd: the Engine pair's results, v_campos cast to float32 for a centre that requires grad,
    through a function of a view matrix as render_splats builds it; campos_grad=False with a tensor keeps the old result and gives the
    tensor no gradient."""
    case, truth, floor = reference(257, 2, 16)
    eng = gsbp_amd.Engine(257, 32, 32, device=dev)
    v = tsg.place(case["v_colors"], dev, False)
    means = tsg.place(case["means"], dev, False).requires_grad_(True)
    dc = tsg.place(case["coeffs"][:, :1], dev, False).requires_grad_(True)
    rest = tsg.place(case["coeffs"][:, 1:], dev, False).requires_grad_(True)
    cp = tsg.place(case["campos"], dev, False).requires_grad_(True)
    out = gsbp_amd.sh_colors(2, means, dc, cp, rest=rest, campos_grad=True)
    out.backward(v)
    det = [t.detach() for t in (means, dc, rest, cp)]
    vh, vt, vm, vc = eng.sh_eval_backward_dev(2, *det, v)
    assert vc.dtype == torch.float64 and vc.shape == (3,)
    assert torch.equal(dc.grad, vh) and torch.equal(rest.grad, vt) and torch.equal(means.grad, vm)
    assert cp.grad.dtype == torch.float32 and torch.equal(cp.grad, vc.float())
    assert torch.equal(out.detach().view(torch.int32), eng.sh_eval_dev(2, *det).view(torch.int32))
    assert max(cref.campos_ratios(vc.cpu().numpy(), truth["v_campos"], floor["v_campos"]).values()) <= FACTOR
    # the host route on the same three floats: the same bits forward and backward
    old = gsbp_amd.sh_colors(2, det[0], det[1], case["campos"].tolist(), rest=det[2])
    assert torch.equal(old.view(torch.int32), out.detach().view(torch.int32))
    vh0, vt0, vm0 = eng.sh_eval_backward(2, det[0], det[1], det[2], case["campos"].tolist(), v)
    assert torch.equal(vh0, vh) and torch.equal(vt0, vt) and torch.equal(vm0, vm)
    # only the centre asks: one output, the same bits
    only = eng.sh_eval_backward_dev(2, *det, v, want_head=False, want_tail=False, want_means=False)
    assert only[:3] == (None, None, None) and torch.equal(only[3], vc)
    cp2 = det[3].clone().requires_grad_(True)
    gsbp_amd.sh_colors(2, det[0], det[1], cp2, rest=det[2], campos_grad=True).backward(v)
    assert torch.equal(cp2.grad, vc.float())
    # a centre that is a function of a view matrix: the chain continues into it
    vmat = torch.eye(4, device=dev)
    vmat[:3, 3] = -det[3]
    vmat.requires_grad_(True)
    gsbp_amd.sh_colors(2, det[0], det[1], -(vmat[:3, :3].T @ vmat[:3, 3]), rest=det[2], campos_grad=True).backward(v)
    assert torch.allclose(vmat.grad[:3, 3], -vc.float(), rtol=1e-6, atol=0) and bool(vmat.grad[:3, :3].any())
    # a detached centre under campos_grad=True: no v_campos is computed, the rest as before
    m3 = det[0].clone().requires_grad_(True)
    gsbp_amd.sh_colors(2, m3, det[1], det[3], rest=det[2], campos_grad=True).backward(v)
    assert torch.equal(m3.grad, vm)
    # degree 0: exact +0 to the centre
    cp0 = det[3].clone().requires_grad_(True)
    d0 = det[1].clone().requires_grad_(True)
    gsbp_amd.sh_colors(0, det[0], d0, cp0, rest=det[2], campos_grad=True).backward(v)
    assert not cp0.grad.view(torch.int32).any() and bool(d0.grad.any())
    # campos_grad=False with a tensor: read on the host, detached -- the old result, no gradient
    cp3 = det[3].clone().requires_grad_(True)
    m4 = det[0].clone().requires_grad_(True)
    plain = gsbp_amd.sh_colors(2, m4, det[1], cp3, rest=det[2])
    plain.backward(v)
    assert torch.equal(plain.detach().view(torch.int32), old.view(torch.int32)) and cp3.grad is None and torch.equal(m4.grad, vm)
    # what campos_grad=True refuses
    for bad in (case["campos"].tolist(), det[3].cpu(), det[3].double(), torch.zeros(4, device=dev)):
        with pytest.raises(gsbp_amd.GwbpError, match="campos must be a float32 HIP tensor of three"):
            gsbp_amd.sh_colors(2, det[0], det[1], bad, rest=det[2], campos_grad=True)
