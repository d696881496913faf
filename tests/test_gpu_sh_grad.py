"""The SH colours' kernel pair on the device (csrc/sh.hip): k_sh_eval against k_sh_colors bit for bit, k_sh_eval_bwd
against sh_colors_torch under autograd in float64 by the floor rule of tests/sh_grad_ref.py, its exact properties, the route through
rasterization(), render_splats on the split tables, and the SH degree schedule of polish_scene and train_scene.

Floor rule, per tensor and figure (Frobenius, max-abs):  |kernel - truth| <= FACTOR x max(|float32 restatement on the CPU - truth|,
2^-24 x the figure of truth).  FACTOR = ceil(2 x the largest ratio measured on an MI355X) over every case of gradient_cases();
tools/time_sh_grad.py measures them with this file's own functions and writes profiles/sh_grad.json "errors".
"""
import ctypes as C
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import raster_grad_ref as rg  # noqa: E402
import sh_grad_ref as ref  # noqa: E402
import test_gpu_raster_grad as trg  # noqa: E402  (its T0 scene, its two sides and its FACTOR rule)

import gsbp_amd  # noqa: E402
from gsbp_amd import _lib  # noqa: E402
from gsbp_amd.polish import render_splats  # noqa: E402

rz = importlib.import_module("gsbp_amd.rasterization")  # (gsbp_amd.rasterization is the function)
pytestmark = pytest.mark.gpu
FACTOR = 5  # ceil(2 x 2.097), the largest ratio of profiles/sh_grad.json "errors" (v_means' max-abs at N = 257, degree 1, K = 4)
SIZES = (1, 255, 256, 257, 1000)  # the workgroup's 256 rows: one short, exact, one over, several
DEGREE_K = [(d, k) for d in range(4) for k in sorted({(d + 1) ** 2, 16})]
PAD = 64  # guard floats around every output


@functools.lru_cache(maxsize=None)
def reference(n, degree, k):
    """The case with its float64 truth and float32 floor (CPU): computed once, shared, never modified."""
    case = ref.make_case(n, degree, k, seed=n)
    if n > 1:  # the promises of the inputs (tests/test_sh_grad_cpu.py has them for its own N)
        clamped, edge = ref.case_facts(case)
        assert clamped >= 0.2 and edge >= ref.EDGE, (clamped, edge)
    return case, ref.autograd(case, torch.float64), ref.autograd(case, torch.float32)


def layouts(k):
    """(name, K_head, whether the tables sit 4 B behind a 16-B boundary)."""
    out = [("single", k, False), ("slice", k, True)]
    if k > 1:
        out += [("split-1", 1, False), ("split-1-slice", 1, True)]
    if k > 4:
        out.append(("split-4", 4, False))
    return out


def place(t, dev, shifted):
    """t on the device, contiguous; shifted: as the [1:] slice of a flat buffer one float longer (4-B aligned, not 16-B aligned)."""
    t = torch.as_tensor(t)
    if not shifted:
        return t.to(dev).contiguous()
    flat = torch.empty(t.numel() + 1, device=dev)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


class Guarded:
    """An output array between PAD guard floats each side, 4 B behind a 16-B boundary when shifted."""

    def __init__(self, shape, dev, shifted):
        self.size = int(np.prod(shape))
        self.at = PAD + (1 if shifted else 0)
        self.buf = torch.full((self.size + 2 * PAD + 1,), 7.0, device=dev)
        self.view = self.buf[self.at:self.at + self.size].view(shape)
        self.ptr = C.c_void_p(self.view.data_ptr())

    def result(self):
        b = self.buf.cpu()
        assert bool((b[:self.at] == 7.0).all()) and bool((b[self.at + self.size:] == 7.0).all()), "a guard row was written"
        return b[self.at:self.at + self.size].view(self.view.shape).numpy().copy()


def raw_call(dev, case, k_head, shifted, want_means=True, want_tables=True):
    """gwbp_sh_eval and gwbp_sh_eval_backward through the C ABI on guarded outputs -> dict(colors, v_coeffs, v_means) in numpy."""
    n, k = case["coeffs"].shape[:2]
    means, v = place(case["means"], dev, shifted), place(case["v_colors"], dev, shifted)
    head = place(case["coeffs"][:, :k_head], dev, shifted)
    tail = place(case["coeffs"][:, k_head:], dev, shifted) if k_head < k else None
    cp = (C.c_float * 3)(*case["campos"].tolist())
    colors = Guarded((n, 3), dev, shifted)
    v_head = Guarded((n, k_head, 3), dev, shifted) if want_tables else None
    v_tail = Guarded((n, k - k_head, 3), dev, shifted) if want_tables and tail is not None else None
    v_means = Guarded((n, 3), dev, shifted) if want_means else None
    p = lambda g: None if g is None else g.ptr  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib = _lib.lib()
    _lib.check(lib.gwbp_sh_eval(n, case["degree"], k_head, k - k_head, _lib.ptr(means), _lib.ptr(head), _lib.ptr(tail), cp, colors.ptr,
                                stream), "gwbp_sh_eval")
    _lib.check(lib.gwbp_sh_eval_backward(n, case["degree"], k_head, k - k_head, _lib.ptr(means), _lib.ptr(head), _lib.ptr(tail), cp,
                                         _lib.ptr(v), p(v_head), p(v_tail), p(v_means), stream), "gwbp_sh_eval_backward")
    torch.cuda.synchronize(dev)
    out = dict(colors=colors.result())
    if want_tables:
        parts = [v_head.result()] + ([v_tail.result()] if v_tail is not None else [])
        out["v_coeffs"] = np.concatenate(parts, axis=1)
    if want_means:
        out["v_means"] = v_means.result()
    return out


def gradient_cases():
    return [(n, d, k, name, k_head, shifted) for n in SIZES for d, k in DEGREE_K for name, k_head, shifted in layouts(k)]


def measure(dev, n, degree, k, k_head, shifted):
    """{(tensor, figure): ratio} of one case, after its exact properties."""
    case, truth, floor = reference(n, degree, k)
    got = raw_call(dev, case, k_head, shifted)
    nb = (degree + 1) ** 2
    assert not got["v_coeffs"][:, nb:].view(np.uint32).any(), "rows above the degree are not exact +0"
    if degree == 0:
        assert not got["v_means"].view(np.uint32).any()
    ref.check_row0(case, got)
    # each output is nullable on its own, and what is still written has the same bits
    only_means = raw_call(dev, case, k_head, shifted, want_tables=False)
    only_tables = raw_call(dev, case, k_head, shifted, want_means=False)
    assert np.array_equal(only_means["v_means"].view(np.uint32), got["v_means"].view(np.uint32))
    assert np.array_equal(only_tables["v_coeffs"].view(np.uint32), got["v_coeffs"].view(np.uint32))
    if n == 1:  # (row 0 is the whole case: checked above, nothing left for the norms)
        return {}
    return ref.ratios(got, truth, floor)


@pytest.mark.parametrize("n", SIZES)
def test_gradients_against_float64_by_the_floor_rule(dev, n):
    worst = (0.0, None)
    for _, d, k, name, k_head, shifted in [c for c in gradient_cases() if c[0] == n]:
        r = measure(dev, n, d, k, k_head, shifted)
        for key, v in r.items():
            worst = max(worst, (v, (d, k, name) + key))
            assert v <= FACTOR, (n, d, k, name, key, v)
    print(f"N = {n}: largest kernel / floor ratio {worst[0]:.3f} at {worst[1]}")


def test_two_runs_give_equal_bits(dev):
    case, _, _ = reference(1000, 3, 16)
    a, b = raw_call(dev, case, 1, False), raw_call(dev, case, 1, False)
    for key in a:
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key


@pytest.mark.parametrize("n", SIZES)
def test_forward_has_the_bits_of_sh_colors(dev, n):
    eng = gsbp_amd.Engine(max(n, 1), 32, 32, device=dev)
    for d, k in DEGREE_K:
        case, _, _ = reference(n, d, k)
        means, table = place(case["means"], dev, False), place(case["coeffs"], dev, False)
        want = eng.sh_colors(d, means, table, case["campos"].tolist()).cpu()
        assert torch.equal(want.view(torch.int32), eng.sh_eval(d, means, table, None, case["campos"].tolist()).cpu().view(torch.int32))
        for name, k_head, shifted in layouts(k):
            got = raw_call(dev, case, k_head, shifted)["colors"]
            assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32)), (d, k, name)
            if k_head < k and not shifted:
                split = eng.sh_eval(d, means, table[:, :k_head].contiguous(), table[:, k_head:].contiguous(), case["campos"].tolist())
                assert torch.equal(split.cpu().view(torch.int32), want.view(torch.int32))


def test_sh_colors_autograd_asks_for_what_is_needed(dev):
    """gsbp_amd.sh_colors under autograd: the Engine pair's results, gradients only where they are needed, zeros (not None) for the
    rows above the degree, nothing for the means at degree 0."""
    case, truth, floor = reference(257, 2, 16)
    cp = case["campos"].tolist()
    eng = gsbp_amd.Engine(257, 32, 32, device=dev)
    v = place(case["v_colors"], dev, False)
    means = place(case["means"], dev, False).requires_grad_(True)
    dc = place(case["coeffs"][:, :1], dev, False).requires_grad_(True)
    rest = place(case["coeffs"][:, 1:], dev, False).requires_grad_(True)
    out = gsbp_amd.sh_colors(2, means, dc, cp, rest=rest)
    out.backward(v)
    vh, vt, vm = eng.sh_eval_backward(2, means.detach(), dc.detach(), rest.detach(), cp, v)
    assert torch.equal(dc.grad, vh) and torch.equal(rest.grad, vt) and torch.equal(means.grad, vm)
    assert not rest.grad[:, 8:].any() and bool(rest.grad[:, :8].any())
    got = dict(colors=out.detach().cpu().numpy(), v_coeffs=torch.cat([vh, vt], dim=1).cpu().numpy(), v_means=vm.cpu().numpy())
    assert max(ref.ratios(got, truth, floor).values()) <= FACTOR
    assert eng.sh_eval_backward(2, means.detach(), dc.detach(), rest.detach(), cp, v, want_head=False, want_means=False)[::2] == (None, None)
    # one table, only the coefficients; then only the means
    table = place(case["coeffs"], dev, False).requires_grad_(True)
    gsbp_amd.sh_colors(2, means.detach(), table, cp).backward(v)
    assert torch.equal(table.grad, torch.cat([vh, vt], dim=1))
    m2 = means.detach().clone().requires_grad_(True)
    gsbp_amd.sh_colors(2, m2, table.detach(), cp).backward(v)
    assert torch.equal(m2.grad, vm)
    # degree 0: the means get None or zeros
    m0 = means.detach().clone().requires_grad_(True)
    d0 = dc.detach().clone().requires_grad_(True)
    gsbp_amd.sh_colors(0, m0, d0, cp, rest=rest.detach()).backward(v)
    assert m0.grad is None or not m0.grad.any()
    assert bool(d0.grad.any())
    # what it refuses
    with pytest.raises(gsbp_amd.GwbpError, match="float32"):
        gsbp_amd.sh_colors(2, means.detach().double(), table.detach(), cp)
    with pytest.raises(gsbp_amd.GwbpError, match="fewer"):
        gsbp_amd.sh_colors(3, means.detach(), table.detach()[:, :9], cp)
    with pytest.raises(gsbp_amd.GwbpError, match="degree"):
        gsbp_amd.sh_colors(4, means.detach(), table.detach(), cp)


# ---- through rasterization() -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raster_reference():
    """T0 with [N, 16, 3] coefficients at sh_degree = 2: the float64 truth and float32 floor of tests/raster_grad_ref.py."""
    case = dict(trg._t0(sh=True), sh_degree=2)
    dev = torch.device("cuda:0")
    cut = rg.kernel_cut(dev, *case["inputs"][:4], case["vm"], case["K"], case["W"], case["H"])
    G, A = trg._weights(case)
    kw = dict(sh_degree=2, campos=(-(case["vm"][:3, :3].T @ case["vm"][:3, 3])).tolist())
    truth, _, _ = rg.gradients(torch.float64, case["inputs"], G, A, case["vm"], case["K"], case["W"], case["H"], cut, **kw)
    floor, _, _ = rg.gradients(torch.float32, case["inputs"], G, A, case["vm"], case["K"], case["W"], case["H"], cut, **kw)
    return dict(case=case, G=G, A=A, truth=truth, floor=floor)


def test_rasterization_takes_the_kernels_and_matches_the_torch_route(dev):
    r = raster_reference()
    rows = {}
    before = rz._SH_KERNEL
    try:
        for on in (True, False):
            rz.set_sh_kernel(on)
            kernel = trg.kernel_gradients(dev, r["case"], r["G"], r["A"])
            rows[on] = rg.report(f"sh-2 kernel={on}", kernel, r["truth"], r["floor"])
            assert not kernel[4][:, 9:].any() and bool(kernel[4][:, :9].any())  # the coefficient rows above degree 2: zeros
    finally:
        rz.set_sh_kernel(before)
    for on in (True, False):
        for row in rows[on]:
            print(row)
        trg.check(rows[on])


def splats_of_t0(dev, degree=3, seed=5):
    cfg, sc = trg.scene_np("T0")
    g = torch.Generator().manual_seed(seed)
    n = cfg.n_gaussians
    return cfg, sc, dict(means=sc["means"].to(dev), rotation=sc["quats"].to(dev), scaling=torch.log(sc["scales"]).to(dev),
                         opacity=torch.logit(sc["opac"].clamp(1e-4, 1 - 1e-4)).to(dev),
                         features_dc=(0.5 * torch.randn(n, 1, 3, generator=g)).to(dev),
                         features_rest=(0.3 * torch.randn(n, (degree + 1) ** 2 - 1, 3, generator=g)).to(dev))


def test_render_splats_has_the_bits_of_the_concatenated_call(dev):
    cfg, sc, splats = splats_of_t0(dev)
    vm, K = sc["vms"][1].to(dev), sc["K"].to(dev)
    with torch.no_grad():
        got = render_splats(splats, vm, K, cfg.width, cfg.height)
        cat = torch.cat([splats["features_dc"], splats["features_rest"]], dim=1)
        want = gsbp_amd.rasterization(splats["means"], splats["rotation"], torch.exp(splats["scaling"]), torch.sigmoid(splats["opacity"]),
                                      cat, vm[None], K[None], cfg.width, cfg.height, sh_degree=3)[0][0]
        low = render_splats(splats, vm, K, cfg.width, cfg.height, sh_degree=1)
        want_low = gsbp_amd.rasterization(splats["means"], splats["rotation"], torch.exp(splats["scaling"]),
                                          torch.sigmoid(splats["opacity"]), cat, vm[None], K[None], cfg.width, cfg.height, sh_degree=1)[0][0]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and bool(got.any())
    assert torch.equal(low.view(torch.int32), want_low.view(torch.int32)) and not torch.equal(low, got)
    with pytest.raises(NotImplementedError, match="camera_grad=True with sh_degree"):
        render_splats(splats, vm.clone().requires_grad_(True), K, cfg.width, cfg.height, camera_grad=True)
    with pytest.raises(gsbp_amd.GwbpError, match="sh_degree must be"):
        render_splats(splats, vm, K, cfg.width, cfg.height, sh_degree=4)


# ---- the schedule ----------------------------------------------------------------------------------------------------------------
def training_setup(dev):
    """test_gpu_densify's T0 setup with a degree-3 table whose higher rows start at zero, as init_splats_from_points leaves them."""
    from test_gpu_densify import t0_training_setup
    cfg, start, K, vms, images = t0_training_setup(dev)
    start = dict(start, features_rest=torch.zeros(start["means"].shape[0], 15, 3, device=dev))
    return cfg, start, K, vms, images


def test_the_schedule_leaves_unused_rows_alone(dev):
    cfg, start, K, vms, images = training_setup(dev)

    def polish(steps):
        return gsbp_amd.polish_scene(start, vms, K, cfg.width, cfg.height, lambda v: images[v], params=("sh0", "shN"), steps=steps,
                                     sh_degree_interval=5)[0]
    four, seven = polish(4), polish(7)
    zero = start["features_rest"].view(torch.int32)
    assert torch.equal(four["features_rest"].view(torch.int32), zero)  # degree 0: zero gradients, and Adam leaves the bits
    assert not torch.equal(four["features_dc"], start["features_dc"])
    moved = seven["features_rest"].view(torch.int32) != zero
    assert bool(moved[:, :3].any()) and not bool(moved[:, 3:].any())  # steps 5 and 6 at degree 1: rows 0 .. 2 of features_rest
    _, history = gsbp_amd.train_scene(start, vms, K, cfg.width, cfg.height, lambda v: images[v], 18, params=("sh0", "shN"),
                                      sh_degree_interval=5)
    assert history["sh_degree"] == [min(s // 5, 3) for s in range(18)] and len(history["loss"]) == 18
    _, plain = gsbp_amd.train_scene(start, vms, K, cfg.width, cfg.height, lambda v: images[v], 3, params=("sh0",))
    assert plain["sh_degree"] == [3, 3, 3]


def test_no_interval_is_the_call_without_the_keyword(dev):
    """sh_degree_interval=None gives the loss bits of the call without the keyword, on the two-tile crop of
    test_gpu_mcmc.py::test_the_default_path_is_unchanged, where training is reproducible by construction (the reason is given there)."""
    cfg, start, K, vms, images = training_setup(dev)
    w, h = 32, 16
    x0, y0 = (cfg.width - w) // 2, (cfg.height - h) // 2
    Kc = K.clone()
    Kc[0, 2] -= x0
    Kc[1, 2] -= y0
    crops = [im[y0:y0 + h, x0:x0 + w].contiguous() for im in images]
    plain = gsbp_amd.train_scene(start, vms, Kc, w, h, lambda v: crops[v], 40, seed=3)[1]
    none = gsbp_amd.train_scene(start, vms, Kc, w, h, lambda v: crops[v], 40, seed=3, sh_degree_interval=None)[1]
    assert len(plain["loss"]) == 40 and plain["loss"] == none["loss"] and plain["n"] == none["n"]
    assert plain["loss"][-1] < plain["loss"][0] and len(set(plain["loss"])) == 40
    a = gsbp_amd.polish_scene(start, vms, Kc, w, h, lambda v: crops[v], params=("opacities", "sh0", "shN"), steps=20, seed=3)[1]
    b = gsbp_amd.polish_scene(start, vms, Kc, w, h, lambda v: crops[v], params=("opacities", "sh0", "shN"), steps=20, seed=3,
                              sh_degree_interval=None)[1]
    assert a == b and len(set(a)) == 20


def test_the_command_line_tools_take_the_interval(dev, tmp_path):
    """run_train.py and run_polish.py --sh-degree-interval, in process.  --synthetic T0 carries a degree-0 table there, so the schedule
    stays at min(s // 5, 0) = 0 (the degrees above are test_the_schedule_leaves_unused_rows_alone's): what is checked is that the
    option reaches the trainers and the history file."""
    import json

    import run_polish
    import run_train
    out = str(tmp_path / "train")
    assert run_train.main(["--synthetic", "T0", "--steps", "12", "--sh-degree-interval", "5", "--out", out]) == 0
    with open(os.path.join(out, "history.json")) as f:
        hist = json.load(f)
    assert hist["sh_degree"] == [0] * 12 and len(hist["loss"]) == 12
    assert run_polish.main(["--synthetic", "T0", "--steps", "7", "--sh-degree-interval", "5", "--out", str(tmp_path / "polish")]) == 0
    for tool in (run_train, run_polish):
        assert "1000" in tool.build_parser().format_help().split("--sh-degree-interval")[-1][:400]
