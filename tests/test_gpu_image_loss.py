"""The photometric loss on the GPU (csrc/ssim.hip through Engine.image_loss and gsbp_amd.photometric): the SSIM map and the gradient
against the float64 torch restatement of the contract (tests/image_loss_ref.py) in the project's floor rule, the sums and the
tiling-independence exactly, autograd into rasterization(), refine_pose(loss="photometric") and run_polish.py.

Floor rule, per figure (Frobenius, max-abs):  |kernel - truth| <= FACTOR x max(|float32 restatement on the CPU - truth|, 2^-24 x the
figure of truth).  FACTOR = ceil(2 x the largest ratio measured on an MI355X) over every case below; tools/record_image_loss.py
measures them and writes profiles/image_loss.json.  The ceiling is 16: tests/test_image_loss_ref_cpu.py shows that a broken contract
sits at 1e5 and more.
"""
import json
import math
import os
import sys

import pytest
import torch

import gsbp_amd
import image_loss_ref as ref
from gsbp_amd import photometric, rasterization
from gsbp_amd.pose import pose_error
from gsbp_amd.rasterization import engine_on

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 6  # ceil(2 x 2.552), the largest ratio of profiles/image_loss.json "errors" (a gradient's max-abs at 45 x 201 x 4, "same")
# 2 x the largest relative difference of the final pose errors between the kernel loss and the torch float32 loss over the 8 repeats
# of profiles/image_loss.json "refine_pose" (1.778e-4; rasterization()'s backward adds with float atomics: the runs differ among
# themselves), rounded down
POSE_MARGIN = 3.5e-4
TY, TX = photometric.SSIM_TILE
SHAPES = [(11, 11), (12, 43), (TY + 10, TX + 10), (TY + 11, TX + 11), (2 * TY + 13, 3 * TX + 9)]
SAME_ONLY = [(1, 1), (3, 5), (10, 64)]
CASES = [(s, p) for s in SHAPES for p in ("valid", "same")] + [(s, "same") for s in SAME_ONLY]
DIMS = (1, 3, 4)
LAMBDAS = (0.0, 0.2, 1.0)


def kernel_ratios(dev, H, W, D, padding, weighted, lam, seed=0):
    """The four ratios of the floor rule for one case: (map Frobenius, map max-abs, gradient Frobenius, gradient max-abs)."""
    x, y = ref.smooth_pair(H, W, D, seed)
    w = ref.smooth_weights(H, W, seed) if weighted else None
    _, smap, grad = engine_on(dev).image_loss(x.to(dev), y.to(dev), lam, padding, pixel_weights=None if w is None else w.to(dev),
                                              want_map=True, want_grad=True)
    _, g64 = ref.stored_map_backward(x, y, lam, padding, w)
    _, g32 = ref.stored_map_backward(x, y, lam, padding, w, dtype=torch.float32)
    m64, m32 = ref.ssim_map(x, y, padding), ref.ssim_map(x, y, padding, torch.float32)
    assert smap.shape == m64.shape and grad.shape == g64.shape
    return ref.floor_ratios(smap.cpu(), m64, m32) + ref.floor_ratios(grad.cpu(), g64, g32)


def all_cases():
    for (H, W), padding in CASES:
        for D in DIMS:
            for weighted in (False, True):
                for lam in LAMBDAS:
                    yield H, W, D, padding, weighted, lam
    yield 12, 43, 32, "valid", True, 0.2
    yield 12, 43, 32, "same", False, 0.2


@pytest.mark.parametrize("shape,padding", CASES)
def test_map_and_gradient_against_float64(dev, shape, padding):
    worst = [0.0] * 4
    for D in DIMS:
        for weighted in (False, True):
            for lam in LAMBDAS:
                r = kernel_ratios(dev, *shape, D, padding, weighted, lam)
                worst = [max(a, b) for a, b in zip(worst, r)]
                assert max(r) <= FACTOR, (shape, padding, D, weighted, lam, r)
    print(f"{shape} {padding}: worst ratios map {worst[0]:.3f} / {worst[1]:.3f}, gradient {worst[2]:.3f} / {worst[3]:.3f}")


@pytest.mark.parametrize("padding,weighted", [("valid", True), ("same", False)])
def test_thirty_two_channels(dev, padding, weighted):
    r = kernel_ratios(dev, 12, 43, 32, padding, weighted, 0.2)
    print(f"D = 32 {padding}: ratios {r}")
    assert max(r) <= FACTOR


def run(dev, x, y, lam=0.2, padding="valid", w=None, **kw):
    return engine_on(dev).image_loss(x, y, lam, padding, pixel_weights=w, want_map=True, want_grad=True, **kw)


@pytest.mark.parametrize("padding", ["valid", "same"])
def test_sums_are_the_float64_sums(dev, padding):
    """Summation order is the only difference: 1e-12 relative.  With weights the products w t are float64 products of float32 values."""
    H, W, D = 2 * TY + 13, 3 * TX + 9, 3
    x, y = (t.to(dev) for t in ref.smooth_pair(H, W, D, 4))
    for w in (None, ref.smooth_weights(H, W, 4).to(dev)):
        table, smap, _ = run(dev, x, y, 0.2, padding, w)
        wd = torch.ones(H, W, device=dev, dtype=torch.float64) if w is None else w.double()
        wv = ref.crop(wd, padding)
        e = x - y  # float32 per element, as the kernel forms it
        want = [(wv[..., None] * smap.double()).sum(), (wd[..., None] * e.abs().double()).sum(), (wd[..., None] * (e * e).double()).sum(),
                wv.sum(), wd.sum(), torch.tensor(float(wv.numel())), torch.tensor(float(H * W)), torch.tensor(float(D))]
        for k, (got, exp) in enumerate(zip(table.cpu().tolist(), [float(v) for v in want])):
            assert abs(got - exp) <= 1e-12 * abs(exp), (padding, w is not None, k, got, exp)
        loss = float(photometric.photometric_loss(x, y, 0.2, padding, w))
        t = table.cpu().tolist()
        exp = 0.8 * t[1] / (D * t[4]) + 0.2 * (1 - t[0] / (D * t[3]))
        assert abs(loss - exp) <= 2.0 ** -23 * abs(exp)
        m = photometric.image_metrics(x, y, w, padding)
        assert m["mse"] == t[2] / (D * t[4]) and m["psnr"] == -10 * math.log10(m["mse"]) and m["ssim"] == t[0] / (D * t[3])
        assert torch.equal(photometric.image_sums(x, y, w, padding), table)
    assert torch.equal(photometric.ssim_map(x, y, padding), smap)


def test_the_map_of_a_crop_is_the_crop_of_the_map(dev):
    """Bit for bit: a blur's chain belongs to its output pixel, not to the tile that computes it.  The offsets move every tile boundary."""
    H, W, D = 2 * TY + 13, 3 * TX + 9, 3
    x, y = (t.to(dev) for t in ref.smooth_pair(H, W, D, 5))
    full = photometric.ssim_map(x, y)
    for a, b, c, d in ((3, H - 1, 7, W - 2), (TY - 1, H, TX + 1, W), (0, 11, 0, 11), (1, TY + 12, 9, TX + 30)):
        part = photometric.ssim_map(x[a:b, c:d], y[a:b, c:d])
        assert torch.equal(part, full[a:b - 10, c:d - 10]), (a, b, c, d)


@pytest.mark.parametrize("padding", ["valid", "same"])
def test_identical_images(dev, padding):
    x = ref.smooth_pair(TY + 11, TX + 11, 3, 6)[0].to(dev)
    x[:4, :9] = 0.0  # a black corner: zero windows
    loss = photometric.photometric_loss(x.clone().requires_grad_(True), x, 0.2, padding)
    assert float(loss.detach()) == 0.0
    table, smap, grad = run(dev, x, x.clone(), 0.2, padding)
    assert torch.equal(smap, torch.ones_like(smap))
    t = table.cpu().tolist()
    assert t[0] / (3 * t[3]) == 1.0 and t[1] == 0.0 and t[2] == 0.0
    assert torch.isfinite(grad).all()
    assert photometric.image_metrics(x, x, padding=padding)["psnr"] == math.inf


def test_strided_inputs_give_the_bits_of_their_copies(dev):
    H, W = TY + 11, TX + 11
    x, y = (t.to(dev) for t in ref.smooth_pair(H, W, 4, 7))
    w = ref.smooth_weights(H, W, 7).to(dev)
    base = run(dev, x[..., :3].contiguous(), y[..., :3].contiguous(), 0.2, "valid", w)
    wide_y = torch.cat([y, y, y], dim=-1)  # pixel stride 12 for y, 4 for x
    wide_w = torch.stack([w, w], dim=-1)[..., 1]
    gout = torch.zeros(H, W, 5, device=dev)
    got = run(dev, x[..., :3], wide_y[..., :3], 0.2, "valid", wide_w, grad_out=gout[..., :3])
    for a, b in zip(base, got):
        assert torch.equal(a, b)
    assert got[2].data_ptr() == gout.data_ptr() and not gout[..., 3:].any()
    for dt in (torch.float16, torch.bfloat16):
        assert all(torch.equal(a, b) for a, b in zip(run(dev, x[..., :3], y[..., :3], 0.2, "same", w.to(dt)),
                                                       run(dev, x[..., :3], y[..., :3], 0.2, "same", w.to(dt).float())))
    mask = w > 0.5
    assert all(torch.equal(a, b) for a, b in zip(run(dev, x, y, 0.2, "same", mask), run(dev, x, y, 0.2, "same", mask.float())))
    # a transposed image has no flat rows: it is copied once
    xt, yt = x.transpose(0, 1), y.transpose(0, 1)
    assert all(torch.equal(a, b) for a, b in zip(run(dev, xt, yt), run(dev, xt.contiguous(), yt.contiguous())))


def test_two_runs_give_the_same_bits(dev):
    H, W = 2 * TY + 13, 3 * TX + 9
    x, y = (t.to(dev) for t in ref.smooth_pair(H, W, 3, 8))
    w = ref.smooth_weights(H, W, 8).to(dev)
    first = [t.clone() for t in run(dev, x, y, 0.2, "same", w)]
    run(dev, y, x, 0.7, "valid")  # (another call on the same workspace in between)
    second = run(dev, x, y, 0.2, "same", w)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize("padding", ["valid", "same"])
def test_all_zero_weights(dev, padding):
    x, y = (t.to(dev) for t in ref.smooth_pair(20, 30, 3, 9))
    w = torch.zeros(20, 30, device=dev)
    xr = x.clone().requires_grad_(True)
    loss = photometric.photometric_loss(xr, y, 0.2, padding, w)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not xr.grad.any()
    # the weights of the border only: under "valid" no window has weight, and the L1 term alone remains
    w[0] = 1.0
    table, _, grad = run(dev, x, y, 0.2, "valid", w)
    assert table[3].item() == 0.0 and table[4].item() == 30.0
    lam = float(torch.tensor(0.2, dtype=torch.float32))  # (lambda reaches the kernel as a float32)
    s_1 = torch.tensor((1.0 - lam) / (3 * 30.0), dtype=torch.float32, device=dev)
    assert not grad[1:].any() and torch.equal(grad[0], s_1 * torch.sign(x[0] - y[0]))


def test_what_raises(dev):
    x, y = (t.to(dev) for t in ref.smooth_pair(10, 64, 3, 1))
    with pytest.raises(gsbp_amd.GwbpError, match="11"):
        photometric.photometric_loss(x, y)
    assert float(photometric.photometric_loss(x, y, padding="same")) > 0
    with pytest.raises(gsbp_amd.GwbpError):
        photometric.photometric_loss(x, y[:, :, :2], padding="same")
    with pytest.raises(gsbp_amd.GwbpError):
        photometric.photometric_loss(x.double(), y.double(), padding="same")
    with pytest.raises(gsbp_amd.GwbpError):
        photometric.photometric_loss(x, y.clone().requires_grad_(True), padding="same")
    wide = torch.zeros(12, 12, 33, device=dev)
    with pytest.raises(gsbp_amd.GwbpError, match="33"):
        photometric.photometric_loss(wide, wide)


# ---- autograd ------------------------------------------------------------------------------------------------------------------------
def t0_render(dev, requires_grad=True):
    from gsbp_amd import synthetic as syn
    cfg = syn.CONFIGS["T0"]
    gauss = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    colors = torch.rand(cfg.n_gaussians, 3, generator=torch.Generator().manual_seed(31)).to(dev).requires_grad_(requires_grad)
    vms, K = syn.make_cameras(cfg).to(dev), syn.intrinsics(cfg).to(dev)
    with torch.no_grad():
        target = rasterization(*gauss, colors.detach(), vms[1:2], K[None], cfg.width, cfg.height, want_meta=False)[0]
    out = rasterization(*gauss, colors, vms[0:1], K[None], cfg.width, cfg.height, want_meta=False)[0]
    return out, target, colors


@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_the_rasteriser_receives_the_kernel_gradient(dev, scale):
    out, target, colors = t0_render(dev)
    seen = []
    # (the hook sits on the [H, W, 3] render: `batch[0]` of a one-camera call IS that tensor, with no autograd node in between)
    out[0].register_hook(lambda g: seen.append(g.clone()))
    loss = photometric.photometric_loss(out, target)
    (scale * loss).backward()
    _, _, grad = engine_on(dev).image_loss(out[0].detach(), target[0], 0.2, "valid", want_grad=True)
    assert len(seen) == 1 and seen[0].shape == out.shape[1:] and grad.abs().max() > 0
    assert torch.equal(seen[0], scale * grad)
    assert colors.grad is not None and torch.isfinite(colors.grad).all() and colors.grad.abs().max() > 0


def test_second_order_uses_the_literal_expression(dev):
    x, y = (t.to(dev) for t in ref.smooth_pair(14, 17, 2, 2))
    xr = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(photometric.photometric_loss(xr, y), xr, create_graph=True)
    assert g.requires_grad
    _, _, grad = engine_on(dev).image_loss(x, y, 0.2, "valid", want_grad=True)
    assert float((g.detach() - grad).norm() / grad.norm()) < 1e-4
    (g * g).sum().backward()
    assert torch.isfinite(xr.grad).all()


def test_a_batch_is_the_mean_of_its_images(dev):
    a, b = ref.smooth_pair(16, 20, 3, 3), ref.smooth_pair(16, 20, 3, 4)
    x, y = torch.stack([a[0], b[0]]).to(dev), torch.stack([a[1], b[1]]).to(dev)
    got = photometric.photometric_loss(x, y)
    each = [photometric.photometric_loss(x[i], y[i]) for i in range(2)]
    assert torch.equal(got, torch.stack(each).mean())


# ---- refine_pose(loss="photometric") -------------------------------------------------------------------------------------------------
def refine_both(dev):
    """refine_pose on the existing camera test's case under the kernel loss and under the torch float32 restatement of it; returns the
    two (angle, distance) pairs, the start's, and the kernel run's result."""
    import camera_grad_ref as cg
    from gsbp_amd import pose
    from test_gpu_camera_grad import gpu_refine
    case = cg.pose_case()
    res_k = gpu_refine(dev, case, loss="photometric")
    kernel_loss = pose.pose_loss
    pose.pose_loss = lambda out, target, weights, loss, lam: ref.loss_of(out, target, lam, "valid", weights, torch.float32)
    try:
        res_t = gpu_refine(dev, case, loss="photometric")
    finally:
        pose.pose_loss = kernel_loss
    start = pose_error(case["vm0"], case["vm_true"])
    return pose_error(res_k["viewmat"], case["vm_true"]), pose_error(res_t["viewmat"], case["vm_true"]), start, res_k


def relative_difference(a, b):
    return max(abs(p - q) / max(abs(q), 1e-300) for p, q in zip(a, b))


def test_refine_pose_photometric(dev):
    end_k, end_t, start, res = refine_both(dev)
    diff = relative_difference(end_k, end_t)
    print(f"refine_pose(photometric): angle {start[0]:.5f} -> {end_k[0]:.5f}, distance {start[1]:.5f} -> {end_k[1]:.5f}; "
          f"torch float32 loss: {end_t[0]:.5f}, {end_t[1]:.5f}; relative difference {diff:.3e}")
    assert res["history"][-1] < res["history"][0]
    assert end_k[0] < start[0] and end_k[1] < start[1]
    assert diff <= min(POSE_MARGIN, 0.10)


# ---- run_polish.py -------------------------------------------------------------------------------------------------------------------
def test_run_polish_synthetic(dev, tmp_path):
    sys.path.insert(0, ROOT)
    import run_polish
    assert run_polish.main(["--synthetic", "T0", "--steps", "40", "--out", str(tmp_path)]) == 0
    history = json.load(open(tmp_path / "history.json"))["history"]
    metrics = json.load(open(tmp_path / "metrics.json"))
    assert len(history) == 40 and history[-1] < history[0]
    assert metrics["after"]["mean"]["psnr"] > metrics["before"]["mean"]["psnr"]
    assert len(metrics["after"]["views"]) == 2 and os.path.exists(tmp_path / "polished.pt")
