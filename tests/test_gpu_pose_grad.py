"""render_splats(pose_grad=True) and render_latents(camera_grad=True): a training step that differentiates with respect to its camera.

The yardstick (tests/pose_sh_ref.py) is the dense float64 render of tests/raster_grad_ref.py with the view matrix as a sixth leaf and
the SH colours' camera centre a function of it; the rule is tests/test_gpu_raster_grad.py's own: kernel error <= its FACTOR x the float32
run of the same restatement, per tensor, Frobenius-relative and max-abs.  The case is T0 with [N, 16, 3] coefficients at degree 2.

That the comparison can fail: the same yardstick with the centre DETACHED -- what rasterization(camera_grad=True) gave beside colours
whose centre was read on the host -- must break the rule for the view matrix, and the test asserts that it does (4e-2 against a floor
of 6e-7 with tests/camera_grad_ref.py's fixed cut on the CPU; the kernels' cut here gives figures of the same size).
"""
import functools
import os
import sys

import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import pose_sh_ref as psr  # noqa: E402
import raster_grad_ref as rg  # noqa: E402
import test_gpu_raster_grad as trg  # noqa: E402  (its T0 scene, its weights, its FACTOR and its check)
from test_gpu_camera_grad import rows_of  # noqa: E402

import gsbp_amd  # noqa: E402
from gsbp_amd.latent_render import render_latents  # noqa: E402
from gsbp_amd.polish import render_splats  # noqa: E402
from gsbp_amd.rasterization import set_sh_kernel, sh_kernel_enabled  # noqa: E402

pytestmark = pytest.mark.gpu
FACTOR, check = trg.FACTOR, trg.check


@functools.lru_cache(maxsize=None)
def reference():
    """The case, the kernels' cut, G, A and the yardstick's six gradients in float64, in float32 and in float64 with the centre
    detached: computed once, shared, never modified."""
    case = psr.case_of(trg._t0(sh=True))
    dev = torch.device("cuda:0")
    args = (case["vm"], case["K"], case["W"], case["H"])
    cut = rg.kernel_cut(dev, *case["inputs"][:4], *args)
    G, A = trg._weights(case)
    truth = psr.gradients(torch.float64, case["inputs"], G, A, *args, cut)
    floor = psr.gradients(torch.float32, case["inputs"], G, A, *args, cut)
    detached = psr.gradients(torch.float64, case["inputs"], G, A, *args, cut, attached=False)
    return dict(case=case, G=G, A=A, truth=truth, floor=floor, detached=detached)


def splat_leaves(dev, case, leaves=True):
    """(splats, geometry, the five tensors in the yardstick's order with the coefficients as (dc, rest)): the activated geometry is
    handed to render_splats as leaves, so that the gradients are the yardstick's (w.r.t. scales and opacities, not their logs)."""
    means, quats, scales, opac = (t.to(dev).requires_grad_(leaves) for t in case["inputs"][:4])
    dc = case["inputs"][4][:, :1].contiguous().to(dev).requires_grad_(leaves)
    rest = case["inputs"][4][:, 1:].contiguous().to(dev).requires_grad_(leaves)
    splats = dict(means=means, rotation=quats, features_dc=dc, features_rest=rest)
    return splats, (means, quats, scales, opac), (means, quats, scales, opac, dc, rest)


def kernel_gradients(dev, ref, leaves=True, **kw):
    """The six gradients of render_splats(pose_grad=True) (None for tensors that are no leaves)."""
    case = ref["case"]
    splats, geometry, ins = splat_leaves(dev, case, leaves)
    vm = case["vm"].to(dev).requires_grad_(True)
    image, alpha = render_splats(splats, vm, case["K"].to(dev), case["W"], case["H"], sh_degree=psr.SH_DEGREE, geometry=geometry,
                                 return_alpha=True, pose_grad=True, **kw)
    loss = (image * ref["G"].to(dev)).sum() + (alpha[..., 0] * ref["A"].to(dev)).sum()
    loss.backward()
    assert vm.grad.dtype == torch.float32 and vm.grad.shape == (4, 4) and not vm.grad[3].any()
    if not leaves:
        assert all(t.grad is None for t in ins)
        return [None] * 5 + [vm.grad.cpu()]
    coeffs = torch.cat([ins[4].grad, ins[5].grad], dim=1)
    return [t.grad.cpu() for t in ins[:4]] + [coeffs.cpu(), vm.grad.cpu()]


def test_the_detached_centre_is_outside_the_rule():
    """The condition under which the next test means something (pure CPU arithmetic on the shared reference)."""
    ref = reference()
    outside, figures = psr.detached_is_outside(ref["truth"], ref["floor"], ref["detached"], FACTOR)
    print(figures)
    assert outside, figures
    assert figures["detached_fro"] > 1000 * FACTOR * figures["floor_fro"]
    # the other five do not depend on where the centre's gradient goes
    for i in range(5):
        assert torch.equal(ref["detached"][i], ref["truth"][i]), psr.NAMES[i]


def test_all_six_gradients_against_the_yardstick(dev):
    ref = reference()
    assert float(ref["truth"][5].abs().max()) > 0 and not ref["truth"][5][3].any()
    kernel = kernel_gradients(dev, ref)
    assert not kernel[4][:, 9:].any() and bool(kernel[4][:, :9].any())  # the coefficient rows above degree 2: zeros
    check(rows_of("pose+sh", kernel, ref["truth"], ref["floor"]))
    # ... and the same kernel result is NOT the detached yardstick's: the colours' share is in it
    (kfro, _), (dfro, _) = rg.errors(kernel[5], ref["truth"][5]), rg.errors(kernel[5], ref["detached"][5])
    assert dfro > 1000 * kfro, (kfro, dfro)


def test_camera_only(dev):
    """Only the view matrix requires grad: the same gradient by the same rule, and nothing else gets a .grad."""
    ref = reference()
    kernel = kernel_gradients(dev, ref, leaves=False)
    check(rows_of("pose-only", kernel, ref["truth"], ref["floor"], tensors=[5]))


def test_the_torch_colours_are_the_other_side(dev):
    """set_sh_kernel(False): sh_colors_torch with the attached centre, by the same rule."""
    ref = reference()
    before = sh_kernel_enabled()
    try:
        set_sh_kernel(False)
        kernel = kernel_gradients(dev, ref)
    finally:
        set_sh_kernel(before)
    check(rows_of("pose+sh torch", kernel, ref["truth"], ref["floor"]))


def test_a_detached_view_is_the_plain_call(dev):
    """pose_grad=True under no_grad, or with a viewmat that does not require grad, has the plain call's bits; camera_grad=True without
    pose_grad keeps its refusal; means2d_grad goes along with pose_grad."""
    ref = reference()
    case = ref["case"]
    K, W, H = case["K"].to(dev), case["W"], case["H"]
    splats, geometry, _ = splat_leaves(dev, case, leaves=False)
    vm = case["vm"].to(dev)
    kw = dict(sh_degree=psr.SH_DEGREE, geometry=geometry)
    plain = render_splats(splats, vm, K, W, H, **kw)
    posed = render_splats(splats, vm, K, W, H, pose_grad=True, **kw)
    assert torch.equal(plain.view(torch.int32), posed.view(torch.int32)) and bool(plain.any()) and not posed.requires_grad
    leaf = vm.clone().requires_grad_(True)
    with torch.no_grad():
        quiet = render_splats(splats, leaf, K, W, H, pose_grad=True, **kw)
    assert torch.equal(plain.view(torch.int32), quiet.view(torch.int32))
    attached = render_splats(splats, leaf, K, W, H, pose_grad=True, **kw)
    assert attached.requires_grad and float((attached.detach() - plain).abs().max()) <= 1e-5  # (the centre computed on the device: same image)
    with pytest.raises(NotImplementedError, match="camera_grad=True with sh_degree"):
        render_splats(splats, leaf, K, W, H, camera_grad=True, **kw)
    image, meta = render_splats(splats, leaf, K, W, H, pose_grad=True, return_meta=True, means2d_grad=True, **kw)
    image.sum().backward()
    assert bool(leaf.grad.any()) and bool(meta["means2d"].grad.any()) and int((meta["radii"] > 0).sum()) > 300


@pytest.mark.parametrize("d", [8, 32])
def test_render_latents_returns_the_projections_view_gradient(dev, d, monkeypatch):
    """render_latents(camera_grad=True): viewmat.grad is Engine.project_backward(want_viewmat=True) on the v_g2d its own backward
    computed (captured, because that array is summed with float atomics and differs from run to run in its last bits), cast to
    float32; the Gaussians' gradients are what they are without the keyword; without it a viewmat that requires grad is refused."""
    ref = reference()
    case = ref["case"]
    K, W, H = case["K"].to(dev), case["W"], case["H"]
    g = torch.Generator().manual_seed(40 + d)
    latents = torch.randn(case["inputs"][0].shape[0], d, generator=g).to(dev)
    G, A = torch.randn(H, W, d, generator=g).to(dev), torch.randn(H, W, generator=g).to(dev)
    geo = [t.to(dev).requires_grad_(True) for t in case["inputs"][:4]]
    vm = case["vm"].to(dev).requires_grad_(True)
    seen = []
    original = gsbp_amd.Engine.render_dots_backward

    def spy(self, *args, **kw):
        seen.append((self, original(self, *args, **kw)))
        return seen[-1][1]
    monkeypatch.setattr(gsbp_amd.Engine, "render_dots_backward", spy)
    out, alpha = render_latents(*geo, latents, vm, K, W, H, camera_grad=True)
    ((out * G).sum() + (alpha * A).sum()).backward()
    assert len(seen) == 1
    eng, v_g2d = seen[0]
    view = eng.view(vm.detach(), K, W, H)
    want = eng.project_backward(view, *[t.detach() for t in geo], v_g2d, needs=(True,) * 4, want_viewmat=True)
    assert vm.grad.dtype == torch.float32 and vm.grad.shape == (4, 4) and not vm.grad[3].any() and bool(vm.grad[:3].any())
    assert torch.equal(vm.grad, want[4].float())
    for t, w in zip(geo, want[:4]):
        assert torch.equal(t.grad, w)
    # without the keyword: refused in the backward, as before; with it and a detached viewmat: nothing for the view
    out, alpha = render_latents(*[t.detach().requires_grad_(True) for t in geo], latents, vm.detach().requires_grad_(True), K, W, H)
    with pytest.raises(NotImplementedError, match="viewmat"):
        ((out * G).sum() + (alpha * A).sum()).backward()
    quiet = vm.detach().clone()
    out, alpha = render_latents(*[t.detach().requires_grad_(True) for t in geo], latents, quiet, K, W, H, camera_grad=True)
    ((out * G).sum() + (alpha * A).sum()).backward()
    assert quiet.grad is None
    with pytest.raises(NotImplementedError, match="K"):
        Kl = K.clone().requires_grad_(True)
        out, alpha = render_latents(*geo, latents, vm, Kl, W, H, camera_grad=True)
        ((out * G).sum() + (alpha * A).sum()).backward()
