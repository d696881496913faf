"""render_latents: gradients w.r.t. means, quats, scales, opacities and a latent table of 48 and 128 channels against the dense float64
yardstick (tests/raster_grad_ref.py), by the floor rule and factor of tests/test_gpu_raster_grad.py: per gradient tensor, the
Frobenius-relative and the max-abs error against the float64 run may be FACTOR = 4 times what the float32 run of the same
restatement has.  The loss is sum(render G) + sum(alpha A) with seeded G and A, on T0 (512 Gaussians, 96 x 64).
"""
import functools

import pytest
import torch

import gsbp_amd
import raster_grad_ref as rg
from gsbp_amd import GwbpError, render_latents
from test_gpu_raster_grad import FACTOR, _t0
from util import rel_row_err

pytestmark = pytest.mark.gpu
DIMS = (48, 128)


@functools.lru_cache(maxsize=None)
def reference(d, view=0):
    """The case, the kernels' cut, G, A and the yardstick's float64 and float32 gradients: computed once, shared, never modified."""
    case = _t0(d, view=view)
    dev = torch.device("cuda:0")
    cut = rg.kernel_cut(dev, *case["inputs"][:4], case["vm"], case["K"], case["W"], case["H"])
    g = torch.Generator().manual_seed(211 + d)
    G, A = torch.randn(case["H"], case["W"], d, generator=g), torch.randn(case["H"], case["W"], generator=g)
    truth, _, _ = rg.gradients(torch.float64, case["inputs"], G, A, case["vm"], case["K"], case["W"], case["H"], cut)
    floor, _, _ = rg.gradients(torch.float32, case["inputs"], G, A, case["vm"], case["K"], case["W"], case["H"], cut)
    return dict(case=case, G=G, A=A, truth=truth, floor=floor)


def _leaves(dev, case):
    return [t.to(dev).requires_grad_(True) for t in case["inputs"]]


def _loss(dev, ref, ins):
    case = ref["case"]
    out, alpha = render_latents(*ins, case["vm"].to(dev), case["K"].to(dev), case["W"], case["H"])
    assert out.shape == (case["H"], case["W"], ins[4].shape[1]) and alpha.shape == (case["H"], case["W"])
    return (out * ref["G"].to(dev)).sum() + (alpha * ref["A"].to(dev)).sum()


def _check(name, kernel, ref):
    rows = rg.report(name, [g.cpu() for g in kernel], ref["truth"], ref["floor"])
    for r in rows:
        print(f"{name:14s} {r['tensor']:9s} floor {r['floor_fro']:.2e} / {r['floor_max']:.2e}   kernel {r['kernel_fro']:.2e} / "
              f"{r['kernel_max']:.2e}   ratio {r['kernel_fro'] / max(r['floor_fro'], 1e-300):.2f} / "
              f"{r['kernel_max'] / max(r['floor_max'], 1e-300):.2f}")
    assert len(rows) == 5 and all(float(t.abs().max()) > 0 for t in ref["truth"])
    bad = [r for r in rows if r["kernel_fro"] > FACTOR * r["floor_fro"] or r["kernel_max"] > FACTOR * r["floor_max"]]
    assert not bad, bad


@pytest.mark.parametrize("d", DIMS)
def test_all_five_gradients(dev, d):
    ref = reference(d)
    ins = _leaves(dev, ref["case"])
    _check(f"latents-{d}", torch.autograd.grad(_loss(dev, ref, ins), ins), ref)


@pytest.mark.parametrize("d", DIMS)
def test_latent_gradient_is_the_scatter_of_the_view(dev, d):
    """v_latents against Engine.scatter of G on an engine of the test's own, as test_colour_only_path_is_unchanged compares."""
    ref = reference(d)
    case = ref["case"]
    n, W, H = case["inputs"][0].shape[0], case["W"], case["H"]
    g = [t.to(dev) for t in case["inputs"][:4]]
    eng = gsbp_amd.Engine(n, W, H, device=dev)
    view = eng.view(case["vm"], case["K"], W, H)
    eng.project(view, *g)
    eng.bin_sort(view)
    eng.blend_weights(view)
    want = torch.zeros(n, d, device=dev)
    eng.scatter(view, ref["G"].to(dev), want, None)
    latents = case["inputs"][4].to(dev).requires_grad_(True)
    out, _ = render_latents(*g, latents, case["vm"].to(dev), case["K"].to(dev), W, H)
    (out * ref["G"].to(dev)).sum().backward()
    assert float(want.abs().max()) > 0 and rel_row_err(latents.grad.cpu().numpy(), want.cpu().numpy()) <= 1e-4


def test_backward_after_another_call_reused_the_engine(dev):
    """Both views' forwards first (the second reuses the workspace), then both backwards: each matches its own view."""
    refs = [reference(48, 0), reference(48, 1)]
    leaves = [_leaves(dev, r["case"]) for r in refs]
    losses = [_loss(dev, r, ins) for r, ins in zip(refs, leaves)]
    for v, (r, loss, ins) in enumerate(zip(refs, losses, leaves)):
        _check(f"stale-view-{v}", torch.autograd.grad(loss, ins), r)


def test_refusals(dev):
    case = _t0(8)
    g = [t.to(dev) for t in case["inputs"][:4]]
    vm, K, W, H = case["vm"].to(dev), case["K"].to(dev), case["W"], case["H"]
    n = g[0].shape[0]
    with pytest.raises(GwbpError, match="1 <= d <= 128"):
        render_latents(*g, torch.zeros(n, 129, device=dev), vm, K, W, H)
    with pytest.raises(GwbpError, match="float32"):
        render_latents(*g, torch.zeros(n, 16, device=dev, dtype=torch.float16), vm, K, W, H)
    with pytest.raises(GwbpError, match="HIP tensors"):
        render_latents(*[t.cpu() for t in g], torch.zeros(n, 16), vm.cpu(), K.cpu(), W, H)
    with pytest.raises(GwbpError, match="HIP tensors"):
        render_latents(*g, torch.zeros(n, 16), vm, K, W, H)
