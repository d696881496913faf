"""The depth-loss kernels on the device (csrc/depth_loss.hip) against tests/depth_loss_ref.py.

Renders of 13 x 19 pixels (no dimension a multiple of anything) with 4 channels (depth in channel 3: the 16-B paths of the map
kernels), 3 channels (channel 2) and 1 channel (channel 0); M in {0, 1, B - 1, B, B + 1, 4 B + 3} points, B = GWBP_DEPTH_BLOCK.

THE BOUND of the gradient maps (not a tuned tolerance).  A pixel's value is the sum of the shares that met there.  One share of
v_alpha is -((v_e A) / (a a)) with v_e = (gy gx) v_d, v_d = -(sgn (q q) c), q = 1 / d, d = gy (gx e00 + fx e01) + fy (gx e10 + fx e11),
e = A / max(a, 1e-10), c = upstream * (float)(scale / M); fx and fy are exact (x - floor(x)), every e and every weight is >= 0, so
nothing cancels and relative errors add to first order.  Roundings: gx, gy (1 each, into d: 2) + e (1) + the two products and the
sum of a row (3) + the two products and the sum of d (3): d carries 9; q = 1 / d: 10; q q: 21; c: 2 (the float64 quotient's
rounding and the product with upstream), (q q) c: 24; gy gx: 3 more with its own rounding, times v_d: 28 less the two of gx, gy
counted twice = 26; v_e A, a a, the quotient: 28 (v_render's share, v_e / am, has 26).  The n shares of a pixel are gathered by n
float32 atomic adds, each rounding a partial sum that is at most sum |shares|.  So, per pixel, with the shares of the float64 chain:

    |kernel - float64| <= (n + 28) 2^-24 sum |shares|            (depth_loss_ref.grad_bound, CHAIN = 28)

which also holds where the restatement (no atomics: a float64 gather of float32 shares) is compared.  A pixel no point touches, and
every channel but the depth's, holds exact zeros.  The map term has one share per pixel and no adds: its gradients are compared BIT
FOR BIT with the restatement, given the scalar c formed from the device's own float64 sum of the weights.

AUTOGRAD FACTOR.  rasterization(render_mode="RGB+D") of T0's first view, depth_point_loss at 300 seeded points, backward: the
gradients at the render and alpha leaves against the literal torch statement in float32 on the device (the floor) with its float64
evaluation as the truth, figures max-abs and Frobenius, points with d = 0 left out (torch is NaN there; the test asserts they are at
most 10 %; 0.3 % here).  Measured on an MI355X, fused error / floor: render 9.27e-4 (max-abs: 1.761e2 against 1.899e5) and 9.28e-4
(Frobenius), alpha 4.66e-4 and 4.88e-4 -- the samples at the rim of the scene have depths near zero, 1 / d^2 is large there, and
grid_sample's coordinate round trip costs torch five digits of it.  AUTOGRAD_FACTOR = ceil(2 x 9.28e-4) = 1.
With a floor that loose this test says that the graph is wired -- the right leaves, the right channel, the upstream factor, no NaN --
and little about accuracy: a fused gradient several hundred times worse would still pass it.  The accuracy check is the derived
per-pixel bound above, which the point and map tests and test_the_functions_through_autograd_match_the_engine assert.
"""
import numpy as np
import pytest
import torch

import depth_loss_ref as ref
import gsbp_amd
from gsbp_amd import _lib, synthetic as syn
from gsbp_amd.rasterization import engine_on

pytestmark = pytest.mark.gpu
F = np.float32
H, W = 13, 19
B = _lib.DEPTH_BLOCK
COUNTS = (0, 1, B - 1, B, B + 1, 4 * B + 3)
LAYOUTS = ((4, 3), (1, 0))
AUTOGRAD_FACTOR = 1.0  # ceil(2 x the largest ratio measured, 9.28e-4): see the module's note
SCALE, UP = 1.3, 0.75


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def ulp_apart(got, want64):
    """|got - want| in units of the float32 spacing at want (want formed in float64)."""
    return abs(float(got) - want64) / float(np.spacing(F(abs(want64)))) if want64 != 0 else abs(float(got)) / 1e-45


@pytest.fixture(scope="module")
def cases(dev):
    """Per layout: the image on the host and the device, the longest point list, and the map; computed once, never written to."""
    out = {}
    pts, g = ref.make_points(max(COUNTS), H, W)
    gmap, wmap = ref.make_depth_map(H, W)
    for Dp, ch in LAYOUTS + ((3, 2),):
        render, alpha = ref.make_image(H, W, Dp, ch)
        out[(Dp, ch)] = dict(render=render, alpha=alpha, A=render[..., ch].copy(), d_render=torch.from_numpy(render).to(dev),
                             d_alpha=torch.from_numpy(alpha).to(dev))
    shared = dict(pts=pts, g=g, gmap=gmap, wmap=wmap, d_pts=torch.from_numpy(pts).to(dev), d_g=torch.from_numpy(g).to(dev),
                  d_gmap=torch.from_numpy(gmap).to(dev), d_wmap=torch.from_numpy(wmap).to(dev))
    return out, shared


@pytest.mark.parametrize("Dp, ch", LAYOUTS)
@pytest.mark.parametrize("M", COUNTS)
def test_point_term_forward_and_backward(dev, cases, Dp, ch, M):
    imgs, s = cases
    c = imgs[(Dp, ch)]
    eng = engine_on(dev)
    pts, g, d_pts, d_g = s["pts"][:M], s["g"][:M], s["d_pts"][:M].contiguous(), s["d_g"][:M].contiguous()
    loss, per_point = eng.depth_points_loss(c["d_render"], c["d_alpha"], d_pts, d_g, ch, SCALE, want_per_point=True)
    again, _ = eng.depth_points_loss(c["d_render"], c["d_alpha"], d_pts, d_g, ch, SCALE)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    cc = F(UP) * ref.scale_over_m(SCALE, M) if M else F(0)  # the kernel's c = upstream * (float)(scale / M), a float32 product
    want = ref.point_terms32(c["A"], c["alpha"], pts, g, cc)
    per_point = per_point.cpu().numpy()
    assert np.array_equal(bits(per_point[:, 0]), bits(want["d"])) and np.array_equal(bits(per_point[:, 1]), bits(want["t"]))
    want_loss = ref.point_loss64(want, SCALE, M)
    print(f"M = {M}: loss {float(loss):.9g}, float64 {want_loss:.17g}, {ulp_apart(loss, want_loss):.3f} ulp")
    assert ulp_apart(loss, want_loss) <= 1.0
    assert np.array_equal(bits(loss.cpu().numpy()), bits(again.cpu().numpy()))
    if M == 0:
        assert float(loss) == 0.0
    # the backward: the upstream gradient is a device scalar
    up = torch.tensor(UP, device=dev)
    v_render, v_alpha = eng.depth_points_backward(c["d_render"], c["d_alpha"], d_pts, d_g, up, ch, SCALE)
    assert tuple(v_render.shape) == (H, W, Dp) and tuple(v_alpha.shape) == (H, W)
    v_render, v_alpha = v_render.cpu().numpy(), v_alpha.cpu().numpy()
    assert np.isfinite(v_render).all() and np.isfinite(v_alpha).all()          # no NaN where d = 0
    assert not v_render[..., [k for k in range(Dp) if k != ch]].any()          # every other channel: exact zeros
    t64 = ref.point_terms64(c["A"], c["alpha"], pts, g, cc)
    vA, va, absA, absa, nA, na = ref.scatter_maps(t64, H, W)
    assert not v_render[..., ch][nA == 0].view(np.uint32).any() and not v_alpha[na == 0].view(np.uint32).any()
    errA, erra = np.abs(v_render[..., ch] - vA), np.abs(v_alpha - va)
    boundA, bounda = ref.grad_bound(nA, absA), ref.grad_bound(na, absa)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"M = {M}: largest error / bound: v_render {np.nanmax(np.where(boundA > 0, errA / boundA, 0)) if M else 0:.3f}, "
              f"v_alpha {np.nanmax(np.where(bounda > 0, erra / bounda, 0)) if M else 0:.3f}")
    assert (errA <= boundA).all() and (erra <= bounda).all()
    if M > 20:
        assert (nA > 1).any() and v_render[..., ch].any() and v_alpha.any()    # corners were shared
        empty = want["d"] == 0
        assert empty.any() and np.array_equal(bits(per_point[empty, 1]), bits(F(1) / g[empty]))


@pytest.mark.parametrize("Dp, ch", LAYOUTS + ((3, 2),))
@pytest.mark.parametrize("kind", ["disparity", "depth"])
@pytest.mark.parametrize("weighted", [False, True])
def test_map_term_forward_and_backward(dev, cases, Dp, ch, kind, weighted):
    imgs, s = cases
    c = imgs[(Dp, ch)]
    eng = engine_on(dev)
    w, d_w = (s["wmap"], s["d_wmap"]) if weighted else (None, None)
    loss, sums = eng.depth_map_loss(c["d_render"], c["d_alpha"], s["d_gmap"], d_w, kind, ch, SCALE)
    again, _ = eng.depth_map_loss(c["d_render"], c["d_alpha"], s["d_gmap"], d_w, kind, ch, SCALE)
    t32 = ref.map_terms32(c["A"], c["alpha"], s["gmap"], w, kind)
    swt, sw = ref.map_sums64(t32)
    got = sums.cpu().numpy()
    assert abs(got[0] - swt) <= 1e-12 * swt and abs(got[1] - sw) <= 1e-12 * sw
    want_loss = ref.map_loss64(t32, SCALE)
    print(f"{kind}, weights {weighted}: loss {float(loss):.9g}, float64 {want_loss:.17g}, {ulp_apart(loss, want_loss):.3f} ulp")
    assert ulp_apart(loss, want_loss) <= 1.0 and np.array_equal(bits(loss.cpu().numpy()), bits(again.cpu().numpy()))
    up = torch.tensor(UP, device=dev)
    v_render, v_alpha = eng.depth_map_backward(c["d_render"], c["d_alpha"], s["d_gmap"], sums, up, d_w, kind, ch, SCALE)
    r2, a2 = eng.depth_map_backward(c["d_render"], c["d_alpha"], s["d_gmap"], sums, up, d_w, kind, ch, SCALE)
    assert torch.equal(v_render.view(torch.int32), r2.view(torch.int32)) and torch.equal(v_alpha.view(torch.int32), a2.view(torch.int32))
    v_render, v_alpha = v_render.cpu().numpy(), v_alpha.cpu().numpy()
    want = ref.map_terms32(c["A"], c["alpha"], s["gmap"], w, kind, ref.map_c(UP, SCALE, float(got[1])))
    assert np.array_equal(bits(v_render[..., ch]), bits(want["v_A"])) and np.array_equal(bits(v_alpha), bits(want["v_a"]))
    assert not v_render[..., [k for k in range(Dp) if k != ch]].view(np.uint32).any()
    assert np.isfinite(v_render).all() and np.isfinite(v_alpha).all() and want["v_A"].any() and want["v_a"].any()
    t64 = ref.map_terms64(c["A"], c["alpha"], s["gmap"], w, kind, ref.map_c(UP, SCALE, float(got[1])))
    for k, v in (("v_A", v_render[..., ch]), ("v_a", v_alpha)):
        assert (np.abs(v - t64[k]) <= ref.grad_bound(1, np.abs(t64[k]))).all(), k


def test_a_map_without_a_valid_pixel_gives_zero_and_zeros(dev, cases):
    imgs, s = cases
    c = imgs[(4, 3)]
    eng = engine_on(dev)
    gmap = torch.from_numpy(ref.make_depth_map(H, W, all_invalid=True)[0]).to(dev)
    for kind in ("disparity", "depth"):
        loss, sums = eng.depth_map_loss(c["d_render"], c["d_alpha"], gmap, None, kind, 3, SCALE)
        v_render, v_alpha = eng.depth_map_backward(c["d_render"], c["d_alpha"], gmap, sums, torch.tensor(UP, device=dev), None, kind, 3,
                                                   SCALE)
        assert float(loss) == 0.0 and sums.tolist() == [0.0, 0.0]
        assert not v_render.view(torch.int32).any() and not v_alpha.view(torch.int32).any()
    # weights that are all zero: the same
    loss, sums = eng.depth_map_loss(c["d_render"], c["d_alpha"], s["d_gmap"], torch.zeros(H, W, device=dev), "depth", 3, SCALE)
    assert float(loss) == 0.0 and sums.tolist() == [0.0, 0.0]


def test_the_functions_through_autograd_match_the_engine(dev, cases):
    imgs, s = cases
    c = imgs[(4, 3)]
    M = B + 1
    render, alpha = c["d_render"].clone().requires_grad_(True), c["d_alpha"].clone()[..., None].requires_grad_(True)
    loss = gsbp_amd.depth_point_loss(render, alpha, s["d_pts"][:M].contiguous(), s["d_g"][:M].contiguous(), scale=SCALE)
    (UP * loss).backward()
    assert tuple(alpha.grad.shape) == (H, W, 1) and torch.isfinite(render.grad).all() and torch.isfinite(alpha.grad).all()
    t64 = ref.point_terms64(c["A"], c["alpha"], s["pts"][:M], s["g"][:M], F(UP) * ref.scale_over_m(SCALE, M))
    vA, va, absA, absa, nA, na = ref.scatter_maps(t64, H, W)
    assert (np.abs(render.grad[..., 3].cpu().numpy() - vA) <= ref.grad_bound(nA, absA)).all()
    assert (np.abs(alpha.grad[..., 0].cpu().numpy() - va) <= ref.grad_bound(na, absa)).all()
    assert not render.grad[..., :3].any()
    render.grad = alpha.grad = None
    loss = gsbp_amd.depth_map_loss(render, alpha, s["d_gmap"], s["d_wmap"], kind="depth", scale=SCALE)
    (UP * loss).backward()
    t32 = ref.map_terms32(c["A"], c["alpha"], s["gmap"], s["wmap"], "depth")
    want = ref.map_terms64(c["A"], c["alpha"], s["gmap"], s["wmap"], "depth", ref.map_c(UP, SCALE, ref.map_sums64(t32)[1]))
    assert (np.abs(render.grad[..., 3].cpu().numpy() - want["v_A"]) <= ref.grad_bound(1, np.abs(want["v_A"]))).all()
    assert (np.abs(alpha.grad[..., 0].cpu().numpy() - want["v_a"]) <= ref.grad_bound(1, np.abs(want["v_a"]))).all()
    # no gradient asked for: no backward launch, None
    plain = gsbp_amd.depth_point_loss(c["d_render"], c["d_alpha"], s["d_pts"][:5].contiguous(), s["d_g"][:5].contiguous())
    assert not plain.requires_grad
    with pytest.raises(gsbp_amd.GwbpError, match="channel"):
        gsbp_amd.depth_point_loss(c["d_render"], c["d_alpha"], s["d_pts"], s["d_g"], channel=4)
    with pytest.raises(gsbp_amd.GwbpError, match="points"):
        gsbp_amd.depth_point_loss(c["d_render"], c["d_alpha"], s["d_pts"][:, :1], s["d_g"])
    with pytest.raises(gsbp_amd.GwbpError, match="float32"):
        gsbp_amd.depth_map_loss(c["d_render"], c["d_alpha"], s["d_gmap"].double())


def figures(err):
    return dict(max_abs=float(err.abs().max()), frobenius=float(err.double().pow(2).sum().sqrt()))


def test_autograd_after_rasterization_against_the_literal_statement_by_the_floor_rule(dev):
    cfg = syn.CONFIGS["T0"]
    means, quats, scales, opac = (t.to(dev) for t in syn.activate(syn.make_scene(cfg)))
    K, vms = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg).to(dev)
    colors = torch.rand(means.shape[0], 3, generator=torch.Generator().manual_seed(5)).to(dev)
    means = means.clone().requires_grad_(True)
    out, alphas, _ = gsbp_amd.rasterization(means, quats, scales, opac, colors, vms[:1], K[None], cfg.width, cfg.height,
                                            render_mode="RGB+D")
    gen = np.random.default_rng(17)
    pts = (gen.uniform(0.0, 1.0, (300, 2)) * np.array([cfg.width - 1.0, cfg.height - 1.0])).astype(F)
    render_h, alpha_h = out[0].detach().cpu().numpy(), alphas[0, ..., 0].detach().cpu().numpy()
    d = ref.point_terms32(render_h[..., 3], alpha_h, pts, np.ones(len(pts), F))["d"]
    empty = float((d == 0).mean())
    print(f"{empty:.3f} of the points sample d = 0")
    assert empty <= 0.10                                  # (checked on the CPU from the restatement alone)
    pts = pts[d > 0]
    g = (d[d > 0] * gen.uniform(0.7, 1.4, len(pts))).astype(F)
    d_pts, d_g = torch.from_numpy(pts).to(dev), torch.from_numpy(g).to(dev)
    # end to end: the graph reaches the Gaussians
    gsbp_amd.depth_point_loss(out[0], alphas[0], d_pts, d_g).backward()
    assert torch.isfinite(means.grad).all() and means.grad.abs().sum() > 0
    # the leaves
    grads = {}
    for name, dtype in (("fused", torch.float32), ("floor", torch.float32), ("truth", torch.float64)):
        render = out[0].detach().to(dtype).requires_grad_(True)
        alpha = alphas[0, ..., 0].detach().to(dtype).requires_grad_(True)
        if name == "fused":
            loss = gsbp_amd.depth_point_loss(render, alpha, d_pts, d_g, scale=SCALE)
        else:
            loss, _ = ref.literal_point_loss(render, alpha, d_pts.to(dtype), d_g.to(dtype), channel=3, scale=SCALE)
        loss.backward()
        grads[name] = (loss.detach(), render.grad[..., 3].double(), alpha.grad.double())
        assert torch.isfinite(render.grad).all() and torch.isfinite(alpha.grad).all()
    worst = 0.0
    for i, leaf in ((1, "render"), (2, "alpha")):
        fused, floor = figures(grads["fused"][i] - grads["truth"][i]), figures(grads["floor"][i] - grads["truth"][i])
        for k in fused:
            ratio = fused[k] / floor[k]
            worst = max(worst, ratio)
            print(f"{leaf} {k}: fused {fused[k]:.3e}, floor {floor[k]:.3e}, ratio {ratio:.3f}")
    print(f"largest ratio {worst:.3f}")
    assert worst <= AUTOGRAD_FACTOR
