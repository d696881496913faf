"""The view's RGB render handed to the 2-D network by the lift's own front (create_feature_field / create_label_field /
create_mask_feature_field(render_colors=..., sh_degree=...), the gwbp_blend_*_rgb blends, Engine.blend_*_rgb).

The reference's per-view loop (backproject.py:89-113, :223-249) renders each view with SH degree 3 and runs its network on that
render.  Here the "network" is a deterministic function of the image (image @ W for pixel maps, a 16 x 16 average pool then
@ W for token maps, argmax over channels for labels), and every image handed over must equal rasterization()'s render bit for
bit; the field must equal that of a feature_fn that calls rasterization() itself."""
import numpy as np
import pytest
import torch

from util import rel_row_err, scene_np, sort_pairs, to_dev

import gsbp_amd
from gsbp_amd import rasterization
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
N_VIEWS = 6  # more views than any pipeline has workspaces: fronts reuse workspaces while earlier images are still held
TOL = 1e-4


@pytest.fixture(scope="module")
def t1(dev):
    cfg, sc = scene_np("T1", n_views=N_VIEWS)
    g = to_dev(sc, dev)
    sh = syn.make_sh_coeffs(cfg, 3, device=dev)
    return cfg, g, sh


def _gauss(g):
    return g["means"], g["quats"], g["scales"], g["opac"]


def _reference_render(cfg, g, colors, v, sh_degree=3, camera_model="pinhole", rasterize_mode="classic"):
    out, _, _ = rasterization(*_gauss(g), colors, g["vms"][v][None], g["K"][None], cfg.width, cfg.height,
                              sh_degree=sh_degree, camera_model=camera_model, rasterize_mode=rasterize_mode)
    return out[0]


def _weights(D, dev, seed=5):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(3, D, generator=gen).to(dev)


def _pixel_net(W):
    return lambda image: image @ W


def _token_net(W, hw):
    def net(image):
        pooled = torch.nn.functional.adaptive_avg_pool2d(image.permute(2, 0, 1)[None], hw)[0].permute(1, 2, 0)
        return (pooled @ W).contiguous()
    return net


def _field(cfg, g, net, dim, colors=None, sh_degree=3, seen=None, keep=None, camera=None, ref_colors=None, **kw):
    """create_feature_field with render_colors (colors given), or with a feature_fn that renders `ref_colors` through
    rasterization() itself (today's way)."""
    camera = camera or {}
    if colors is not None:
        def fn(v, image):
            assert image.shape == (cfg.height, cfg.width, 3) and image.dtype == torch.float32 and image.is_contiguous()
            if seen is not None:
                seen.append((v, image.clone()))
            if keep is not None:
                keep.append((v, image))
            return net(image)
        extra = dict(render_colors=colors, sh_degree=sh_degree)
    else:
        def fn(v):
            return net(_reference_render(cfg, g, ref_colors, v, sh_degree, **camera))
        extra = {}
    return gsbp_amd.create_feature_field(*_gauss(g), g["vms"], g["K"], cfg.width, cfg.height, fn, dim, return_partials=True,
                                         **camera, **extra, **kw)



def _check_images(cfg, g, sh, seen, n_views=N_VIEWS, **camera):
    got = {}
    for v, img in seen:
        got[v] = img  # (the last call per view: an overflow retry asks again)
    assert sorted(got) == list(range(n_views))
    for v, img in got.items():
        ref = _reference_render(cfg, g, sh, v, **camera)
        assert torch.equal(img, ref), f"view {v}: max |diff| {float((img - ref).abs().max())}"


def _check_field(a, b):
    _, Fa, da, sa = a
    _, Fb, db, sb = b
    assert sa["overflow"] == 0 and sb["overflow"] == 0
    assert rel_row_err(Fa.cpu().numpy(), Fb.cpu().numpy()) <= TOL
    assert rel_row_err(da.cpu().numpy()[:, None], db.cpu().numpy()[:, None]) <= TOL


# ---- the blends themselves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["store", "halves", "halves_d", "tokens"])
@pytest.mark.parametrize("weighted", [False, True])
def test_rgb_blend_renders_like_render_pixels_and_blends_like_the_plain_blend(t1, dev, form, weighted):
    """gwbp_blend_*_rgb: image == gwbp_render_pixels bit for bit, and the weight store, d, token sums and alphas equal those of
    the blend without the composite."""
    cfg, g, sh = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    eng.set_narrow_scatter(form == "store")
    pw = syn.make_pixel_weights(cfg, 1, device=dev, kind="confidence") if weighted else None
    view = eng.view(g["vms"][1], g["K"], cfg.width, cfg.height)
    cols = eng.view_colors(view, g["means"], sh, 3)

    def front():
        eng.project(view, *_gauss(g))
        eng.bin_sort(view)

    front()
    ref_img, ref_alpha = eng.render_pixels(view, cols)
    d0 = torch.zeros(cfg.n_gaussians, device=dev)
    d1 = torch.zeros(cfg.n_gaussians, device=dev)
    lr = (8, 12)
    if form == "tokens":  # (the token-quadrant sums: test_token_rgb_blend_lifts_the_same_field)
        a0 = (eng.blend_tokens_weighted(view, *lr, pw, want_alphas=True) if weighted
              else eng.blend_tokens(view, *lr, want_alphas=True))
        front()
        img, a1 = eng.blend_tokens_rgb(view, *lr, cols, pixel_weights=pw, want_alphas=True)
    else:
        dd = d0 if form == "halves_d" else None
        a0 = (eng.blend_weighted(view, pw, want_alphas=True, d=dd) if weighted
              else eng.blend_weights(view, want_alphas=True, d=dd))
        k0, w0 = sort_pairs(*(t.cpu().numpy() for t in eng.dump_pairs(view)))
        st0 = eng.stats()
        front()
        img, a1 = eng.blend_weights_rgb(view, cols, pixel_weights=pw, d=d1 if form == "halves_d" else None, want_alphas=True)
        k1, w1 = sort_pairs(*(t.cpu().numpy() for t in eng.dump_pairs(view)))
        st1 = eng.stats()
        assert np.array_equal(k0, k1) and np.array_equal(w0.view(np.uint32), w1.view(np.uint32))
        assert st0 == st1
        # (d is added with one float atomic per record: equal up to the order of those additions)
        assert float((d0 - d1).abs().max()) <= 1e-5 * float(d0.abs().max())
    assert torch.equal(img, ref_img) and torch.equal(a1, a0) and torch.equal(a1, ref_alpha)
    assert torch.equal(img, _reference_render(cfg, g, sh, 1))
    assert float(img.abs().sum()) > 0


def test_token_rgb_blend_lifts_the_same_field(t1, dev):
    cfg, g, sh = t1
    D, lr = 256, (8, 12)
    tok = torch.randn(*lr, D, generator=torch.Generator(device="cpu").manual_seed(3)).to(dev)
    out = []
    for rgb in (False, True):
        eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
        view = eng.view(g["vms"][0], g["K"], cfg.width, cfg.height)
        eng.project(view, *_gauss(g))
        eng.bin_sort(view)
        F = torch.zeros(cfg.n_gaussians, D, device=dev)
        d = torch.zeros(cfg.n_gaussians, device=dev)
        if rgb:
            eng.blend_tokens_rgb(view, *lr, eng.view_colors(view, g["means"], sh, 3))
        else:
            eng.blend_tokens(view, *lr)
        eng.scatter_tokens(view, tok, F, d)
        out.append((F, d))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---- every schedule of the drivers: image parity and field parity ------------------------------------------------------
SCHEDULES = {
    "slab_d512": dict(dim=512),
    "tokens": dict(dim=256, upsample="nearest", lowres=(8, 12)),
    "bilinear": dict(dim=128, upsample="bilinear", lowres=(34, 50)),
    "fused_d16": dict(dim=16),                           # small scene: view-per-stream schedule
    "fused_d16_two": dict(dim=16, pipeline=2),           # the fused kernel beside a side stream
    "encoder_in_blend": dict(dim=64, encoder=16),
    "tokens_stream_safe": dict(dim=256, upsample="nearest", lowres=(8, 12), feature_fn_stream_safe=True),
    "fused_d16_stream_safe": dict(dim=16, feature_fn_stream_safe=True),
    "serial": dict(dim=64, pipeline=False),
    "serial_tokens": dict(dim=256, upsample="nearest", lowres=(8, 12), pipeline=False),
    "weighted_d512": dict(dim=512, weighted=True),
    "weighted_fused": dict(dim=16, weighted=True),
}


def _schedule_net(cfg, spec, dev):
    lowres = spec.get("lowres")
    W = _weights(spec["dim"], dev)
    return _token_net(W, lowres) if lowres else _pixel_net(W)


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_images_and_field_match_rasterization_fed_network(t1, dev, name):
    cfg, g, sh = t1
    spec = dict(SCHEDULES[name])
    net = _schedule_net(cfg, spec, dev)
    dim = spec.pop("dim")
    spec.pop("lowres", None)
    if spec.pop("weighted", False):
        spec["pixel_weight_fn"] = lambda v: syn.make_pixel_weights(cfg, v, device=dev, kind="confidence")
    enc = spec.pop("encoder", None)
    if enc is not None:
        spec["encoder"] = torch.randn(dim, enc, generator=torch.Generator(device="cpu").manual_seed(9)).to(dev) / 8.0
    seen = []
    a = _field(cfg, g, net, dim, colors=sh, seen=seen, **spec)
    b = _field(cfg, g, net, dim, ref_colors=sh, **spec)
    _check_images(cfg, g, sh, seen)
    _check_field(a, b)


@pytest.mark.parametrize("camera_model", ["pinhole", "fisheye", "ortho"])
@pytest.mark.parametrize("rasterize_mode", ["classic", "antialiased"])
def test_camera_models(t1, dev, camera_model, rasterize_mode):
    cfg, g, sh = t1
    if camera_model == "ortho":  # an orthographic camera wants a focal length in pixels per world unit
        g = dict(g, K=g["K"].clone())
        g["K"][0, 0] = g["K"][1, 1] = 60.0
    cam = dict(camera_model=camera_model, rasterize_mode=rasterize_mode)
    net = _pixel_net(_weights(64, dev))
    seen = []
    a = _field(cfg, g, net, 64, colors=sh, seen=seen, camera=cam)
    b = _field(cfg, g, net, 64, camera=cam, ref_colors=sh)
    _check_images(cfg, g, sh, seen, **cam)
    _check_field(a, b)


def test_plain_colours_without_sh(t1, dev):
    cfg, g, _ = t1
    cols = torch.rand(cfg.n_gaussians, 3, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev)
    seen = []
    net = _pixel_net(_weights(512, dev))
    a = _field(cfg, g, net, 512, colors=cols, sh_degree=None, seen=seen)
    for v, img in seen:
        assert torch.equal(img, _reference_render(cfg, g, cols, v, sh_degree=None))
    _check_field(a, _field(cfg, g, net, 512, sh_degree=None, ref_colors=cols))


@pytest.mark.parametrize("schedule", ["composite", "render_pixels"])
def test_held_images_are_never_overwritten(t1, dev, monkeypatch, schedule):
    """A feature_fn that keeps every image until the job ends finds each one still equal to its reference render."""
    cfg, g, sh = t1
    if schedule == "render_pixels":
        monkeypatch.setattr(gsbp_amd.ViewPipeline, "RENDER_IN_BLEND", {"store": False, "halves": False, "tokens": False})
    keep = []
    _field(cfg, g, _pixel_net(_weights(512, dev)), 512, colors=sh, keep=keep)
    torch.cuda.synchronize()
    _check_images(cfg, g, sh, keep)


def test_render_pixels_fallback_gives_the_same_images_and_field(t1, dev, monkeypatch):
    cfg, g, sh = t1
    net = _pixel_net(_weights(512, dev))
    seen_a, seen_b = [], []
    a = _field(cfg, g, net, 512, colors=sh, seen=seen_a)
    monkeypatch.setattr(gsbp_amd.ViewPipeline, "RENDER_IN_BLEND", {"store": False, "halves": False, "tokens": False})
    b = _field(cfg, g, net, 512, colors=sh, seen=seen_b)
    assert all(va == vb and torch.equal(ia, ib) for (va, ia), (vb, ib) in zip(seen_a, seen_b))
    _check_field(a, b)


def test_overflow_retry(t1, dev):
    """An engine too small for the views overflows, the job restarts with grown capacities, and feature_fn is asked again:
    same field, and the images of the retry are right."""
    cfg, g, sh = t1
    net = _pixel_net(_weights(512, dev))
    small = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, tight_binning=True, isect_cap=4096)
    seen = []
    a = _field(cfg, g, net, 512, colors=sh, seen=seen, engine=small)
    assert small.isect_cap > 4096 and len(seen) > N_VIEWS  # it did overflow and retry
    _check_images(cfg, g, sh, seen)
    _check_field(a, _field(cfg, g, net, 512, ref_colors=sh))


# ---- labels and masks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [True, False])
def test_label_field(t1, dev, pipeline):
    cfg, g, sh = t1
    W = _weights(5, dev, seed=11)

    def labels_of(image):
        return (image @ W).argmax(dim=2).to(torch.int32)

    seen = []

    def fn(v, image):
        seen.append((v, image.clone()))
        return labels_of(image)

    a = gsbp_amd.create_label_field(*_gauss(g), g["vms"], g["K"], cfg.width, cfg.height, fn, 5, pipeline=pipeline,
                                    return_partials=True, render_colors=sh, sh_degree=3)
    b = gsbp_amd.create_label_field(*_gauss(g), g["vms"], g["K"], cfg.width, cfg.height,
                                    lambda v: labels_of(_reference_render(cfg, g, sh, v)), 5, pipeline=pipeline,
                                    return_partials=True)
    _check_images(cfg, g, sh, seen)
    _check_field(a, b)


@pytest.mark.parametrize("pipeline", [True, False])
def test_mask_feature_field(t1, dev, pipeline):
    cfg, g, sh = t1
    W = _weights(6, dev, seed=12)
    table = torch.randn(6, 64, generator=torch.Generator(device="cpu").manual_seed(4)).to(dev)

    def mask_of(image):
        return (image @ W).argmax(dim=2).to(torch.int32), table

    seen = []

    def fn(v, image):
        seen.append((v, image.clone()))
        return mask_of(image)

    a = gsbp_amd.create_mask_feature_field(*_gauss(g), g["vms"], g["K"], cfg.width, cfg.height, fn, 64, pipeline=pipeline,
                                           return_partials=True, render_colors=sh, sh_degree=3)
    b = gsbp_amd.create_mask_feature_field(*_gauss(g), g["vms"], g["K"], cfg.width, cfg.height,
                                           lambda v: mask_of(_reference_render(cfg, g, sh, v)), 64, pipeline=pipeline,
                                           return_partials=True)
    _check_images(cfg, g, sh, seen)
    _check_field(a, b)


# ---- full size ------------------------------------------------------------------------------------------------------------
def test_c2_full_size_two_views(dev, orc, monkeypatch):
    """C2 geometry (1M Gaussians, 1600 x 1060), two views, D = 512 through the pipelined driver, whose front runs the 256-channel
    storing blend with the composite (k_blend<kHalves, 1, false, true>): each image equals rasterization()'s, and the field equals
    the CPU oracle's on the maps made from them."""
    cfg = syn.CONFIGS["C2"]
    V = 2
    g_cpu = syn.activate(syn.make_scene(cfg))
    means, quats, scales, opac = [t.to(dev) for t in g_cpu]
    vms, K = syn.make_cameras(cfg, n_views=V), syn.intrinsics(cfg)
    sh = syn.make_sh_coeffs(cfg, 3, device=dev)
    W = _weights(512, dev)
    composites = []
    orig = gsbp_amd.Engine.blend_weights_rgb

    def spy(self, *a, **k):
        composites.append(self._wide_requested())
        return orig(self, *a, **k)

    monkeypatch.setattr(gsbp_amd.Engine, "blend_weights_rgb", spy)
    maps = {}

    def fn(v, image):
        maps[v] = (image.clone(), image @ W)
        return maps[v][1]

    out, F, d, st = gsbp_amd.create_feature_field(means, quats, scales, opac, vms.to(dev), K.to(dev), cfg.width, cfg.height, fn,
                                                  512, return_partials=True, render_colors=sh, sh_degree=3)
    assert st["overflow"] == 0 and composites == [True] * V and sorted(maps) == list(range(V))
    for v in range(V):
        ref, _, _ = rasterization(means, quats, scales, opac, sh, vms[v:v + 1].to(dev), K[None].to(dev), cfg.width, cfg.height,
                                  sh_degree=3)
        assert torch.equal(maps[v][0], ref[0]), v
    Fr = np.zeros((cfg.n_gaussians, 512), np.float64)
    dr = np.zeros(cfg.n_gaussians, np.float64)
    pairs = 0
    for v in range(V):
        info = orc.backproject_view(*[t.numpy() for t in g_cpu], vms[v].numpy(), K.numpy(), cfg.width, cfg.height,
                                    maps[v][1].cpu().numpy(), Fr, dr)
        pairs += info["n_pairs"]
    assert st["n_pairs"] == pairs
    assert rel_row_err(F.cpu().numpy(), Fr) <= TOL
    assert rel_row_err(d.cpu().numpy()[:, None], dr[:, None]) <= TOL
