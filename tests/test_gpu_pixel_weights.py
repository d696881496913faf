"""Per-pixel weight maps on the GPU (the gwbp_*_ex blends, Engine.*_weighted, create_feature_field / create_label_field
(pixel_weight_fn=...)).  The definition is the reference's per-view loop with both targets multiplied by c:
    F[g] += sum_p w_g(p) c(p) f(p),   d[g] += sum_p w_g(p) c(p)
so F must equal the oracle's F of the map c f, and d the oracle's F of the one-channel map c.  The store itself is checked
entry for entry: a mask filters the unweighted store, a float map scales its weights by exactly one rounding."""
import numpy as np
import pytest
import torch

from util import rel_row_err, scene_np, sort_pairs, to_dev

import gsbp_amd
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
TOL = 1e-4
N_VIEWS = 5  # more views than the small-scene pipeline has workspaces: fronts beyond the first ones wait on the map's event


@pytest.fixture(scope="module")
def t1(dev):
    cfg, sc = scene_np("T1", n_views=N_VIEWS)
    return cfg, sc, to_dev(sc, dev)


def _front(eng, cfg, g, v, wide=False, **cam):
    eng.set_narrow_scatter(not wide)
    view = eng.view(g["vms"][v], g["K"], cfg.width, cfg.height, **cam)
    eng.project(view, g["means"], g["quats"], g["scales"], g["opac"])
    eng.bin_sort(view)
    return view


def _dump(eng, view):
    gid, pix, w = (t.cpu().numpy() for t in eng.dump_pairs(view))
    return gid, pix, w


def _conf(cfg, v, dev):
    return syn.make_pixel_weights(cfg, v, device=dev, kind="confidence")


def _mask(cfg, v, dev):
    return syn.make_pixel_weights(cfg, v, device=dev)


# ---- the weight store, exactly ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_mask_filters_the_unweighted_store(t1, dev, wide):
    cfg, _, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _front(eng, cfg, g, 0, wide)
    a0 = eng.blend_weights(view, want_alphas=True)
    k0, w0 = sort_pairs(*_dump(eng, view))
    m = _mask(cfg, 0, dev)
    for c in (m, m.to(torch.uint8) * 255):  # bool, and a 0 / 255 PNG mask
        view = _front(eng, cfg, g, 0, wide)
        a1 = eng.blend_weighted(view, c, want_alphas=True)
        k1, w1 = sort_pairs(*_dump(eng, view))
        keep = m.reshape(-1).cpu().numpy()[(k0 & 0xFFFFFFFF).astype(np.int64)]
        assert 0 < len(k1) < len(k0)
        assert np.array_equal(k1, k0[keep]) and np.array_equal(w1.view(np.uint32), w0[keep].view(np.uint32))
        assert torch.equal(a0, a1)  # the alpha map is the unweighted one
        assert eng.stats()["n_pairs"] == len(k1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_float_map_scales_each_stored_weight_by_one_rounding(t1, dev, dtype):
    cfg, _, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _front(eng, cfg, g, 1)
    eng.blend_weights(view)
    k0, w0 = sort_pairs(*_dump(eng, view))
    c = _conf(cfg, 1, dev).to(dtype)
    view = _front(eng, cfg, g, 1)
    eng.blend_weighted(view, c)
    k1, w1 = sort_pairs(*_dump(eng, view))
    cf = c.float().reshape(-1).cpu().numpy()[(k0 & 0xFFFFFFFF).astype(np.int64)]
    keep = cf != 0
    want = (w0[keep].astype(np.float32) * cf[keep].astype(np.float32)).astype(np.float32)  # fl(w c)
    assert np.array_equal(k1, k0[keep]) and np.array_equal(w1.view(np.uint32), want.view(np.uint32))


def test_all_ones_and_all_zeros(t1, dev):
    cfg, _, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _front(eng, cfg, g, 0)
    eng.blend_weights(view)
    k0, w0 = sort_pairs(*_dump(eng, view))
    n_headers0 = eng.stats()["n_headers"]
    for ones in (torch.ones(cfg.height, cfg.width, device=dev), torch.ones(cfg.height, cfg.width, dtype=torch.uint8, device=dev)):
        view = _front(eng, cfg, g, 0)
        eng.blend_weighted(view, ones)
        k1, w1 = sort_pairs(*_dump(eng, view))
        assert np.array_equal(k1, k0) and np.array_equal(w1.view(np.uint32), w0.view(np.uint32))
        assert eng.stats()["n_headers"] == n_headers0
    # all zero: no entry, no header, F = d = 0 through the store, the fused kernels and token space
    zero = torch.zeros(cfg.height, cfg.width, device=dev)
    for wide in (False, True):
        view = _front(eng, cfg, g, 0, wide)
        a = eng.blend_weighted(view, zero, want_alphas=True)
        st = eng.stats()
        assert st["n_headers"] == 0 and st["n_pairs"] == 0 and float(a.max()) > 0
        F, d = torch.zeros(cfg.n_gaussians, 256, device=dev), torch.zeros(cfg.n_gaussians, device=dev)
        eng.scatter(view, syn.make_feature_map(cfg, 0, device=dev, dim=256), F, d)
        assert float(F.abs().max()) == 0 and float(d.abs().max()) == 0
    for D in (8, 24):
        view = _front(eng, cfg, g, 0)
        F, d = torch.zeros(cfg.n_gaussians, D, device=dev), torch.zeros(cfg.n_gaussians, device=dev)
        eng.blend_scatter_weighted(view, syn.make_feature_map(cfg, 0, device=dev, dim=D), zero, F, d)
        assert float(F.abs().max()) == 0 and float(d.abs().max()) == 0 and eng.stats()["n_headers"] == 0
    view = _front(eng, cfg, g, 0)
    eng.blend_tokens_weighted(view, 8, 12, zero)
    F, d = torch.zeros(cfg.n_gaussians, 64, device=dev), torch.zeros(cfg.n_gaussians, device=dev)
    eng.scatter_tokens(view, torch.randn(8, 12, 64, device=dev), F, d)
    assert float(F.abs().max()) == 0 and float(d.abs().max()) == 0 and eng.stats()["n_headers"] == 0


def test_token_space_all_ones_is_bit_identical_and_alphas_unchanged(t1, dev):
    """Token space is deterministic (no atomics), so an all-ones map must give F and d bit for bit."""
    cfg, _, g = t1
    tok = torch.randn(8, 12, 64, device=dev)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    res = []
    for c in (None, torch.ones(cfg.height, cfg.width, device=dev), torch.ones(cfg.height, cfg.width, dtype=torch.bool, device=dev)):
        view = _front(eng, cfg, g, 0)
        a = eng.blend_tokens(view, 8, 12, want_alphas=True) if c is None else eng.blend_tokens_weighted(view, 8, 12, c, want_alphas=True)
        F, d = torch.zeros(cfg.n_gaussians, 64, device=dev), torch.zeros(cfg.n_gaussians, device=dev)
        eng.scatter_tokens(view, tok, F, d)
        res.append((F, d, a))
    for F, d, a in res[1:]:
        assert torch.equal(F, res[0][0]) and torch.equal(d, res[0][1]) and torch.equal(a, res[0][2])
    # a mask: the alpha map still the unweighted one
    view = _front(eng, cfg, g, 0)
    assert torch.equal(eng.blend_tokens_weighted(view, 8, 12, _mask(cfg, 0, dev), want_alphas=True), res[0][2])


def test_fused_kernels_alphas_unchanged(t1, dev):
    cfg, _, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    c = _conf(cfg, 0, dev)
    for D in (8, 24):
        feats = syn.make_feature_map(cfg, 0, device=dev, dim=D)
        F = torch.zeros(cfg.n_gaussians, D, device=dev)
        a0 = eng.blend_scatter(_front(eng, cfg, g, 0), feats, F, None, want_alphas=True)
        a1 = eng.blend_scatter_weighted(_front(eng, cfg, g, 0), feats, c, F, None, want_alphas=True)
        assert torch.equal(a0, a1)


def test_validator_on_the_device(t1, dev):
    cfg, _, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _front(eng, cfg, g, 0)
    with pytest.raises(gsbp_amd.GwbpError, match=r"\[H,W\]"):
        eng.blend_weighted(view, torch.ones(cfg.height, cfg.width + 1, device=dev))
    with pytest.raises(gsbp_amd.GwbpError, match=r"\[H,W\]"):
        eng.blend_weighted(view, torch.ones(cfg.height, cfg.width, 1, device=dev))
    with pytest.raises(gsbp_amd.GwbpError, match="float32"):
        eng.blend_weighted(view, torch.ones(cfg.height, cfg.width, dtype=torch.int32, device=dev))
    with pytest.raises(gsbp_amd.GwbpError, match="device"):
        eng.blend_weighted(view, torch.ones(cfg.height, cfg.width))


# ---- the drivers against the oracle -------------------------------------------------------------------------------------------
def _oracle_Fd(orc, cfg, sc, maps, weights, ids):
    """(F of the maps c f, F of the one-channel maps c) through the C oracle: what F and d of the weighted job must be."""
    h = [sc[k].numpy() for k in ("means", "quats", "scales", "opac")]
    vms = [sc["vms"][v].numpy() for v in ids]
    # (uint8 / bool maps are read as 0 / 1: a 0 / 255 mask weighs its pixels by 1)
    cw = [(lambda c: (c != 0).float() if c.dtype in (torch.uint8, torch.bool) else c.float())(weights(v)).cpu() for v in ids]
    fw = [(maps(v).float().cpu() * c[..., None]).numpy() for v, c in zip(ids, cw)]
    D = fw[0].shape[2]
    _, F, _, _ = orc.backproject_oracle(*h, vms, sc["K"].numpy(), cfg.width, cfg.height, lambda i: fw[i], D)
    _, dF, _, _ = orc.backproject_oracle(*h, vms, sc["K"].numpy(), cfg.width, cfg.height,
                                         lambda i: np.ascontiguousarray(cw[i].numpy()[..., None]), 1)
    return F, dF[:, 0]


def _check(F, d, Fr, dr):
    assert np.abs(dr).max() > 0
    assert rel_row_err(F.cpu().numpy(), Fr) <= TOL
    assert rel_row_err(d.cpu().numpy()[:, None], dr[:, None]) <= TOL


def _upsampled(cfg, low, mode):
    kw = {"align_corners": False} if mode == "bilinear" else {}
    return torch.nn.functional.interpolate(low.float().permute(2, 0, 1)[None], size=(cfg.height, cfg.width), mode=mode,
                                           **kw)[0].permute(1, 2, 0)


WEIGHT_KINDS = ["bool", "u8", "f16", "bf16", "f32", "f32_channel_slice"]


def _weights(cfg, dev, kind):
    def fn(v):
        c = _conf(cfg, v, dev)
        if kind == "bool":
            return c > 0
        if kind == "u8":
            return (c > 0).to(torch.uint8) * 255
        if kind == "f16":
            return c.half()
        if kind == "bf16":
            return c.bfloat16()
        if kind == "f32":
            return c
        return torch.stack([torch.zeros_like(c), c, torch.ones_like(c)], dim=-1)[:, :, 1]  # strides (3 W, 3)
    return fn


@pytest.mark.parametrize("kind", WEIGHT_KINDS)
def test_weight_types_against_the_oracle(t1, dev, orc, kind):
    cfg, sc, g = t1
    ids = list(range(N_VIEWS))
    feats = lambda v: syn.make_feature_map(cfg, v, device=dev, dim=256)  # noqa: E731
    wf = _weights(cfg, dev, kind)
    Fr, dr = _oracle_Fd(orc, cfg, sc, feats, wf, ids)
    _, F, d, st = gsbp_amd.create_feature_field(g["means"], g["quats"], g["scales"], g["opac"], g["vms"], g["K"], cfg.width,
                                                cfg.height, feats, 256, return_partials=True, pixel_weight_fn=wf)
    assert st["overflow"] == 0
    _check(F, d, Fr, dr)


# (schedule name, create_feature_field keywords, D, map kind)
SCHEDULES = [
    ("fused_quarter_view_per_stream", dict(), 24, None),
    ("fused_small_serial", dict(pipeline=False), 8, None),
    ("narrow_128", dict(), 128, None),
    ("narrow_128_no_fuse_serial", dict(pipeline=False, fuse_small=False), 16, None),
    ("wide_256", dict(), 256, None),
    ("wide_512", dict(), 512, None),
    ("serial_256", dict(pipeline=False), 256, None),
    ("pipeline_2", dict(pipeline=2), 128, None),
    ("half_fp16_256", dict(), 256, "fp16"),
    ("half_bf16_128_serial", dict(pipeline=False), 128, "bf16"),
    ("nearest_token", dict(upsample="nearest"), 64, "low"),
    ("nearest_token_serial", dict(upsample="nearest", pipeline=False), 64, "low"),
    ("nearest_pixel_slabs", dict(upsample="nearest", token_space=False), 64, "low"),
    ("bilinear", dict(upsample="bilinear"), 128, "low"),
    ("encoder_in_blend", dict(), 32, "encoder"),
    ("encoder_in_blend_split", dict(encoder_split=True), 32, "encoder"),
    ("encoder_in_staging", dict(fuse_encoder=True), 32, "encoder"),
    ("encoder_ahead", dict(encoder_in_blend=False), 32, "encoder"),
    ("encoder_serial", dict(pipeline=False), 32, "encoder"),
]


@pytest.mark.parametrize("name, kw, D, kind", SCHEDULES, ids=[s[0] for s in SCHEDULES])
def test_schedules_against_the_oracle(t1, dev, orc, name, kw, D, kind):
    cfg, sc, g = t1
    ids = list(range(N_VIEWS))
    wf = _weights(cfg, dev, "f32")
    enc = None
    if kind == "low":
        lows = {v: torch.randn(8, 12, D, generator=torch.Generator().manual_seed(v)).to(dev) for v in ids}
        maps, ref_maps = lows.__getitem__, (lambda v: _upsampled(cfg, lows[v], kw["upsample"]))
    elif kind == "encoder":
        enc = torch.randn(D, 8, generator=torch.Generator().manual_seed(7)).to(dev) / D ** 0.5
        maps = lambda v: syn.make_feature_map(cfg, v, device=dev, dim=D)  # noqa: E731
        ref_maps = lambda v: maps(v) @ enc  # noqa: E731
    else:
        dt = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(kind, torch.float32)
        maps = lambda v: syn.make_feature_map(cfg, v, device=dev, dim=D).to(dt)  # noqa: E731
        ref_maps = maps
    Fr, dr = _oracle_Fd(orc, cfg, sc, ref_maps, wf, ids)
    _, F, d, st = gsbp_amd.create_feature_field(g["means"], g["quats"], g["scales"], g["opac"], g["vms"], g["K"], cfg.width,
                                                cfg.height, maps, D, encoder=enc, return_partials=True, pixel_weight_fn=wf,
                                                **kw)
    assert st["overflow"] == 0
    _check(F, d, Fr, dr)


@pytest.mark.parametrize("camera_model", ["ortho", "fisheye"])
@pytest.mark.parametrize("rasterize_mode", ["classic", "antialiased"])
@pytest.mark.parametrize("D", [24, 256])
def test_camera_models_equal_the_unweighted_library_on_c_times_f(t1, dev, camera_model, rasterize_mode, D):
    """Under a camera model / rasterize mode the weighted job must equal the unweighted job on c f (F) and on c (d)."""
    cfg, sc, g = t1
    wf = _weights(cfg, dev, "f32")
    maps = lambda v: syn.make_feature_map(cfg, v, device=dev, dim=D)  # noqa: E731
    args = (g["means"], g["quats"], g["scales"], g["opac"], g["vms"], g["K"], cfg.width, cfg.height)
    cam = dict(camera_model=camera_model, rasterize_mode=rasterize_mode, return_partials=True)
    _, F, d, _ = gsbp_amd.create_feature_field(*args, maps, D, pixel_weight_fn=wf, **cam)
    _, Fr, _, _ = gsbp_amd.create_feature_field(*args, lambda v: maps(v) * wf(v)[..., None], D, **cam)
    _, dr, _, _ = gsbp_amd.create_feature_field(*args, lambda v: wf(v)[..., None].contiguous(), 1, **cam)
    _check(F, d, Fr.cpu().numpy(), dr[:, 0].cpu().numpy())


@pytest.mark.parametrize("pipeline", [True, False])
def test_label_field_against_the_oracle(t1, dev, orc, pipeline):
    cfg, sc, g = t1
    K = 5
    ids = list(range(N_VIEWS))
    wf = _weights(cfg, dev, "f32")
    labels = lambda v: syn.make_label_map(cfg, v, K, device=dev)  # noqa: E731
    one_hot = lambda v: torch.nn.functional.one_hot(labels(v).long(), K).float()  # noqa: E731
    Fr, dr = _oracle_Fd(orc, cfg, sc, one_hot, wf, ids)
    P, F, d, st = gsbp_amd.create_label_field(g["means"], g["quats"], g["scales"], g["opac"], g["vms"], g["K"], cfg.width,
                                              cfg.height, labels, K, pipeline=pipeline, return_partials=True,
                                              pixel_weight_fn=wf)
    assert st["overflow"] == 0
    _check(F, d, Fr, dr)
    rows = d > 0  # fractions sum to 1 over the weighted pixels
    assert float((P[rows].sum(1) - 1).abs().max()) < 1e-5


def test_grow_and_retry_with_small_capacities(t1, dev, orc):
    cfg, sc, g = t1
    ids = list(range(N_VIEWS))
    wf = _weights(cfg, dev, "bool")
    maps = lambda v: syn.make_feature_map(cfg, v, device=dev, dim=128)  # noqa: E731
    Fr, dr = _oracle_Fd(orc, cfg, sc, maps, wf, ids)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, isect_cap=3000, pair_cap=1 << 15,
                          tight_binning=True)
    _, F, d, st = gsbp_amd.create_feature_field(g["means"], g["quats"], g["scales"], g["opac"], g["vms"], g["K"], cfg.width,
                                                cfg.height, maps, 128, engine=eng, return_partials=True, pixel_weight_fn=wf)
    assert st["overflow"] == 0 and eng.isect_cap > 3000
    _check(F, d, Fr, dr)


def test_mean_reduction_keeps_its_scales(t1, dev, orc):
    cfg, sc, g = t1
    wf = _weights(cfg, dev, "f32")
    maps = lambda v: syn.make_feature_map(cfg, v, device=dev, dim=256)  # noqa: E731
    args = (g["means"], g["quats"], g["scales"], g["opac"], g["vms"], g["K"], cfg.width, cfg.height, maps, 256)
    _, Fs, ds, _ = gsbp_amd.create_feature_field(*args, return_partials=True, pixel_weight_fn=wf)
    _, Fm, dm, _ = gsbp_amd.create_feature_field(*args, reduction="mean", return_partials=True, pixel_weight_fn=wf)
    HW = cfg.height * cfg.width
    assert rel_row_err(Fm.cpu().numpy() * (HW * 256), Fs.cpu().numpy()) <= TOL
    assert rel_row_err(dm.cpu().numpy()[:, None] * (HW * 3), ds.cpu().numpy()[:, None]) <= TOL


def test_reference_autograd_loop_equals_weighted_partials(t1, dev):
    """The reference's loop (backproject.py:115-151) run literally through the drop-in rasterization() and autograd, with both
    targets multiplied by c: (out * feats * c[..., None]).sum() and (out0 * c[..., None]).sum()."""
    from gsbp_amd import rasterization
    cfg, sc, g = t1
    D = 32
    wf = _weights(cfg, dev, "f32")
    maps = lambda v: syn.make_feature_map(cfg, v, device=dev, dim=D)  # noqa: E731
    n = cfg.n_gaussians
    Fr, dr = torch.zeros(n, D, device=dev), torch.zeros(n, device=dev)
    for v in range(N_VIEWS):
        c = wf(v)
        colors = torch.zeros(n, D, device=dev, requires_grad=True)
        out, _, _ = rasterization(g["means"], g["quats"], g["scales"], g["opac"], colors, viewmats=g["vms"][v][None],
                                  Ks=g["K"][None], width=cfg.width, height=cfg.height, want_meta=False)
        (out[0] * maps(v) * c[..., None]).sum().backward()
        Fr += colors.grad
        colors0 = torch.zeros(n, 3, device=dev, requires_grad=True)
        out0, _, _ = rasterization(g["means"], g["quats"], g["scales"], g["opac"], colors0, viewmats=g["vms"][v][None],
                                   Ks=g["K"][None], width=cfg.width, height=cfg.height, want_meta=False)
        (out0[0] * c[..., None]).sum().backward()
        dr += colors0.grad[:, 0]
    args = (g["means"], g["quats"], g["scales"], g["opac"], g["vms"], g["K"], cfg.width, cfg.height)
    _, F, d, _ = gsbp_amd.create_feature_field(*args, maps, D, return_partials=True, pixel_weight_fn=wf)
    _check(F, d, Fr.cpu().numpy().astype(np.float64), dr.cpu().numpy().astype(np.float64))
    K = 4
    labels = lambda v: syn.make_label_map(cfg, v, K, device=dev)  # noqa: E731
    FL = torch.zeros(n, K, device=dev)
    for v in range(N_VIEWS):
        colors = torch.zeros(n, K, device=dev, requires_grad=True)
        out, _, _ = rasterization(g["means"], g["quats"], g["scales"], g["opac"], colors, viewmats=g["vms"][v][None],
                                  Ks=g["K"][None], width=cfg.width, height=cfg.height, want_meta=False)
        (out[0] * torch.nn.functional.one_hot(labels(v).long(), K).float() * wf(v)[..., None]).sum().backward()
        FL += colors.grad
    _, F2, d2, _ = gsbp_amd.create_label_field(*args, labels, K, return_partials=True, pixel_weight_fn=wf)
    _check(F2, d2, FL.cpu().numpy().astype(np.float64), dr.cpu().numpy().astype(np.float64))


def test_full_size_c2_half_mask_and_dino64(dev, orc):
    """One full-size view at C2 geometry (1M Gaussians, 1600 x 1060, D = 512) with a half-image mask, and one at DINO64 geometry
    (64 x 64 x 1024 tokens, token space, mean reduction), each against the unweighted library on c f and c."""
    for name in ("C2", "DINO64"):
        cfg = syn.CONFIGS[name]
        cfg = syn.Config(**{**cfg.__dict__, "n_views": 1})
        means, quats, scales, opac = (t.to(dev) for t in syn.activate(syn.make_scene(cfg)))
        K, vms = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg).to(dev)
        half = torch.zeros(cfg.height, cfg.width, dtype=torch.bool, device=dev)
        half[:, : cfg.width // 2] = True
        low = syn.make_feature_map(cfg, 0, device=dev)
        up = low if cfg.upsample is None else _upsampled(cfg, low, cfg.upsample)
        args = (means, quats, scales, opac, vms, K, cfg.width, cfg.height)
        kw = dict(return_partials=True, reduction=cfg.reduction)
        _, F, d, st = gsbp_amd.create_feature_field(*args, lambda v: low, cfg.feat_dim, upsample=cfg.upsample,
                                                    pixel_weight_fn=lambda v: half, **kw)
        assert st["overflow"] == 0
        _, Fr, _, _ = gsbp_amd.create_feature_field(*args, lambda v: up * half[..., None], cfg.feat_dim, **kw)
        _, dr, _, _ = gsbp_amd.create_feature_field(*args, lambda v: half[..., None].float(), 1, reduction="sum",
                                                    return_partials=True)
        if cfg.reduction == "mean":
            dr = dr / float(cfg.height * cfg.width * 3)  # d's scale under reduction="mean" (backproject.py:283)
        del up
        _check(F, d, Fr.cpu().numpy(), dr[:, 0].cpu().numpy())
        del F, d, Fr, dr, low
        torch.cuda.empty_cache()
