"""Mask-pooled features on the GPU (gwbp_scatter_mask_features, Engine.scatter_mask_features, create_mask_feature_field,
run_backproject.py --mask-features): every result must equal the back-projection of the materialised map table[L] -- a zero row
where a label is outside [0, M) -- through the C oracle and through create_feature_field, up to the order of the sums."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import rel_row_err, scene_np, to_dev

import gsbp_amd
from gsbp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4    # F and d
TOL_FIN = 1e-5  # finalised rows


def _materialise(L, table):
    """[H, W, D] float32 table[L] with a zero row wherever L is outside [0, M)."""
    L = L.to(torch.int64)
    M = table.shape[0]
    ok = ((L >= 0) & (L < M))[..., None]
    return torch.where(ok, table.float()[L.clamp(0, M - 1)], torch.zeros((), device=table.device))


@pytest.fixture(scope="module")
def t1(dev):
    cfg, sc = scene_np("T1")
    return cfg, sc, to_dev(sc, dev)


@pytest.fixture(scope="module")
def c1(dev):
    cfg, sc = scene_np("C1")
    return cfg, sc, to_dev(sc, dev)


def _blended(eng, cfg, g, v, **cam):
    view = eng.view(g["vms"][v], g["K"], cfg.width, cfg.height, **cam)
    eng.project(view, g["means"], g["quats"], g["scales"], g["opac"])
    eng.bin_sort(view)
    eng.blend_weights(view)
    return view


def _scatter(eng, view, L, table, dev, upsample=None, with_d=True):
    D = table.shape[1]
    F = torch.zeros(eng.n, D, device=dev)
    d = torch.zeros(eng.n, device=dev) if with_d else None
    eng.scatter_mask_features(view, L, table, F, d, upsample=upsample)
    st = eng.stats()
    assert st["overflow"] == 0, st
    return F, d


def _oracle(orc, cfg, sc, v, feats):
    h = [sc[k].numpy() for k in ("means", "quats", "scales", "opac")]
    Fr = np.zeros((cfg.n_gaussians, feats.shape[2]), np.float64)
    dr = np.zeros(cfg.n_gaussians, np.float64)
    info = orc.backproject_view(*h, sc["vms"][v].numpy(), sc["K"].numpy(), cfg.width, cfg.height,
                                np.ascontiguousarray(feats.cpu().numpy()), Fr, dr)
    return Fr, dr, info


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.int32, torch.int64])
def test_engine_equals_materialised_map_oracle(c1, dev, orc, dtype):
    """C1 view 0, Voronoi mask ids in [-1, M + 1] (some pixels outside the table), every label type; d given and d = NULL."""
    cfg, sc, g = c1
    M, D = 40, 64
    L, table = syn.make_mask_features(cfg, 0, M + 3, D)
    L = L - 1
    table = table[:M].contiguous()
    L = (L % 256).to(torch.uint8) if dtype == torch.uint8 else L.to(dtype)
    Fr, dr, _ = _oracle(orc, cfg, sc, 0, _materialise(L, table))
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _blended(eng, cfg, g, 0)
    F, d = _scatter(eng, view, L.to(dev), table.to(dev), dev)
    assert np.abs(Fr).max() > 0
    assert rel_row_err(F.cpu().numpy(), Fr) <= TOL
    assert rel_row_err(d.cpu().numpy()[:, None], dr[:, None]) <= TOL
    F2, _ = _scatter(eng, view, L.to(dev), table.to(dev), dev, with_d=False)
    assert rel_row_err(F2.cpu().numpy(), Fr) <= TOL


def test_all_ignored_map_adds_only_d(t1, dev):
    cfg, sc, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _blended(eng, cfg, g, 1)
    table = torch.randn(5, 8, device=dev)
    F0, d0 = _scatter(eng, view, syn.make_label_map(cfg, 1, 5).to(dev), table, dev)
    for bad in (-1, 5, 1000):
        F, d = _scatter(eng, view, torch.full((cfg.height, cfg.width), bad, dtype=torch.int32, device=dev), table, dev)
        assert float(F.abs().max()) == 0.0
        assert float((d - d0).abs().max()) <= 1e-5 * float(d0.max())


def test_mismatched_blend_is_flagged_and_left_untouched(t1, dev):
    """After blend_tokens the workspace holds no weight store: overflow bit 2, F and d untouched."""
    cfg, sc, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = eng.view(g["vms"][0], g["K"], cfg.width, cfg.height)
    eng.project(view, g["means"], g["quats"], g["scales"], g["opac"])
    eng.bin_sort(view)
    eng.blend_tokens(view, 8, 12)
    with pytest.raises(gsbp_amd.GwbpError):
        eng.scatter_mask_features(view, syn.make_label_map(cfg, 0, 4).to(dev), torch.randn(4, 8, device=dev),
                                  torch.zeros(cfg.n_gaussians, 8, device=dev), None)
    eng._tokens = None  # (the Engine refuses this itself; the C entry point is what is checked here)
    F = torch.zeros(cfg.n_gaussians, 8, device=dev)
    d = torch.zeros(cfg.n_gaussians, device=dev)
    eng.scatter_mask_features(view, syn.make_label_map(cfg, 0, 4).to(dev), torch.randn(4, 8, device=dev), F, d)
    assert eng.stats()["overflow"] & 4
    assert float(F.abs().max()) == 0.0 and float(d.abs().max()) == 0.0


def test_engine_refuses_token_blend_and_bad_inputs(t1, dev):
    cfg, sc, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _blended(eng, cfg, g, 0)
    F = torch.zeros(cfg.n_gaussians, 8, device=dev)
    L = syn.make_label_map(cfg, 0, 4)
    tab = torch.randn(4, 8, device=dev)
    for bad_l, bad_t in ((L, tab), (L.float().to(dev), tab), (L.to(dev)[:-1], tab), (L.to(dev), tab.cpu()),
                         (L.to(dev), tab.to(torch.float64)), (L.to(dev), tab[None]), (L.to(dev), tab[:, :4])):
        with pytest.raises(gsbp_amd.GwbpError):
            eng.scatter_mask_features(view, bad_l, bad_t, F, None)


def test_spill_path_per_pixel_random(t1, dev, orc):
    """An independent mask id per pixel: records with far more than four distinct labels spill; still table[L]'s result."""
    cfg, sc, g = t1
    M, D = 300, 64
    L, table = syn.make_mask_features(cfg, 0, M, D, per_pixel=True)
    Fr, dr, _ = _oracle(orc, cfg, sc, 0, _materialise(L, table))
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _blended(eng, cfg, g, 0)
    before = int(eng.mask_spilled.item()) if getattr(eng, "mask_spilled", None) is not None else 0
    F, d = _scatter(eng, view, L.to(dev), table.to(dev), dev)
    assert int(eng.mask_spilled.item()) - before > 0
    assert rel_row_err(F.cpu().numpy(), Fr) <= TOL
    assert rel_row_err(d.cpu().numpy()[:, None], dr[:, None]) <= TOL


def test_bit_identical_without_spills(c1, dev):
    """Three masks (with -1, at most four distinct keys per record): nothing spills, F and d are the same bit for bit."""
    cfg, sc, g = c1
    L, table = syn.make_mask_features(cfg, 0, 4, 256, device=dev)
    L = L - 1
    table = table[:3].contiguous()
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _blended(eng, cfg, g, 0)
    F1, d1 = _scatter(eng, view, L, table, dev)
    F2, d2 = _scatter(eng, view, L, table, dev)
    assert int(eng.mask_spilled.item()) == 0
    assert float(F1.abs().max()) > 0
    assert torch.equal(F1, F2) and torch.equal(d1, d2)


def _field_vs_materialised(cfg, g, mask_fn, dim, upsample=None, **kw):
    """create_mask_feature_field against create_feature_field(table[L], return_partials=True)."""
    args = (g["means"], g["quats"], g["scales"], g["opac"], g["vms"], g["K"], cfg.width, cfg.height)
    out, F, d, st = gsbp_amd.create_mask_feature_field(*args, mask_fn, dim, upsample=upsample, return_partials=True, **kw)

    def feature_fn(v):
        L, table = mask_fn(v)
        return _materialise(L, table)
    _, Fo, do, _ = gsbp_amd.create_feature_field(*args, feature_fn, dim, upsample=upsample, return_partials=True,
                                                 **{k: v for k, v in kw.items() if k != "engine"})
    ref = gsbp_amd.finalize_reference(Fo, do)
    assert out.shape == (cfg.n_gaussians, dim) and st["overflow"] == 0
    assert float(Fo.abs().max()) > 0
    assert rel_row_err(F.cpu().numpy(), Fo.cpu().numpy()) <= TOL
    assert rel_row_err(d.cpu().numpy()[:, None], do.cpu().numpy()[:, None]) <= TOL
    assert float((out - ref).abs().max()) <= TOL_FIN
    return out, F, d, st


@pytest.mark.parametrize("pipeline", [True, False])
@pytest.mark.parametrize("cam", [dict(), dict(camera_model="fisheye"), dict(rasterize_mode="antialiased")])
def test_field_equals_feature_field_on_materialised_maps(c1, dev, pipeline, cam):
    cfg, sc, g = c1
    maps = {}
    for v in range(cfg.n_views):  # M differs per view; some ids outside the table
        L, t = syn.make_mask_features(cfg, v, 30 + 7 * v, 128, device=dev)
        maps[v] = (L - 1, t[: 28 + 7 * v].contiguous())
    _field_vs_materialised(cfg, g, maps.__getitem__, 128, pipeline=pipeline, **cam)


def test_pipelined_and_serial_drivers_agree(c1, dev):
    cfg, sc, g = c1
    maps = {v: syn.make_mask_features(cfg, v, 50, 96, device=dev) for v in range(cfg.n_views)}
    args = (g["means"], g["quats"], g["scales"], g["opac"], g["vms"], g["K"], cfg.width, cfg.height, maps.__getitem__, 96)
    _, Fp, dp, _ = gsbp_amd.create_mask_feature_field(*args, pipeline=True, return_partials=True)
    _, Fs, ds, _ = gsbp_amd.create_mask_feature_field(*args, pipeline=False, return_partials=True)
    assert rel_row_err(Fp.cpu().numpy(), Fs.cpu().numpy()) <= TOL
    assert rel_row_err(dp.cpu().numpy()[:, None], ds.cpu().numpy()[:, None]) <= TOL


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_tables(c1, dev, dtype):
    cfg, sc, g = c1
    maps = {v: (lambda m: (m[0], m[1].to(dtype)))(syn.make_mask_features(cfg, v, 60, 256, device=dev))
            for v in range(cfg.n_views)}
    _field_vs_materialised(cfg, g, maps.__getitem__, 256)


def test_low_resolution_maps_nearest(c1, dev):
    cfg, sc, g = c1
    maps = {v: syn.make_mask_features(cfg, v, 40, 64, device=dev, size=(37, 53)) for v in range(cfg.n_views)}
    _field_vs_materialised(cfg, g, maps.__getitem__, 64, upsample="nearest")


@pytest.mark.parametrize("kind", ["mask", "confidence"])
def test_pixel_weights(c1, dev, kind):
    cfg, sc, g = c1
    maps = {v: syn.make_mask_features(cfg, v, 40, 64, device=dev) for v in range(cfg.n_views)}
    _field_vs_materialised(cfg, g, maps.__getitem__, 64,
                           pixel_weight_fn=lambda v: syn.make_pixel_weights(cfg, v, device=dev, kind=kind))


def test_mean_reduction(c1, dev):
    cfg, sc, g = c1
    maps = {v: syn.make_mask_features(cfg, v, 40, 64, device=dev) for v in range(cfg.n_views)}
    _field_vs_materialised(cfg, g, maps.__getitem__, 64, reduction="mean")


@pytest.mark.parametrize("dim", [3, 130])
def test_narrow_widths_take_the_fallback(c1, dev, dim):
    cfg, sc, g = c1
    assert not gsbp_amd.Engine.mask_fast_path(dim)
    maps = {v: syn.make_mask_features(cfg, v, 40, dim, device=dev) for v in range(cfg.n_views)}
    _field_vs_materialised(cfg, g, maps.__getitem__, dim)


@pytest.fixture(scope="module")
def c2(dev):
    cfg = syn.CONFIGS["C2"]
    means, quats, scales, opac = syn.activate(syn.make_scene(cfg))
    sc = dict(means=means, quats=quats, scales=scales, opac=opac, vms=syn.make_cameras(cfg, n_views=2), K=syn.intrinsics(cfg))
    return cfg, sc, to_dev(sc, dev)


def test_c2_geometry_one_view_against_oracle_and_feature_field(c2, dev, orc):
    cfg, sc, g = c2
    M, D = 200, 512
    L, table = syn.make_mask_features(cfg, 0, M, D)
    feats = _materialise(L, table)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, tight_binning=True)
    view = _blended(eng, cfg, g, 0)
    F, d = _scatter(eng, view, L.to(dev), table.to(dev), dev)
    Fr, dr, _ = _oracle(orc, cfg, sc, 0, feats)
    assert rel_row_err(F.cpu().numpy(), Fr) <= TOL
    assert rel_row_err(d.cpu().numpy()[:, None], dr[:, None]) <= TOL
    Ff = torch.zeros_like(F)
    df = torch.zeros_like(d)
    eng.scatter(view, feats.to(dev), Ff, df)
    assert rel_row_err(F.cpu().numpy(), Ff.cpu().numpy()) <= TOL
    out, ref = eng.finalize(F, d), gsbp_amd.finalize_reference(Ff, df)
    assert float((out - ref).abs().max()) <= TOL_FIN


def test_cli_mask_features(dev, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_backproject.py"), "--synthetic", "C1", "--mask-features",
                        "synthetic", "--num-masks", "50", "--no-prune", "--results-dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = torch.load(tmp_path / "features_lseg.pt")
    cfg = syn.CONFIGS["C1"]
    means, quats, scales, opac = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    ref = gsbp_amd.create_mask_feature_field(means, quats, scales, opac, syn.make_cameras(cfg), syn.intrinsics(cfg), cfg.width,
                                             cfg.height, lambda v: syn.make_mask_features(cfg, v, 50, cfg.feat_dim, device=dev),
                                             cfg.feat_dim).cpu()
    assert out.shape == (cfg.n_gaussians, cfg.feat_dim)
    assert float((out - ref).abs().max()) <= TOL_FIN
