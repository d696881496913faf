"""Integer label maps on the GPU (gwbp_scatter_labels, Engine.scatter_labels, create_label_field, run_backproject.py
--num-classes): every result must equal the back-projection of one_hot(L, K).float() -- through the C oracle, through
create_feature_field and through the reference's own autograd loop -- up to the order of the atomic sums.  A label outside
[0, K) is an all-zero one-hot row: nothing in F, its weight still in d."""
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
TOL = 1e-5


def _one_hot(L, K):
    """[H, W, K] float32 one-hot of the label values as stored; ids outside [0, K) give an all-zero row."""
    L = L.to(torch.int64)
    ok = (L >= 0) & (L < K)
    oh = torch.zeros(*L.shape, K, device=L.device)
    return oh.scatter_(-1, torch.where(ok, L, 0)[..., None], ok[..., None].float())


@pytest.fixture(scope="module")
def t1(dev):
    cfg, sc = scene_np("T1")
    return cfg, sc, to_dev(sc, dev)


def _blended(eng, cfg, g, v, wide=False, **cam):
    eng.set_narrow_scatter(not wide)
    view = eng.view(g["vms"][v], g["K"], cfg.width, cfg.height, **cam)
    eng.project(view, g["means"], g["quats"], g["scales"], g["opac"])
    eng.bin_sort(view)
    eng.blend_weights(view)
    return view


def _labels(eng, view, L, K, dev, upsample=None, with_d=True):
    F = torch.zeros(eng.n, K, device=dev)
    d = torch.zeros(eng.n, device=dev) if with_d else None
    eng.scatter_labels(view, L, F, d, K, upsample=upsample)
    st = eng.stats()
    assert st["overflow"] == 0, st
    return F, d, st


def _oracle(orc, cfg, sc, v, oh):
    h = [sc[k].numpy() for k in ("means", "quats", "scales", "opac")]
    Fr = np.zeros((cfg.n_gaussians, oh.shape[2]), np.float64)
    dr = np.zeros(cfg.n_gaussians, np.float64)
    info = orc.backproject_view(*h, sc["vms"][v].numpy(), sc["K"].numpy(), cfg.width, cfg.height,
                                np.ascontiguousarray(oh.cpu().numpy()), Fr, dr)
    return Fr, dr, info


DTYPES = [torch.uint8, torch.int16, torch.int32, torch.int64]


@pytest.mark.parametrize("K", [1, 5, 64, 300])
@pytest.mark.parametrize("dtype", DTYPES)
def test_scatter_labels_equals_one_hot_oracle(t1, dev, orc, K, dtype):
    """T1 view 0, Voronoi labels in [-1, K + 1] (so some ids are ignored), every native element type and int64; both store
    layouts (narrow: one run per record; wide: half-tile lists padded between the halves)."""
    cfg, sc, g = t1
    L = syn.make_label_map(cfg, 0, K + 3) - 1
    L = (L % 256).to(torch.uint8) if dtype == torch.uint8 else L.to(dtype)
    Fr, dr, info = _oracle(orc, cfg, sc, 0, _one_hot(L, K))
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    for wide in (False, True):
        view = _blended(eng, cfg, g, 0, wide=wide)
        F, d, st = _labels(eng, view, L.to(dev), K, dev)
        assert st["n_pairs"] == info["n_pairs"]
        assert np.abs(Fr).max() > 0 or K == 1
        assert rel_row_err(F.cpu().numpy(), Fr) <= TOL, (K, dtype, wide)
        assert rel_row_err(d.cpu().numpy()[:, None], dr[:, None]) <= TOL
        # d = NULL (what the pipelined driver passes): F alone, the same F
        F2, _, _ = _labels(eng, view, L.to(dev), K, dev, with_d=False)
        assert rel_row_err(F2.cpu().numpy(), Fr) <= TOL


def test_ignored_and_single_class_maps(t1, dev):
    cfg, sc, g = t1
    K = 6
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _blended(eng, cfg, g, 1)
    F0, d0, _ = _labels(eng, view, syn.make_label_map(cfg, 1, K).to(dev), K, dev)
    for bad in (-1, K, 1000):
        F, d, _ = _labels(eng, view, torch.full((cfg.height, cfg.width), bad, dtype=torch.int32, device=dev), K, dev)
        assert float(F.abs().max()) == 0.0
        assert float((d - d0).abs().max()) <= 1e-6 * float(d0.max())
    k = 4
    F, d, _ = _labels(eng, view, torch.full((cfg.height, cfg.width), k, dtype=torch.int16, device=dev), K, dev)
    assert float(d.max()) > 0
    assert float((F[:, k] - d).abs().max()) <= 1e-6 * float(d.max())
    others = torch.cat([F[:, :k], F[:, k + 1:]], dim=1)
    assert float(others.abs().max()) == 0.0


def test_store_without_weights_is_flagged_and_left_untouched(t1, dev):
    """After the fused blend + scatter kernel the workspace holds no weight store: overflow bit 2, F and d untouched."""
    cfg, sc, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = eng.view(g["vms"][0], g["K"], cfg.width, cfg.height)
    eng.project(view, g["means"], g["quats"], g["scales"], g["opac"])
    eng.bin_sort(view)
    feats = syn.make_feature_map(cfg, 0, device=dev, dim=4)
    eng.blend_scatter(view, feats, torch.zeros(cfg.n_gaussians, 4, device=dev), None)
    F = torch.zeros(cfg.n_gaussians, 3, device=dev)
    d = torch.zeros(cfg.n_gaussians, device=dev)
    eng.scatter_labels(view, syn.make_label_map(cfg, 0, 3).to(dev), F, d, 3)
    assert eng.stats()["overflow"] & 4
    assert float(F.abs().max()) == 0.0 and float(d.abs().max()) == 0.0


def test_per_pixel_random_labels_k1000(t1, dev, orc):
    """The worst case of the key reduction: an independent id per pixel, K = 1000 (more distinct labels per record than leader
    rounds: the rest add entry by entry)."""
    cfg, sc, g = t1
    K = 1000
    L = syn.make_label_map(cfg, 0, K, per_pixel=True)
    Fr, dr, _ = _oracle(orc, cfg, sc, 0, _one_hot(L, K))
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    for wide in (False, True):
        view = _blended(eng, cfg, g, 0, wide=wide)
        F, d, _ = _labels(eng, view, L.to(dev), K, dev)
        assert rel_row_err(F.cpu().numpy(), Fr) <= TOL
        assert rel_row_err(d.cpu().numpy()[:, None], dr[:, None]) <= TOL


def test_low_resolution_map_with_nearest_upsampling(t1, dev):
    cfg, sc, g = t1
    K = 9
    low = syn.make_label_map(cfg, 1, K, size=(23, 37), n_seeds=40).to(torch.int16).to(dev)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _blended(eng, cfg, g, 1)
    ymap, xmap = eng.nearest_maps(23, 37, cfg.height, cfg.width)
    full = low[ymap.long()][:, xmap.long()]
    ref = torch.nn.functional.interpolate(low[None, None].float(), size=(cfg.height, cfg.width), mode="nearest")[0, 0]
    assert torch.equal(full.float(), ref)
    F1, d1, _ = _labels(eng, view, low, K, dev, upsample="nearest")
    F2, d2, _ = _labels(eng, view, full, K, dev)
    assert rel_row_err(F1.cpu().numpy(), F2.cpu().numpy()) <= 1e-6
    assert rel_row_err(d1.cpu().numpy()[:, None], d2.cpu().numpy()[:, None]) <= 1e-6
    with pytest.raises(gsbp_amd.GwbpError):
        _labels(eng, view, low, K, dev)  # a low-resolution map without upsample="nearest"


def test_engine_rejects_bad_label_inputs(t1, dev):
    cfg, sc, g = t1
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    view = _blended(eng, cfg, g, 0)
    F = torch.zeros(cfg.n_gaussians, 4, device=dev)
    L = syn.make_label_map(cfg, 0, 4)
    for bad in (L, L.float().to(dev), L.to(dev)[None], L.to(dev)[:-1]):
        with pytest.raises(gsbp_amd.GwbpError):
            eng.scatter_labels(view, bad, F, None, 4)
    with pytest.raises(gsbp_amd.GwbpError):
        eng.scatter_labels(view, L.to(dev), torch.zeros(cfg.n_gaussians, 3, device=dev), None, 4)


def _fractions(F, d):
    return torch.where(d[:, None] > 0, F / d.clamp_min(1e-30)[:, None], torch.zeros_like(F))


def _field_vs_one_hot(cfg, g, label_fn, K, views=None, **kw):
    """create_label_field against create_feature_field(one_hot, return_partials=True)'s F / d."""
    args = (g["means"], g["quats"], g["scales"], g["opac"], g["vms"], g["K"], cfg.width, cfg.height)
    P, F, d, st = gsbp_amd.create_label_field(*args, label_fn, K, views=views, return_partials=True, **kw)
    _, Fo, do, _ = gsbp_amd.create_feature_field(*args, lambda v: _one_hot(label_fn(v), K), K, views=views, return_partials=True,
                                                 **{k: v for k, v in kw.items() if k != "engine"})
    assert P.shape == (cfg.n_gaussians, K) and st["overflow"] == 0
    assert rel_row_err(F.cpu().numpy(), Fo.cpu().numpy()) <= TOL
    assert rel_row_err(d.cpu().numpy()[:, None], do.cpu().numpy()[:, None]) <= TOL
    assert float((P - _fractions(Fo, do)).abs().max()) <= TOL
    assert float(P.min()) >= 0.0 and float(P.sum(dim=1).max()) <= 1.0 + 1e-5
    return P, F, d


@pytest.mark.parametrize("camera_model", ["pinhole", "ortho", "fisheye"])
@pytest.mark.parametrize("rasterize_mode", ["classic", "antialiased"])
@pytest.mark.parametrize("pipeline", [True, False])
def test_create_label_field_equals_one_hot_feature_field(t1, dev, camera_model, rasterize_mode, pipeline):
    cfg, sc, g = t1
    K = 5
    maps = {v: (syn.make_label_map(cfg, v, K + 1) - 1).to(dev) for v in range(cfg.n_views)}  # some pixels ignored (-1)
    P, _, d = _field_vs_one_hot(cfg, g, maps.__getitem__, K, pipeline=pipeline, camera_model=camera_model,
                                rasterize_mode=rasterize_mode)
    assert float(d.max()) > 0 and float(P.sum(dim=1).max()) > 0.5


@pytest.mark.parametrize("pipeline", [True, False])
def test_small_capacities_grow_and_retry(t1, dev, pipeline):
    cfg, sc, g = t1
    K = 7
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, isect_cap=3000, pair_cap=1 << 15,
                          tight_binning=True)
    maps = {v: syn.make_label_map(cfg, v, K).to(dev) for v in range(cfg.n_views)}
    _field_vs_one_hot(cfg, g, maps.__getitem__, K, pipeline=pipeline, engine=eng)
    assert eng.isect_cap > 3000


@pytest.fixture(scope="module")
def c2(dev):
    cfg = syn.CONFIGS["C2"]
    means, quats, scales, opac = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    return cfg, dict(means=means, quats=quats, scales=scales, opac=opac, vms=syn.make_cameras(cfg, n_views=4),
                     K=syn.intrinsics(cfg))


def test_c2_geometry_one_view_against_oracle(c2, dev, orc):
    cfg, g = c2
    K = 64
    L = syn.make_label_map(cfg, 0, K)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, tight_binning=True)
    view = _blended(eng, cfg, g, 0)
    F, d, st = _labels(eng, view, L.to(dev), K, dev)
    sc = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in g.items()}
    Fr, dr, info = _oracle(orc, cfg, sc, 0, _one_hot(L, K))
    assert st["n_pairs"] == info["n_pairs"]
    assert rel_row_err(F.cpu().numpy(), Fr) <= TOL
    assert rel_row_err(d.cpu().numpy()[:, None], dr[:, None]) <= TOL


def test_c2_geometry_four_pipelined_views_against_one_hot_driver(c2, dev):
    cfg, g = c2
    K = 64
    _field_vs_one_hot(cfg, g, lambda v: syn.make_label_map(cfg, v, K, device=dev), K, pipeline=True)


def test_reference_autograd_loop_equals_label_partials(dev):
    """The literal reference loop (backproject.py:115-151) at C1 through the drop-in rasterization(): per view
    (render(zeros[N, K]) * one_hot).sum().backward() for F and render(zeros[N, 3]).sum().backward()[:, 0] for d."""
    from gsbp_amd import rasterization
    cfg, sc = scene_np("C1")
    g = to_dev(sc, dev)
    K, N, W, H = 8, cfg.n_gaussians, cfg.width, cfg.height
    maps = {v: syn.make_label_map(cfg, v, K).to(dev) for v in range(cfg.n_views)}
    args = (g["means"], g["quats"], g["scales"], g["opac"])
    F = torch.zeros(N, K, device=dev)
    d = torch.zeros(N, device=dev)
    for v in range(cfg.n_views):
        colors = torch.zeros(N, K, device=dev, requires_grad=True)
        out, _, _ = rasterization(*args, colors, g["vms"][v][None], g["K"][None], width=W, height=H, want_meta=False)
        (out[0] * _one_hot(maps[v], K)).sum().backward()
        F += colors.grad
        c3 = torch.zeros(N, 3, device=dev, requires_grad=True)
        out3, _, _ = rasterization(*args, c3, g["vms"][v][None], g["K"][None], width=W, height=H, want_meta=False)
        out3.sum().backward()
        d += c3.grad[:, 0]
    P, Fl, dl, _ = gsbp_amd.create_label_field(*args, g["vms"], g["K"], W, H, maps.__getitem__, K, return_partials=True)
    assert rel_row_err(Fl.cpu().numpy(), F.cpu().numpy()) <= TOL
    assert rel_row_err(dl.cpu().numpy()[:, None], d.cpu().numpy()[:, None]) <= TOL
    assert float((P - _fractions(F, d)).abs().max()) <= TOL


def _cli(tmp, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_backproject.py"), "--synthetic", "C1", "--num-classes", "8",
                        "--results-dir", str(tmp), *flags], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_label_field_pruned_and_unpruned(dev, tmp_path):
    a, b = tmp_path / "pruned", tmp_path / "all"
    _cli(a)
    _cli(b, "--no-prune")
    keep = torch.load(a / "prune_mask.pt")
    pa, pb = torch.load(a / "label_field.pt"), torch.load(b / "label_field.pt")
    assert not (b / "prune_mask.pt").exists() and not (a / "features_lseg.pt").exists()
    assert pa.shape == (int(keep.sum()), 8) and pb.shape == (10000, 8) and 0 < int(keep.sum()) < 10000
    for p in (pa, pb):
        assert float(p.min()) >= 0.0 and float(p.max()) <= 1.0 + 1e-6 and float(p.sum(dim=1).max()) <= 1.0 + 1e-5
    cfg = syn.CONFIGS["C1"]
    means, quats, scales, opac = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    vms, K = syn.make_cameras(cfg), syn.intrinsics(cfg)

    def label_fn(v):
        return syn.make_label_map(cfg, v, 8, device=dev)
    ref_b = gsbp_amd.create_label_field(means, quats, scales, opac, vms, K, cfg.width, cfg.height, label_fn, 8).cpu()
    assert float((pb - ref_b).abs().max()) <= TOL
    k = keep.to(dev)
    ref_a = gsbp_amd.create_label_field(means[k], quats[k], scales[k], opac[k], vms, K, cfg.width, cfg.height, label_fn, 8).cpu()
    assert float((pa - ref_a).abs().max()) <= TOL
