"""The two ways the post-lift modules reach a projected view (gsbp_amd._views), through their public callers: the grow-and-retry
branch of the pass over many views (score_label_views, score_field_views) and the reuse of rasterization()'s front cache by the
one-view calls (render_label_maps, render_label_argmax, probe_pixels, render_field_agreement).  Scene: T1 with four views, the one
on which tests/test_gpu_parity.py forces growth with isect_cap=3000."""
import pytest
import torch

import gsbp_amd
from gsbp_amd import synthetic as syn
from gsbp_amd.rasterization import _ENGINES

from util import scene_np, to_dev

pytestmark = pytest.mark.gpu
N_VIEWS, K_CLASSES, DIM, SKIPPED = 4, 7, 24, 1


@pytest.fixture(scope="module")
def t1(dev):
    cfg, sc = scene_np("T1", n_views=N_VIEWS)
    g = to_dev(sc, dev)
    gen = torch.Generator().manual_seed(5)
    labels = torch.randint(0, K_CLASSES, (cfg.n_gaussians,), generator=gen).to(dev)
    field = torch.randn(cfg.n_gaussians, DIM, generator=gen).to(dev)
    gts = [syn.make_label_map(cfg, v, K_CLASSES).to(dev) for v in range(N_VIEWS)]
    maps = [syn.make_feature_map(cfg, v, device=dev) for v in range(N_VIEWS)]
    return cfg, g, (g["means"], g["quats"], g["scales"], g["opac"]), labels, field, gts, maps


def _score(which, t1):
    cfg, g, gauss, labels, field, gts, maps = t1
    if which == "labels":
        return gsbp_amd.score_label_views(*gauss, labels, K_CLASSES, g["vms"], g["K"], cfg.width, cfg.height,
                                          lambda v: None if v == SKIPPED else gts[v])
    return gsbp_amd.score_field_views(*gauss, field, g["vms"], g["K"], cfg.width, cfg.height,
                                      lambda v: None if v == SKIPPED else maps[v])


@pytest.mark.parametrize("which", ["labels", "field"])
def test_a_pass_that_overflows_grows_the_workspace_and_gives_the_same_bits(dev, t1, which):
    cfg, g = t1[0], t1[1]
    key = (str(g["means"].device), cfg.n_gaussians, cfg.width, cfg.height)
    _ENGINES.pop(key, None)
    want = _score(which, t1)  # on a fresh engine of default capacities
    n_isect = _ENGINES[key].stats()["n_isect"]  # of the view scored last
    print(f"{which}: n_isect of the last view {n_isect}, default isect_cap {_ENGINES[key].isect_cap}")
    assert n_isect > 3000  # the small engine below cannot hold the view: its first pass must overflow
    del _ENGINES[key]
    small = _ENGINES[key] = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, isect_cap=3000)
    got = _score(which, t1)
    assert got.dtype == want.dtype and torch.equal(got.view(torch.int64), want.view(torch.int64))
    assert _ENGINES[key] is small and small.isect_cap > 3000
    live = [v for v in range(N_VIEWS) if v != SKIPPED]
    for t in (want, got):
        assert not bool(t[SKIPPED].any()) and all(bool(t[v].any()) for v in live)
    del _ENGINES[key]  # (the grown engine is nobody else's default)


def test_one_view_calls_after_a_rendered_frame_project_what_they_did_before(dev, t1, monkeypatch):
    cfg, g, gauss, labels, _, _, _ = t1
    W, H = cfg.width, cfg.height
    gen = torch.Generator().manual_seed(6)
    field = torch.randn(cfg.n_gaussians, 32, generator=gen).to(dev)
    K = g["K"]
    calls = []
    orig = gsbp_amd.Engine.project

    def project(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(gsbp_amd.Engine, "project", project)

    def counted(fn):
        before = len(calls)
        fn()
        return len(calls) - before

    def after_a_frame_of(colors, v):
        vm, fmap = g["vms"][v], syn.make_feature_map(cfg, v, device=dev, dim=32)
        frame = counted(lambda: gsbp_amd.rasterization(*gauss, colors, g["vms"][v:v + 1], K[None], W, H, want_meta=False))
        return [frame,
                counted(lambda: gsbp_amd.render_label_maps(*gauss, labels, K_CLASSES, vm, K, W, H)),
                counted(lambda: gsbp_amd.render_label_argmax(*gauss, labels, K_CLASSES, vm, K, W, H)),
                counted(lambda: gsbp_amd.probe_pixels(*gauss, field, vm, K, W, H, [[100, 60], [3, 130]])),
                counted(lambda: gsbp_amd.render_field_agreement(*gauss, field, fmap, vm, K, W, H))]

    narrow = after_a_frame_of(field[:, :3].contiguous(), 0)  # a 3-channel frame: rendered pixel-parallel, no weight store is blended
    wide = after_a_frame_of(field, 1)                        # a 32-channel frame: rendered from the weight store, alphas kept
    print("Engine.project calls [frame, label maps, label argmax, probe, agreement]: after an RGB frame", narrow,
          "after a 32-channel frame", wide)
    # The counts of the commit before the helpers were shared: the front cache is host logic, and these are what that commit's
    # run_front gives for the same calls (worked out there on a stand-in engine; not yet recorded on a device).  The first three
    # re-project nothing, as their docstrings promise; the agreement needs the weight store and its alphas, which only the wide
    # frame leaves behind.
    assert narrow == [1, 0, 0, 0, 1]
    assert wide == [1, 0, 0, 0, 0]
