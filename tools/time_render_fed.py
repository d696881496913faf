#!/usr/bin/env python3
"""The reference's whole per-view loop -- render the view with SH degree 3, run the 2-D network on the render, lift its map
(backproject.py:89-151, :223-283) -- at full size: ms per view of

  plain          create_feature_field on a precomputed map (no render, no network): the lift alone
  raster         feature_fn(v) = net(rasterization(..., colors_all, sh_degree=3)): a second front per view (today's way)
  render_fed     create_feature_field(render_colors=colors_all, sh_degree=3), feature_fn(v, image) = net(image): the lift's
                 front renders the view (the storing / token blends composite it while they blend)
  render_px      render_fed with ViewPipeline.RENDER_IN_BLEND off: gwbp_render_pixels on the same workspace after bin_sort

The stub network is the same function of the image in raster, render_fed and render_px: image @ W[3, D] at full resolution
(C2, C5), a box pool to the config's low-resolution grid then @ W (DINO64, LSEG480).  The forms of one config ALTERNATE inside
every round so that drift hits them alike; hip events around each whole call after one untimed call; the last of --rounds
rounds is reported.  C2N is C2 with allow_wide=False: its front blends with the 128-channel kernel's store (kStore).

"blend_alone" (--blend-reps > 0): the front's blend of one view by itself, on one stream with nothing beside it, per config in
the blend mode its pipeline uses (C2, LSEG480: kHalves with d; C2N: kStore; DINO64: kToken) -- plain, with the composite, and
render_pixels + plain; project + bin_sort before every repetition, hip events around the blend (and the render) only, median
of the repetitions, the variants alternating.  The recorded profiles/render_fed.json is

    timeout -k 10 1500 python tools/time_render_fed.py --out profiles/render_fed.json

and the kernel times of the same isolated blends come from a run of their own:

    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -o kstats -- \
        python tools/time_render_fed.py --configs C2,C2N,DINO64 --views 0 --blend-reps 20
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gsbp_amd  # noqa: E402  (before the first HIP call: hardware queues)
import torch  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402

RENDER_OFF = {"store": False, "halves": False, "tokens": False}
# config name -> (BASELINE config, extra create_feature_field keywords, the blend its pipeline's front runs)
VARIANTS = {"C2": ("C2", {}, "halves"), "C2N": ("C2", dict(allow_wide=False), "store"), "DINO64": ("DINO64", {}, "tokens"),
            "LSEG480": ("LSEG480", {}, "halves"), "C5": ("C5", {}, None)}


def _events(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def _net(cfg, dev):
    D = cfg.feat_dim
    W = torch.randn(3, D, generator=torch.Generator(device="cpu").manual_seed(5)).to(dev)
    if cfg.lowres is None:
        return lambda image: image @ W

    def net(image):
        pooled = torch.nn.functional.adaptive_avg_pool2d(image.permute(2, 0, 1)[None], cfg.lowres)[0].permute(1, 2, 0)
        return (pooled @ W).contiguous()
    return net


def run_config(name, views, rounds, dev):
    base, extra, _ = VARIANTS[name]
    cfg = syn.CONFIGS[base]
    g = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    vms, K = syn.make_cameras(cfg, n_views=views).to(dev), syn.intrinsics(cfg).to(dev)
    sh = syn.make_sh_coeffs(cfg, 3, device=dev)
    feats = syn.make_feature_map(cfg, 0, device=dev)
    enc = syn.make_encoder(cfg).to(dev) if cfg.encoder_dim else None
    args = (*g, vms, K, cfg.width, cfg.height)
    kw = dict(upsample=cfg.upsample, reduction=cfg.reduction, encoder=enc, **extra)
    net = _net(cfg, dev)

    def raster(v):
        img, _, _ = gsbp_amd.rasterization(*g, sh, vms[v][None], K[None], cfg.width, cfg.height, sh_degree=3, want_meta=False)
        return net(img[0])

    def render_px():
        saved = gsbp_amd.ViewPipeline.RENDER_IN_BLEND
        gsbp_amd.ViewPipeline.RENDER_IN_BLEND = RENDER_OFF
        try:
            gsbp_amd.create_feature_field(*args, lambda v, image: net(image), cfg.feat_dim, render_colors=sh, sh_degree=3, **kw)
        finally:
            gsbp_amd.ViewPipeline.RENDER_IN_BLEND = saved

    jobs = {
        "plain": lambda: gsbp_amd.create_feature_field(*args, lambda v: feats, cfg.feat_dim, **kw),
        "raster": lambda: gsbp_amd.create_feature_field(*args, raster, cfg.feat_dim, **kw),
        "render_fed": lambda: gsbp_amd.create_feature_field(*args, lambda v, image: net(image), cfg.feat_dim, render_colors=sh,
                                                            sh_degree=3, **kw),
        "render_px": render_px,
    }
    rows = {}
    for r in range(rounds):
        for k, fn in jobs.items():
            fn()
            ms = _events(fn) / views
            rows[k] = dict(config=name, form=k, ms_view=round(ms, 4), round=r)
        for k in rows:
            rows[k]["minus_plain"] = round(rows[k]["ms_view"] - rows["plain"]["ms_view"], 4)
        rows["render_fed"]["saved_vs_raster"] = round(rows["raster"]["ms_view"] - rows["render_fed"]["ms_view"], 4)
        print(json.dumps(list(rows.values())), flush=True)
    del feats
    torch.cuda.empty_cache()
    return list(rows.values())


def blend_alone(name, reps, dev):
    """The front's blend of view 0 alone: plain / composite / render_pixels + plain, ms (hip events, median of `reps`)."""
    base, _, mode = VARIANTS[name]
    if mode is None:
        return []
    cfg = syn.CONFIGS[base]
    g = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    vm, K = syn.make_cameras(cfg, n_views=1)[0], syn.intrinsics(cfg)
    sh = syn.make_sh_coeffs(cfg, 3, device=dev)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, tight_binning=True)
    eng.set_narrow_scatter(mode == "store")
    view = eng.view(vm, K, cfg.width, cfg.height)
    cols = eng.view_colors(view, g[0], sh, 3)
    image = torch.empty(cfg.height, cfg.width, 3, device=dev)
    d = torch.zeros(cfg.n_gaussians, device=dev) if mode == "halves" else None

    def plain():
        if mode == "tokens":
            eng.blend_tokens(view, *cfg.lowres)
        else:
            eng.blend_weights(view, d=d)

    def composite():
        if mode == "tokens":
            eng.blend_tokens_rgb(view, *cfg.lowres, cols, image)
        else:
            eng.blend_weights_rgb(view, cols, image, d=d)

    def render_px():
        eng.render_rgb(view, cols, image)
        plain()

    variants = {"plain": plain, "composite": composite, "render_px_then_plain": render_px}
    times = {k: [] for k in variants}
    for r in range(reps + 1):
        for k, fn in variants.items():
            eng.project(view, *g)
            eng.bin_sort(view)
            torch.cuda.synchronize()
            ms = _events(fn)
            if r > 0:  # (the first round warms up)
                times[k].append(ms)
    assert eng.stats()["overflow"] == 0
    rows = []
    for k, v in times.items():
        v = sorted(v)
        rows.append(dict(config=name, blend=mode, variant=k, median_ms=round(v[len(v) // 2], 4), min_ms=round(v[0], 4),
                         reps=len(v)))
    print(json.dumps(rows), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C2N,DINO64,LSEG480,C5")
    ap.add_argument("--views", type=int, default=24, help="views per timed call (0: no end-to-end timing)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blend-reps", type=int, default=20, help="repetitions of the isolated blends (0: none)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows, alone = [], []
    for name in a.configs.split(","):
        if a.views > 0:
            rows += run_config(name, a.views, a.rounds, dev)
        if a.blend_reps > 0:
            alone += blend_alone(name, a.blend_reps, dev)
            torch.cuda.empty_cache()
    res = dict(tool="tools/time_render_fed.py", device=torch.cuda.get_device_name(0), views=a.views, rounds=a.rounds,
               blend_reps=a.blend_reps, date=time.strftime("%Y-%m-%d"), rows=rows, blend_alone=alone)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
