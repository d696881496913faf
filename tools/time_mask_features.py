#!/usr/bin/env python3
"""Mask-pooled features at C2 geometry (1 M Gaussians, 1600 x 1060, D = 512): create_mask_feature_field against what a user
does without it, alternating the variants in one process.

    timeout -k 10 1500 python tools/time_mask_features.py --out profiles/mask_features.json

Per view (hip events around a whole create_* call over --views views, after one untimed call; every variant once per round,
--rounds rounds, all rounds reported):
  (a) masks          create_mask_feature_field on (labels, table) pairs built once (200-mask Voronoi maps, int32, fp32 tables)
  (b) materialise    create_feature_field whose feature_fn builds table[L] (a zero row outside [0, M)) per view
  (c) prebuilt       create_feature_field on the same [H, W, D] maps built before the timed calls
  (d) masks_random   (a) on per-pixel-random label maps (records spill past the four slots)
  kernel_ms          view 0 blended once (the pipelined driver's store), then Engine.scatter_mask_features with d = None timed
                     alone, Voronoi and per-pixel-random; the two kernels' own times come from a rocprofv3 --kernel-trace --stats
                     run of this tool (--quick)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gsbp_amd  # noqa: E402  (before the first HIP call: hardware queues)
import torch  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402


def _materialise(L, table):
    L = L.to(torch.int64)
    M = table.shape[0]
    ok = ((L >= 0) & (L < M))[..., None]
    return torch.where(ok, table.float()[L.clamp(0, M - 1)], torch.zeros((), device=table.device))


def _timed(fn):
    fn()  # untimed: allocations, the pipeline's engines
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--masks", type=int, default=200)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="one round, the kernel timing and (a) only (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    means, quats, scales, opac = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    vms, K = syn.make_cameras(cfg, n_views=a.views), syn.intrinsics(cfg)
    W, H, D = cfg.width, cfg.height, a.dim
    vor = [syn.make_mask_features(cfg, v, a.masks, D, device=dev) for v in range(a.views)]
    rnd = [syn.make_mask_features(cfg, v, a.masks, D, device=dev, per_pixel=True) for v in range(a.views)]
    args = (means, quats, scales, opac, vms, K, W, H)

    # the kernels alone on one blended view
    eng = gsbp_amd.Engine(cfg.n_gaussians, W, H, device=dev, tight_binning=True)
    eng.set_narrow_scatter(False)
    view = eng.view(vms[0], K, W, H)
    eng.project(view, means, quats, scales, opac)
    eng.bin_sort(view)
    eng.blend_weights(view)
    F = torch.zeros(cfg.n_gaussians, D, device=dev)
    kernel = {}
    for name, (L, tab) in (("voronoi", vor[0]), ("random", rnd[0])):
        eng.scatter_mask_features(view, L, tab, F, None)
        s0 = int(eng.mask_spilled.item())
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            eng.scatter_mask_features(view, L, tab, F, None)
        t1.record()
        torch.cuda.synchronize()
        kernel[name] = dict(ms=round(t0.elapsed_time(t1) / a.reps, 4),
                            spilled_records=(int(eng.mask_spilled.item()) - s0) // a.reps)
    st = eng.stats()
    kernel["n_isect"], kernel["n_headers"], kernel["n_pairs"] = st["n_isect"], st["n_headers"], st["n_pairs"]
    print(json.dumps({"kernel": kernel}), flush=True)
    del eng, F

    def masks(maps):
        return lambda: gsbp_amd.create_mask_feature_field(*args, maps.__getitem__, D)

    def materialise():
        return gsbp_amd.create_feature_field(*args, lambda v: _materialise(*vor[v]), D)

    variants = {"a_masks": masks(vor)}
    if not a.quick:
        variants["b_materialise"] = materialise
        variants["d_masks_random"] = masks(rnd)
    rounds = []
    for r in range(1 if a.quick else a.rounds):
        res = {}
        for name, fn in variants.items():
            res[name] = round(_timed(fn) / a.views, 3)
        if not a.quick:  # (c) needs the maps of every view at once: built for this variant only
            pre = [_materialise(*vor[v]) for v in range(a.views)]
            res["c_prebuilt"] = round(_timed(lambda: gsbp_amd.create_feature_field(*args, pre.__getitem__, D)) / a.views, 3)
            del pre
            torch.cuda.empty_cache()
        rounds.append(res)
        print(json.dumps({"round": r, "ms_per_view": res}), flush=True)
    out = dict(config=a.config, width=W, height=H, dim=D, masks=a.masks, views=a.views, device=torch.cuda.get_device_name(0),
               kernel_alone=kernel, ms_per_view_rounds=rounds)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
