#!/usr/bin/env python3
"""Integer label maps at C2 geometry (1 M Gaussians, 1600 x 1060): the label scatter kernel alone and the step per view of
create_label_field, against create_feature_field on the one-hot map of the same labels.

    timeout -k 10 1200 python tools/time_label_field.py --out profiles/label_field.json

For every K in --classes and two maps -- "voronoi": the Voronoi cells of 200 random seeds, one random id per cell (a segmenter's
regions); "random": an independent random id per pixel (the worst case of the per-record reduction by label):
  kernel_ms        view 0 projected, sorted and blended once (the store of the pipelined driver: half-tile lists, d added by the
                   blend), then Engine.scatter_labels with d = None timed alone with hip events, --reps times
  labels_ms_view   create_label_field over --views views (every view gets the same map object), hip events around the whole call
                   after one untimed call
  one_hot_ms_view  create_feature_field over the same views on one_hot(L, K).float(), built once before the timed calls
  one_hot_kernel_ms  the feature scatter of the one-hot map on the same blended view (Engine.scatter), for comparison
Every configuration runs --rounds times and reports the last round.
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


def _events(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def _one_hot(L, K):
    L = L.to(torch.int64)
    ok = (L >= 0) & (L < K)
    oh = torch.zeros(*L.shape, K, device=L.device)
    return oh.scatter_(-1, torch.where(ok, L, 0)[..., None], ok[..., None].float())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--classes", default="2,64,256,1000")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    g = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    vms, K = syn.make_cameras(cfg, n_views=a.views), syn.intrinsics(cfg)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, tight_binning=True)
    eng.set_narrow_scatter(False)
    view = eng.view(vms[0], K, cfg.width, cfg.height)
    eng.project(view, *g)
    eng.bin_sort(view)
    eng.blend_weights(view, d=torch.zeros(cfg.n_gaussians, device=dev))
    st = eng.stats()
    assert st["overflow"] == 0, st
    args = (*g, vms, K, cfg.width, cfg.height)
    rows = []
    for nc in [int(x) for x in a.classes.split(",")]:
        for kind in ("voronoi", "random"):
            L = syn.make_label_map(cfg, 0, nc, device=dev, per_pixel=kind == "random")
            oh = _one_hot(L, nc)
            F = torch.zeros(cfg.n_gaussians, nc, device=dev)
            Fo = torch.zeros(cfg.n_gaussians, nc, device=dev)
            for _ in range(a.rounds):
                kern = _events(lambda: eng.scatter_labels(view, L, F, None, nc), a.reps)
                kern_oh = _events(lambda: eng.scatter(view, oh, Fo, None), max(1, a.reps // 5))
                gsbp_amd.create_label_field(*args, lambda v: L, nc)
                lab = _events(lambda: gsbp_amd.create_label_field(*args, lambda v: L, nc), 1) / a.views
                gsbp_amd.create_feature_field(*args, lambda v: oh, nc)
                one = _events(lambda: gsbp_amd.create_feature_field(*args, lambda v: oh, nc), 1) / a.views
            P = gsbp_amd.create_label_field(*args, lambda v: L, nc)
            _, Fl, dl, _ = gsbp_amd.create_label_field(*args, lambda v: L, nc, return_partials=True)
            _, Ff, df, _ = gsbp_amd.create_feature_field(*args, lambda v: oh, nc, return_partials=True)
            scale = float(Ff.norm(dim=1).max())
            err = float((Fl - Ff).norm(dim=1).max()) / max(scale, 1e-30)
            distinct = float((L[:, 1:] != L[:, :-1]).float().mean())
            row = dict(config=a.config, classes=nc, map=kind, kernel_ms=round(kern, 4), one_hot_kernel_ms=round(kern_oh, 4),
                       labels_ms_view=round(lab, 4), one_hot_ms_view=round(one, 4),
                       speedup_vs_one_hot=round(one / lab, 2), max_row_err_vs_one_hot=err,
                       label_changes_per_pixel_step=round(distinct, 4), rows_sum_max=float(P.sum(dim=1).max()))
            print(json.dumps(row), flush=True)
            rows.append(row)
            del oh, F, Fo, Ff, Fl, P
            torch.cuda.empty_cache()
    res = dict(tool="tools/time_label_field.py", device=torch.cuda.get_device_name(0), views=a.views, reps=a.reps,
               rounds=a.rounds, n_pairs_view0=st["n_pairs"], n_headers_view0=st["n_headers"],
               weight_store_bytes_view0=8 * st["n_pairs"], date=time.strftime("%Y-%m-%d"), rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
