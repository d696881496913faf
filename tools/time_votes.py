#!/usr/bin/env python3
"""Per-view votes at C2 geometry (1 M Gaussians, 1600 x 1060): the binary vote against the label field on the same maps, and the
projection vote.

    timeout -k 10 900 python tools/time_votes.py --out profiles/votes.json

For every K in --classes and two maps -- "voronoi": the Voronoi cells of 200 random seeds, one random id per cell (a segmenter's
regions); "random": an independent random id per pixel (the worst case of the per-record reduction by word):
  vote_kernel_ms        view 0 projected, sorted and blended once (the vote pipeline's store: no half-tile lists, no d), then
                        Engine.vote_labels (bitset kernel + commit) timed alone with hip events, --reps times
  label_kernel_ms       Engine.scatter_labels with d = None on the same store, for comparison
  binary_ms_view        create_vote_field(method="binary") over --views views, hip events around the whole call after one
                        untimed call
  labels_ms_view        create_label_field over the same views and maps
  projection_ms_view    create_vote_field(method="projection") over the same views
  project_ms / vote_projected_ms   Engine.project and Engine.vote_projected of view 0 alone
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--classes", default="2,64,1000")
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
    view = eng.view(vms[0], K, cfg.width, cfg.height)
    eng.project(view, *g)
    eng.bin_sort(view)
    eng.blend_weights(view)
    st = eng.stats()
    assert st["overflow"] == 0, st
    proj = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    args = (*g, vms, K, cfg.width, cfg.height)
    rows = []
    for nc in [int(x) for x in a.classes.split(",")]:
        for kind in ("voronoi", "random"):
            L = syn.make_label_map(cfg, 0, nc, device=dev, per_pixel=kind == "random")
            C = torch.zeros(cfg.n_gaussians, nc, device=dev)
            n = torch.zeros(cfg.n_gaussians, device=dev)
            F = torch.zeros(cfg.n_gaussians, nc, device=dev)
            for _ in range(a.rounds):
                vk = _events(lambda: eng.vote_labels(view, L, C, n, nc), a.reps)
                lk = _events(lambda: eng.scatter_labels(view, L, F, None, nc), a.reps)
                gsbp_amd.create_vote_field(*args, lambda v: L, nc, method="binary")
                binary = _events(lambda: gsbp_amd.create_vote_field(*args, lambda v: L, nc, method="binary"), 1) / a.views
                gsbp_amd.create_label_field(*args, lambda v: L, nc)
                lab = _events(lambda: gsbp_amd.create_label_field(*args, lambda v: L, nc), 1) / a.views
                gsbp_amd.create_vote_field(*args, lambda v: L, nc, method="projection")
                pr = _events(lambda: gsbp_amd.create_vote_field(*args, lambda v: L, nc, method="projection"), 1) / a.views
                pk = _events(lambda: proj.project(view, *g), a.reps)
                vp = _events(lambda: proj.vote_projected(view, L, C, n, nc), a.reps)
            Cb, nb = gsbp_amd.create_vote_field(*args, lambda v: L, nc, method="binary")
            row = dict(config=a.config, classes=nc, map=kind, vote_kernel_ms=round(vk, 4), label_kernel_ms=round(lk, 4),
                       binary_ms_view=round(binary, 4), labels_ms_view=round(lab, 4),
                       binary_vs_labels=round(binary / lab, 3), projection_ms_view=round(pr, 4), project_ms=round(pk, 4),
                       vote_projected_ms=round(vp, 4), gaussians_voting=int((nb > 0).sum()),
                       max_votes=float(Cb.max()))
            print(json.dumps(row), flush=True)
            rows.append(row)
            del C, n, F, Cb, nb
            torch.cuda.empty_cache()
    cmd = (f"python tools/time_votes.py --config {a.config} --classes {a.classes} --views {a.views} --reps {a.reps} "
           f"--rounds {a.rounds} --out profiles/votes.json")
    res = dict(tool="tools/time_votes.py", command=cmd,
               device=torch.cuda.get_device_name(0), views=a.views, reps=a.reps, rounds=a.rounds,
               n_pairs_view0=st["n_pairs"], n_headers_view0=st["n_headers"], date=time.strftime("%Y-%m-%d"), rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
