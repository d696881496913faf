#!/usr/bin/env python3
"""The mask association at C2 geometry (1 M Gaussians, 1600 x 1060): per view the two integer kernels, the float label kernel on
the same map and store beside them, and the form a user had to write before the kernels existed.

    timeout -k 10 900 python tools/time_associate.py --out profiles/associate.json

Maps: the Voronoi cells of --masks random 2-D seeds, each cell one random id below --masks (synthetic.make_label_map), a new map
per view; --groups columns of votes.  The views run the real association (overlap, host match, votes, argmax), so every view's kernels see the groups the
views before it made.  Per view, each figure the mean of --reps launches between hip events, after one untimed launch, and the
three kernels alternate --rounds times (the last round is reported):
  overlap_ms        Engine.label_overlap into a [masks + 1, groups + 1] int64 table
  votes_ms          Engine.label_votes into the [N, groups] int64 votes (a scratch copy: the timed adds change no decision)
  scatter_labels_ms Engine.scatter_labels with d = None into an [N, masks] fp32 table: the same walk with float adds
  today_ms          what stands in for overlap without it: the [N, masks] fp32 table zeroed, scatter_labels, and
                    zeros(groups + 1, masks).index_add_(0, group + 1, table); today_peak_bytes is what the three hold at once
  host_match_ms     the table's copy to the host and match_masks (host clock around a synchronise)
The summary holds the medians over the views and the ratios overlap / scatter_labels and votes / scatter_labels.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gsbp_amd  # noqa: E402  (before the first HIP call: hardware queues)
import torch  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402
from gsbp_amd.associate import group_of_votes, match_masks  # noqa: E402


def _events(fn, reps):
    fn()
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
    ap.add_argument("--masks", type=int, default=200)
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_associate.py needs a GPU")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    n, K, G = cfg.n_gaussians, a.masks, a.groups
    g = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    vms, Kmat = syn.make_orbit(cfg, a.views), syn.intrinsics(cfg)
    eng = gsbp_amd.Engine(n, cfg.width, cfg.height, device=dev, tight_binning=True)
    votes = torch.zeros(n, G, dtype=torch.int64, device=dev)
    scratch = torch.zeros(n, G, dtype=torch.int64, device=dev)
    group = torch.full((n,), -1, dtype=torch.int32, device=dev)
    O = torch.zeros(K + 1, G + 1, dtype=torch.int64, device=dev)
    F = torch.zeros(n, K, device=dev)
    n_groups, rows = 0, []
    for v in range(a.views):
        L = syn.make_label_map(cfg, v, K, device=dev, n_seeds=K)
        view = eng.view(vms[v], Kmat, cfg.width, cfg.height)
        eng.project(view, *g)
        eng.bin_sort(view)
        eng.blend_weights(view)
        st = eng.stats()
        assert st["overflow"] == 0, st
        O.zero_()
        eng.label_overlap(view, L, group, O, K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        remap, n_groups, counts = match_masks(O.cpu().numpy(), n_groups, max_groups=G, return_counts=True)
        host_ms = (time.perf_counter() - t0) * 1e3
        remap_dev = torch.from_numpy(remap).to(dev)

        def today():
            F.zero_()
            eng.scatter_labels(view, L, F, None, K)
            return torch.zeros(G + 1, K, device=dev).index_add_(0, group.long() + 1, F)

        for _ in range(a.rounds):
            ov = _events(lambda: eng.label_overlap(view, L, group, O, K), a.reps)
            vo = _events(lambda: eng.label_votes(view, L, remap_dev, scratch, K), a.reps)
            sl = _events(lambda: eng.scatter_labels(view, L, F, None, K), a.reps)
            td = _events(today, a.reps)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev) - F.numel() * 4
        torch.cuda.reset_peak_memory_stats(dev)
        today()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - base
        eng.label_votes(view, L, remap_dev, votes, K)
        group = group_of_votes(votes)
        row = dict(view=v, n_pairs=st["n_pairs"], n_headers=st["n_headers"], overlap_ms=round(ov, 4), votes_ms=round(vo, 4),
                   scatter_labels_ms=round(sl, 4), today_ms=round(td, 4), today_peak_bytes=int(peak), host_match_ms=round(host_ms, 3),
                   n_groups=n_groups, grouped=int((group >= 0).sum()), **counts)
        print(json.dumps(row), flush=True)
        rows.append(row)

    def med(key):
        return statistics.median(r[key] for r in rows)

    summary = dict(overlap_ms=med("overlap_ms"), votes_ms=med("votes_ms"), scatter_labels_ms=med("scatter_labels_ms"),
                   today_ms=med("today_ms"), overlap_vs_scatter_labels=round(med("overlap_ms") / med("scatter_labels_ms"), 3),
                   votes_vs_scatter_labels=round(med("votes_ms") / med("scatter_labels_ms"), 3),
                   overlap_vs_today=round(med("overlap_ms") / med("today_ms"), 3),
                   table_bytes=(K + 1) * (G + 1) * 8, votes_bytes=n * G * 8, today_peak_bytes=max(r["today_peak_bytes"] for r in rows))
    print(json.dumps(summary), flush=True)
    cmd = (f"python tools/time_associate.py --config {a.config} --masks {K} --groups {G} --views {a.views} --reps {a.reps} "
           f"--rounds {a.rounds} --out profiles/associate.json")
    res = dict(tool="tools/time_associate.py", command=cmd, device=torch.cuda.get_device_name(0), masks=K, groups=G, views=a.views,
               reps=a.reps, rounds=a.rounds, date=time.strftime("%Y-%m-%d"), summary=summary, rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
