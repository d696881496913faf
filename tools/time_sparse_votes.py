#!/usr/bin/env python3
"""The votes into per-Gaussian slot lists against the dense votes, at tools/time_associate.py's case: C2 geometry (1 M Gaussians,
1600 x 1060), per view the Voronoi cells of --masks random seeds with one random id each, --groups groups, medians over --views
views.

    timeout -k 10 900 python tools/time_sparse_votes.py --out profiles/sparse_votes.json

Kernels.  The views run the real dense association, so every view's kernels see the remap the views before it made.  Per view,
on the same view, map, remap and weight store, three forms alternate --rounds times (the last round is reported), each figure the
mean of --reps launches, every launch between its own pair of hip events after one untimed launch:
  dense_ms   Engine.label_votes into an [N, groups] int64 scratch table
  cold_ms    Engine.label_votes_sparse at --slots slots into EMPTY lists (reset before every launch, outside the events): every
             first add of a key inserts
  warm_ms    the same call into lists this view has already been voted into: every key is found
Whole association.  associate_masks over the same views and maps on one shared Engine, host clock around a synchronise, per
view: votes="dense" and votes="sparse" alternating --rounds times (the last round is reported), then ONE sparse-only case with
--big-masks ids per view and --big-groups groups, where the dense table would take 8 * N * big_groups bytes.  peak_bytes is
torch's peak of allocated memory above what was allocated before the call (the Engine's workspace is not in it).
The derived figure, not a measurement: the lists take N * (12 * slots + 8) bytes.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gsbp_amd  # noqa: E402  (before the first HIP call: hardware queues)
import torch  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402
from gsbp_amd.associate import associate_masks, group_of_votes, match_masks  # noqa: E402
from gsbp_amd.sparse_votes import (new_sparse_votes, sparse_votes_bytes, sparse_votes_dense, sparse_votes_groups,  # noqa: E402
                                   sparse_votes_stats)


def _events(fn, reps, before=None):
    """Mean ms of fn() over reps launches, each between its own events; before() runs ahead of every launch, outside them."""
    if before:
        before()
    fn()
    pairs = []
    for _ in range(reps):
        if before:
            before()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        pairs.append((t0, t1))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs) / reps


def _whole(dev, views, run):
    """(ms per view, peak bytes above the start, result) of one associate_masks call."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (the overflow warning: its count is in the result)
        out = run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / views, int(torch.cuda.max_memory_allocated(dev) - base), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--masks", type=int, default=200)
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--big-masks", type=int, default=1000)
    ap.add_argument("--big-groups", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_sparse_votes.py needs a GPU")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    n, K, G, S = cfg.n_gaussians, a.masks, a.groups, a.slots
    g = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    vms, Kmat = syn.make_orbit(cfg, a.views), syn.intrinsics(cfg)
    eng = gsbp_amd.Engine(n, cfg.width, cfg.height, device=dev, tight_binning=True)
    maps = [syn.make_label_map(cfg, v, K, device=dev, n_seeds=K) for v in range(a.views)]

    # ---- the kernels, view by view inside the real dense association
    votes = torch.zeros(n, G, dtype=torch.int64, device=dev)
    scratch = torch.zeros(n, G, dtype=torch.int64, device=dev)
    group = torch.full((n,), -1, dtype=torch.int32, device=dev)
    O = torch.zeros(K + 1, G + 1, dtype=torch.int64, device=dev)
    cold, warm = new_sparse_votes(n, S, device=dev), new_sparse_votes(n, S, device=dev)
    n_groups, rows = 0, []

    def reset():
        cold.keys.fill_(-1)
        cold.vals.zero_()
        cold.spill.zero_()

    for v in range(a.views):
        L = maps[v]
        view = eng.view(vms[v], Kmat, cfg.width, cfg.height)
        eng.project(view, *g)
        eng.bin_sort(view)
        eng.blend_weights(view)
        st = eng.stats()
        assert st["overflow"] == 0, st
        O.zero_()
        eng.label_overlap(view, L, group, O, K)
        remap, n_groups, _ = match_masks(O.cpu().numpy(), n_groups, max_groups=G, return_counts=True)
        remap_dev = torch.from_numpy(remap).to(dev)
        warm.keys.fill_(-1)
        warm.vals.zero_()
        warm.spill.zero_()
        eng.label_votes_sparse(view, L, remap_dev, warm, K)  # from here on every key of this view is found
        for _ in range(a.rounds):
            de = _events(lambda: eng.label_votes(view, L, remap_dev, scratch, K), a.reps)
            co = _events(lambda: eng.label_votes_sparse(view, L, remap_dev, cold, K), a.reps, before=reset)
            wa = _events(lambda: eng.label_votes_sparse(view, L, remap_dev, warm, K), a.reps)
        # the same integers at the size timed: one vote into empty lists against one vote into a zeroed table
        reset()
        eng.label_votes_sparse(view, L, remap_dev, cold, K)
        scratch.zero_()
        eng.label_votes(view, L, remap_dev, scratch, K)
        exact = cold.spill == 0
        same = bool(torch.equal(sparse_votes_dense(cold, G)[exact], scratch[exact])) and bool(
            torch.equal(cold.vals.sum(dim=1) + cold.spill, scratch.sum(dim=1)))
        eng.label_votes(view, L, remap_dev, votes, K)
        group = group_of_votes(votes)
        row = dict(view=v, n_pairs=st["n_pairs"], n_headers=st["n_headers"], dense_ms=round(de, 4), cold_ms=round(co, 4),
                   warm_ms=round(wa, 4), n_groups=n_groups, one_view_overflow_rows=int((~exact).sum()), equals_dense=same)
        print(json.dumps(row), flush=True)
        rows.append(row)
    del votes, scratch, cold, warm, O
    torch.cuda.empty_cache()

    # ---- the whole association per view, dense against sparse, then the case no dense table can hold
    gv, vd, Kd = g, vms.to(dev), Kmat.to(dev)

    def run(mode, masks, max_groups, mask_fn):
        return lambda: associate_masks(*gv, vd, Kd, cfg.width, cfg.height, mask_fn, masks, max_groups=max_groups, engine=eng,
                                       votes=mode, slots=S)

    for _ in range(a.rounds):
        d_ms, d_peak, dense = _whole(dev, a.views, run("dense", K, G, lambda v: maps[v]))
        dense_groups, dense_n = dense.groups, dense.n_groups
        del dense
        torch.cuda.empty_cache()
        s_ms, s_peak, sparse = _whole(dev, a.views, run("sparse", K, G, lambda v: maps[v]))
    s_stats = sparse_votes_stats(sparse.votes)
    certain = sparse_votes_groups(sparse.votes)[1]
    whole = dict(dense_ms_per_view=round(d_ms, 3), sparse_ms_per_view=round(s_ms, 3), dense_peak_bytes=d_peak, sparse_peak_bytes=s_peak,
                 n_groups_dense=dense_n, n_groups_sparse=sparse.n_groups, sparse_stats=s_stats,
                 groups_equal_on_certain_rows=bool(torch.equal(sparse.groups[certain], dense_groups[certain])),
                 groups_equal_everywhere=bool(torch.equal(sparse.groups, dense_groups)))
    print(json.dumps(whole), flush=True)
    del sparse, dense_groups
    torch.cuda.empty_cache()
    big_maps = [syn.make_label_map(cfg, v, a.big_masks, device=dev, n_seeds=a.big_masks) for v in range(a.views)]
    b_ms, b_peak, big_run = _whole(dev, a.views, run("sparse", a.big_masks, a.big_groups, lambda v: big_maps[v]))
    big = dict(masks=a.big_masks, max_groups=a.big_groups, ms_per_view=round(b_ms, 3), peak_bytes=b_peak, n_groups=big_run.n_groups,
               dense_votes_would_take_bytes=8 * n * a.big_groups, sparse_stats=sparse_votes_stats(big_run.votes))
    print(json.dumps(big), flush=True)

    def med(key):
        return statistics.median(r[key] for r in rows)

    summary = dict(dense_ms=med("dense_ms"), cold_ms=med("cold_ms"), warm_ms=med("warm_ms"),
                   cold_vs_dense=round(med("cold_ms") / med("dense_ms"), 3), warm_vs_dense=round(med("warm_ms") / med("dense_ms"), 3),
                   whole_sparse_vs_dense=round(s_ms / d_ms, 3), lists_bytes_derived=sparse_votes_bytes(n, S),
                   dense_votes_bytes=8 * n * G, equals_dense=all(r["equals_dense"] for r in rows))
    print(json.dumps(summary), flush=True)
    cmd = (f"python tools/time_sparse_votes.py --config {a.config} --masks {K} --groups {G} --slots {S} --views {a.views} "
           f"--reps {a.reps} --rounds {a.rounds} --big-masks {a.big_masks} --big-groups {a.big_groups} --out profiles/sparse_votes.json")
    res = dict(tool="tools/time_sparse_votes.py", command=cmd, device=torch.cuda.get_device_name(0), n=n, masks=K, groups=G, slots=S,
               views=a.views, reps=a.reps, rounds=a.rounds, date=time.strftime("%Y-%m-%d"), summary=summary, whole=whole, big=big,
               rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
