#!/usr/bin/env python3
"""Times the regions (csrc/regions.hip) and writes profiles/regions.json.

    python tools/time_regions.py [--sizes 100000,1000000] [--dims 512,1024] [--ks 8,16] [--repeats 5] [--out profiles/regions.json]

The first N means of the C2 synthetic scene with regions.synthetic_regions features of width D, the neighbour list of
spatial_knn(means, k + 1) (itself is one of them: k + 1 columns).  Timed separately with device events, each once per round after a
warm-up round, median over the rounds: the similarity kernel, the union and the flatten; gwbp_neighbor_mean on the same list and
field (it gathers (k + 1) N rows and writes N, where the similarity kernel gathers (k + 1) N and reads N); the literal torch form
Fn = F.normalize(f); (Fn[:, None] * Fn[idx]).sum(-1) in row chunks that fit, with its peak memory; and radius_components' union on
the same means at suggest_radius, for scale.  Beside them two HBM times at the 6.29 TB/s a float4 copy reaches on this chip:
"fetch per use", (k + 2) N rows of 4 D bytes -- every listed row fetched from HBM each time it is used, no cache counted, which a
kernel can beat when lists share rows -- and the floor proper, the N distinct rows read once.  The similarity and neighbor_mean
figures are of the Python wrappers: they include the allocation of the outputs (the caching allocator's, after the warm-up round).
The expectation the figures are reported against: the
similarity kernel takes at most 1.25 x gwbp_neighbor_mean on the same inputs.  The file is rewritten after every case.
"""
import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gsbp_amd  # noqa: E402
from gsbp_amd import components as comp, regions, spatial, synthetic as syn  # noqa: E402
from gsbp_amd._lib import ptr  # noqa: E402
from gsbp_amd._views import run  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # a float4 copy on the MI355X, measured
TORCH_CHUNK_BYTES = 2 << 30


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def med(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def stages(f, idx, sim_min, times=None):
    """One similarity_components by hand, stage by stage; times: a dict of lists that takes each stage's milliseconds."""
    n, k = idx.shape
    dev = f.device

    def stage(name, fn):
        ms, out = timed(fn)
        if times is not None:
            times.setdefault(name, []).append(ms)
        return out

    sim, live = stage("similarity", lambda: regions._similarity(f, idx))
    parent = torch.arange(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    root = torch.empty(n, dtype=torch.int32, device=dev)
    stage("union", lambda: run("gwbp_edge_union", dev, C.c_int64(n), k, ptr(idx), ptr(sim), ptr(live), None, None, C.c_float(sim_min),
                               C.c_float(float("inf")), ptr(count), ptr(parent), ptr(status)))
    stage("flatten", lambda: run("gwbp_components_flatten", dev, C.c_int64(n), ptr(count), 1, None, ptr(parent), ptr(root), ptr(status)))
    stage("neighbor_mean", lambda: spatial.neighbor_mean(f, idx))
    assert int(status) == 0
    return sim, root


def torch_form(f, idx):
    """(sim [N, k], peak bytes): the literal form in row chunks of about TORCH_CHUNK_BYTES of gathered rows."""
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn = torch.nn.functional.normalize(f)
    n, k = idx.shape
    rows = max(1, TORCH_CHUNK_BYTES // (k * f.shape[1] * 4))
    out = torch.empty(n, k, dtype=torch.float32, device=f.device)
    for a in range(0, n, rows):
        out[a:a + rows] = (fn[a:a + rows, None] * fn[idx[a:a + rows].long().clamp(min=0)]).sum(-1)
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--dims", default="512,1024")
    ap.add_argument("--ks", default="8,16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sim-min", type=float, default=regions.DEFAULT_SIM_MIN)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_regions.py needs a GPU")
    dev = torch.device("cuda")
    c2 = syn.make_scene(syn.CONFIGS["C2"])["means"].float()
    res = {"tool": "tools/time_regions.py", "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "repeats": args.repeats, "timing": "device events; every stage once per round after a warm-up round, median over rounds; similarity and neighbor_mean "
                     "are timed through their Python wrappers and include the allocation of their outputs (caching allocator)",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "expectation": "similarity <= 1.25 x neighbor_mean on the same inputs", "cases": []}
    for n in (int(s) for s in args.sizes.split(",")):
        n = min(n, int(c2.shape[0]))
        host = c2[:n]
        p = host.to(dev)
        radius = gsbp_amd.suggest_radius(p)
        grid = comp._plan(p, radius, None, None)
        r2 = comp._r2(radius)
        built = comp._build(p, grid)
        count = comp._count(built, grid, None, r2, p, built[2], None, 1)
        walk = comp._walk_args(n, built[0], built[1], grid, None, r2)
        runion = []
        for _ in range(args.repeats + 1):
            parent = torch.arange(n, dtype=torch.int32, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            runion.append(timed(lambda: run("gwbp_radius_union", dev, *walk, ptr(count), 1, ptr(parent), ptr(status)))[0])
        for d in (int(s) for s in args.dims.split(",")):
            f = regions.synthetic_regions(host, d=d)[0].to(dev)
            for k in (int(s) for s in args.ks.split(",")):
                idx = gsbp_amd.spatial_knn(p, k + 1)[1]
                case = {"n": n, "D": d, "k": k, "columns": k + 1, "sim_min": args.sim_min}
                sim, root = stages(f, idx, args.sim_min)  # warm-up
                times = {}
                for _ in range(args.repeats):
                    stages(f, idx, args.sim_min, times)
                case.update({name: med(v) for name, v in times.items()})
                per_use_ms = (k + 2) * n * 4 * d / HBM_BYTES_PER_S * 1e3
                case["hbm_ms_fetch_per_use"] = round(per_use_ms, 3)  # (k + 2) N rows: not a floor, rows that lists share may hit a cache
                case["hbm_ms_distinct_rows_floor"] = round(n * 4 * d / HBM_BYTES_PER_S * 1e3, 3)
                case["similarity_over_fetch_per_use"] = round(case["similarity"]["median_ms"] / per_use_ms, 3)
                case["similarity_over_neighbor_mean"] = round(case["similarity"]["median_ms"] / case["neighbor_mean"]["median_ms"], 3)
                case["regions"] = int(torch.unique(root[root >= 0]).numel())
                case["radius_union_same_means"] = dict(med(runion[1:]), radius=radius)
                torch_form(f[:4096], idx[:4096].clamp(max=4095))  # warm-up
                ms, (lit, peak) = timed(lambda: torch_form(f, idx))
                ok = ~torch.isnan(sim)
                case["torch_form"] = {"ms": round(ms, 3), "peak_bytes": int(peak),
                                      "max_abs_difference": float((lit[ok] - sim[ok]).abs().max()) if bool(ok.any()) else 0.0}
                del lit
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as fh:
                    json.dump(res, fh, indent=1)
            del f
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
