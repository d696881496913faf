#!/usr/bin/env python3
"""Times the radius components (csrc/components.hip) and writes profiles/components.json.

    python tools/time_components.py [--sizes 100000,1000000] [--repeats 5] [--out profiles/components.json]

N points on (a) the C2 synthetic scene's means (uniform) and (b) spatial.clustered_points (64 Gaussian clusters with sigma over two
decades plus 0.1 % far floaters), at min_points 1 and 8, the radius from suggest_radius (2 x the median distance to the 8th
neighbour).  Build (cell keys + sort + build kernel), count, union, attach and flatten are timed separately with device events, each
once per round, median over the rounds; beside them the whole radius_components call (with the dense numbering), the candidates a
point's lane computed a distance to and the neighbours it found, and the grid's statistics -- cells that hold thousands of points make
the walk quadratic in their occupancy, as they do for spatial_knn.  Against: sklearn's DBSCAN on a host copy (how the reference
searches neighbours), skipped where its neighbourhood lists would not fit (more than --sklearn-pairs neighbour pairs: it stores
them all), and one spatial_knn(k = 8) on the same points as a scale.  The file is rewritten after every case.
"""
import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gsbp_amd  # noqa: E402
from gsbp_amd import components as comp, spatial, synthetic as syn  # noqa: E402
from gsbp_amd._lib import ptr  # noqa: E402
from gsbp_amd._views import run  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def med(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def stages(p, grid, r2, min_points, times=None):
    """One radius_components by hand, stage by stage; times: a dict of lists that takes each stage's milliseconds."""
    n, dev = p.shape[0], p.device

    def stage(name, fn):
        ms, out = timed(fn)
        if times is not None:
            times.setdefault(name, []).append(ms)
        return out

    built = stage("build", lambda: comp._build(p, grid))
    pts, cell_start, perm = built
    count = stage("count", lambda: comp._count(built, grid, None, r2, p, perm, None, min_points))
    parent = torch.arange(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    walk = comp._walk_args(n, pts, cell_start, grid, None, r2)
    stage("union", lambda: run("gwbp_radius_union", dev, *walk, ptr(count), min_points, ptr(parent), ptr(status)))
    attach = None
    if min_points > 1:
        attach = torch.empty(n, dtype=torch.int32, device=dev)
        stage("attach", lambda: run("gwbp_radius_attach", dev, *walk, ptr(count), min_points, ptr(attach)))
    root = torch.empty(n, dtype=torch.int32, device=dev)
    stage("flatten", lambda: run("gwbp_components_flatten", dev, C.c_int64(n), ptr(count), min_points, ptr(attach), ptr(parent),
                                 ptr(root), ptr(status)))
    assert int(status) == 0
    return built, root


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn-pairs", type=float, default=3e8, help="skip sklearn above this many neighbour pairs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_components.py needs a GPU")
    dev = torch.device("cuda")
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        DBSCAN = None
    c2 = syn.make_scene(syn.CONFIGS["C2"])["means"].float()
    res = {"tool": "tools/time_components.py", "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "repeats": args.repeats, "timing": "device events; every stage once per round, median over rounds; sklearn: wall clock, once",
           "cases": []}
    for n in (int(s) for s in args.sizes.split(",")):
        n = min(n, int(c2.shape[0]))
        for name, host in (("uniform_C2", c2[:n]), ("clustered", spatial.clustered_points(n))):
            p = host.to(dev)
            radius = gsbp_amd.suggest_radius(p)
            r2 = comp._r2(radius)
            grid = comp._plan(p, radius, None, None)
            knn = [timed(lambda: gsbp_amd.spatial_knn(p, 8))[0] for _ in range(args.repeats + 1)][1:]
            for min_points in (1, 8):
                case = {"set": name, "n": n, "radius": radius, "min_points": min_points}
                built, root = stages(p, grid, r2, min_points)  # warm-up
                case["grid"] = spatial.grid_stats(grid, built[1])
                visited = torch.empty(n, dtype=torch.int32, device=dev)
                full = comp._count(built, grid, None, r2, p, built[2], None, comp.INT32_MAX, visited)
                case["neighbours_per_point"] = round(float(full.double().mean()), 2)
                case["candidates_visited_per_point"] = round(float(visited.double().mean()), 2)
                times, whole = {}, []
                for _ in range(args.repeats):
                    stages(p, grid, r2, min_points, times)
                    whole.append(timed(lambda: gsbp_amd.radius_components(p, radius, min_points))[0])
                ours = gsbp_amd.radius_components(p, radius, min_points)
                case.update({k: med(v) for k, v in times.items()})
                case["radius_components_call"] = med(whole)
                case["components"], case["noise"] = int(ours.sizes.numel()), int((ours.labels < 0).sum())
                case["spatial_knn_k8_same_points"] = med(knn)
                pairs = float(full.double().sum())
                if DBSCAN is None:
                    case["sklearn_dbscan"] = "sklearn does not import"
                elif pairs > args.sklearn_pairs:
                    case["sklearn_dbscan"] = f"skipped: {pairs:.3g} neighbour pairs (it stores them all)"
                else:
                    x = host.numpy().astype("float64")
                    t0 = time.perf_counter()
                    sk = DBSCAN(eps=radius, min_samples=min_points).fit(x)
                    case["sklearn_dbscan"] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 1),
                                              "components": int(sk.labels_.max()) + 1, "noise": int((sk.labels_ < 0).sum())}
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
