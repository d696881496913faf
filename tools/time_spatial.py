#!/usr/bin/env python3
"""Times the spatial k-NN search (csrc/spatial.hip) and what is built on it, and writes profiles/spatial.json.

    python tools/time_spatial.py [--n 1000000] [--repeats 20] [--out profiles/spatial.json]

N points at k = 4, 8, 16 on (a) the C2 synthetic scene's means (uniform) and (b) spatial.clustered_points: 64 Gaussian clusters with
sigma over two decades plus 0.1 % far floaters.  Build (cell keys + sort + build kernel) and search are timed separately with device
events; every form takes its turn in each of the `repeats` rounds of one run, and the median is reported with the grid's statistics
beside it.  Against: chunked torch.cdist + topk on the GPU at --torch-n points (its cost is quadratic: the time is reported as
measured at that size and, marked as such, scaled by (N / torch_n)^2); sklearn's NearestNeighbors on the host if it imports;
smooth_labels; smooth_features at D = 512 against features[idx].mean(1) with both peak memories.
"""
import argparse
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
from gsbp_amd import spatial, synthetic as syn  # noqa: E402
from gsbp_amd.spatial import _grid_args, _sorted_keys  # noqa: E402
from gsbp_amd._lib import ptr  # noqa: E402
from gsbp_amd._views import ld, run  # noqa: E402
import ctypes as C  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def build(p, grid):
    skeys, perm = _sorted_keys(p, grid)
    pts = torch.empty(p.shape[0], 4, dtype=torch.float32, device=p.device)
    cell_start = torch.empty(grid.cells + 1, dtype=torch.int32, device=p.device)
    run("gwbp_spatial_build", p.device, C.c_int64(p.shape[0]), ptr(p), C.c_int64(ld(p)), ptr(skeys), ptr(perm), C.c_int64(grid.cells),
        ptr(pts), ptr(cell_start))
    return pts, cell_start, perm


def search(p, grid, built, k):
    pts, cell_start, perm = built
    n = p.shape[0]
    idx = torch.empty(n, k, dtype=torch.int32, device=p.device)
    dist = torch.empty(n, k, dtype=torch.float32, device=p.device)
    run("gwbp_spatial_knn", p.device, C.c_int64(n), ptr(pts), ptr(cell_start), *_grid_args(grid), C.c_int64(n), ptr(p), C.c_int64(ld(p)),
        ptr(perm), k, ptr(idx), ptr(dist))
    return dist, idx


def torch_knn(p, k, chunk=4096):
    d, i = [], []
    for s in range(0, p.shape[0], chunk):
        dd, ii = torch.cdist(p[s:s + chunk], p).topk(k, dim=1, largest=False)
        d.append(dd)
        i.append(ii)
    return torch.cat(d), torch.cat(i)


def med(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--torch-n", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_spatial.py needs a GPU")
    dev = torch.device("cuda")
    ks = (4, 8, 16)
    uniform = syn.make_scene(syn.CONFIGS["C2"])["means"].float()[:args.n]
    n = int(uniform.shape[0])  # (the C2 scene has 1 M Gaussians: a larger --n is cut to that, for every set alike)
    sets = {"uniform_C2": uniform.to(dev), "clustered": spatial.clustered_points(n).to(dev)}
    res = {"tool": "tools/time_spatial.py", "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "n": int(uniform.shape[0]), "repeats": args.repeats, "timing": "device events; every form once per round, median over rounds",
           "sets": {}}

    state = {}
    for name, p in sets.items():
        grid = spatial.plan_grid(p)
        built = build(p, grid)
        stats = spatial.grid_stats(grid, built[1])
        for k in ks:
            search(p, grid, built, k)  # warm-up of every shape
        torch.cuda.synchronize()
        state[name] = (p, grid, built)
        res["sets"][name] = {"grid": stats, "build": [], **{f"search_k{k}": [] for k in ks}}
        print(name, json.dumps(stats), flush=True)
    for _ in range(args.repeats):
        for name, (p, grid, built) in state.items():
            res["sets"][name]["build"].append(timed(lambda: build(p, grid))[0])
            for k in ks:
                res["sets"][name][f"search_k{k}"].append(timed(lambda: search(p, grid, built, k))[0])
    for name in state:
        for key in ["build"] + [f"search_k{k}" for k in ks]:
            res["sets"][name][key] = med(res["sets"][name][key])
        print(name, json.dumps({key: v["median_ms"] for key, v in res["sets"][name].items() if key != "grid"}), flush=True)

    # the build when a caller's small cell_size gives the largest grid there is (2^24 cells: one binary search per cell), and the
    # automatic cell size against 2 and 8 points per cell (k = 8, uniform set)
    p = state["uniform_C2"][0]
    ext = float((p.max(dim=0).values - p.min(dim=0).values).max())
    big = spatial.plan_grid(p, cell_size=ext / 250.0)
    build(p, big)
    res["build_max_cells"] = {"cells": big.cells, "dims": list(big.dims), **med([timed(lambda: build(p, big))[0] for _ in range(args.repeats)])}
    print("build_max_cells", json.dumps(res["build_max_cells"]), flush=True)
    res["points_per_cell_k8"] = {}
    variants = {ppc: spatial.plan_grid(p, points_per_cell=ppc) for ppc in (1.0, 2.0, 4.0, 8.0, 16.0)}
    built_v = {ppc: build(p, g) for ppc, g in variants.items()}
    times_v = {ppc: [] for ppc in variants}
    for ppc in variants:
        search(p, variants[ppc], built_v[ppc], 8)
    for _ in range(args.repeats):
        for ppc in variants:
            times_v[ppc].append(timed(lambda: search(p, variants[ppc], built_v[ppc], 8))[0])
    for ppc in variants:
        res["points_per_cell_k8"][str(ppc)] = {"cells": variants[ppc].cells, **med(times_v[ppc])}
    print("points_per_cell_k8", json.dumps(res["points_per_cell_k8"]), flush=True)
    del built_v

    # the torch form on the GPU, at a size its quadratic cost allows
    tn = min(args.torch_n, n)
    res["torch_cdist_topk"] = {"n": tn, "chunk": 4096, "k": 8}
    for name, (p, grid, built) in state.items():
        sub = p[:: max(n // tn, 1)][:tn].contiguous()
        torch_knn(sub, 8)
        ts = [timed(lambda: torch_knn(sub, 8))[0] for _ in range(3)]
        d_ref, i_ref = torch_knn(sub, 8)
        ours = [timed(lambda: gsbp_amd.spatial_knn(sub, 8))[0] for _ in range(5)]
        d, i = gsbp_amd.spatial_knn(sub, 8)
        res["torch_cdist_topk"][name] = {**med(ts), "scaled_to_n_ms": round(statistics.median(ts) * (n / tn) ** 2, 1),
                                         "scaled": f"measured at n = {tn}, multiplied by (N / n)^2 = {(n / tn) ** 2:g}: NOT measured at N",
                                         "spatial_knn_same_points_ms": med(ours)["median_ms"],
                                         "kth_distance_max_rel_diff": float(((d[:, -1] - d_ref[:, -1]).abs() / d_ref[:, -1].clamp(min=1e-30)).max())}
        print("torch", name, json.dumps(res["torch_cdist_topk"][name]), flush=True)

    try:
        from sklearn.neighbors import NearestNeighbors
        host = sets["uniform_C2"].cpu().numpy()
        t0 = time.perf_counter()
        NearestNeighbors(n_neighbors=4, metric="euclidean").fit(host).kneighbors(host)
        res["sklearn_host_k4"] = {"n": n, "seconds": round(time.perf_counter() - t0, 3)}
    except ImportError:
        res["sklearn_host_k4"] = "sklearn is not installed on the measuring machine: not measured"

    # what is built on the search: the label vote, and the neighbour mean at D = 512 against the torch form
    p, grid, built = state["uniform_C2"]
    _, idx = search(p, grid, built, 8)
    labels = torch.randint(0, 16, (n,), generator=torch.Generator().manual_seed(0)).to(dev)
    gsbp_amd.smooth_labels(p, labels, 16, neighbors=idx)
    feats = torch.randn(n, 512, generator=torch.Generator().manual_seed(1)).to(dev)
    forms = {"smooth_labels_k8": lambda: gsbp_amd.smooth_labels(p, labels, 16, neighbors=idx),
             "smooth_features_D512_k8": lambda: gsbp_amd.smooth_features(p, feats, neighbors=idx),
             "torch_gather_mean_D512_k8": lambda: feats[idx.long()].mean(1)}
    times, peaks = {key: [] for key in forms}, {}
    for key, fn in forms.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peaks[key] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        del out
    for _ in range(args.repeats):
        for key, fn in forms.items():
            times[key].append(timed(fn)[0])
    a, b = forms["smooth_features_D512_k8"](), forms["torch_gather_mean_D512_k8"]()
    res["on_top"] = {key: {**med(times[key]), "peak_mib": peaks[key]} for key in forms}
    res["on_top"]["smooth_features_max_abs_diff_to_torch"] = float((a - b).abs().max())
    # the mean's floor: k rows of D floats read (mostly from cache: neighbours share rows) and one written, at 8 TB/s HBM -- stated,
    # not claimed
    res["on_top"]["smooth_features_bytes_moved_if_nothing_cached"] = n * 512 * 4 * (8 + 1)
    print(json.dumps(res["on_top"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
