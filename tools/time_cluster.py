#!/usr/bin/env python3
"""The two passes of a k-means step on a full-size field, beside what they replace: kmeans_assign against knn_search(k = 1) (the same
score tile with a top-k list) and against the torch form -- (X[i:i+c] @ C.T).argmax(1) in chunks -- and cluster_sums against
index_add_ (float atomics: not reproducible) and against its floor, one read of the field.  Also one whole Lloyd step (assign,
stable sort, sums, centroid update).

    timeout -k 10 1100 python tools/time_cluster.py --out profiles/cluster.json

Every form is warmed up once; then the forms of a group run alternately, --repeats rounds, each call between two hip events; the
median (and min) over the rounds is reported.  peak_mib is the torch.cuda.max_memory_allocated delta of one call (outputs and
workspace included).  Floors: the assignment's is its 2 N K D FLOP over the fp32 matrix pipe's 157.3 TF peak; the sums' is one read
of the field at the measured 6.29 TB/s copy rate.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gsbp_amd  # noqa: E402
import torch  # noqa: E402
from gsbp_amd import cluster  # noqa: E402

PEAK = 157.3e12
HBM = 6.29e12
CHUNK = 65536  # rows per matmul of the torch assignment: a [CHUNK, K] score block


def peak_of(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def timed_group(forms, repeats):
    """forms: {name: fn}.  Warm-up and peak per form, then `repeats` rounds that run every form once, in turn."""
    out = {name: dict(peak_mib=peak_of(fn)) for name, fn in forms.items()}
    ts = {name: [] for name in forms}
    for _ in range(repeats):
        for name, fn in forms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ts[name].append(t0.elapsed_time(t1))
    for name in forms:
        out[name].update(median_ms=round(statistics.median(ts[name]), 3), min_ms=round(min(ts[name]), 3),
                         max_ms=round(max(ts[name]), 3))
    return out


def torch_assign(X, Ct):
    lab = torch.empty(X.shape[0], dtype=torch.int64, device=X.device)
    for i in range(0, X.shape[0], CHUNK):
        lab[i:i + CHUNK] = (X[i:i + CHUNK] @ Ct).argmax(dim=1)
    return lab


def torch_sums(X, lab, k):
    return torch.zeros(k, X.shape[1], device=X.device).index_add_(0, lab, X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="512,1024")
    ap.add_argument("--ks", default="64,256,1024")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(tool="tools/time_cluster.py", device=torch.cuda.get_device_name(0), repeats=a.repeats, date=time.strftime("%Y-%m-%d"),
               peak_fp32_matrix_flops=PEAK, hbm_copy_bytes_per_s=HBM, torch_chunk_rows=CHUNK, rows=[])
    n = a.n
    for D in [int(x) for x in a.dims.split(",")]:
        X = torch.randn(n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(D))
        X /= X.norm(dim=1, keepdim=True)
        for k in [int(x) for x in a.ks.split(",")]:
            c = cluster._unit(X[torch.randperm(n, generator=torch.Generator().manual_seed(k))[:k].to(dev)])
            ct = c.t().contiguous()
            bias = cluster.centroid_bias(c, "euclidean")
            assign = timed_group({
                "kmeans_assign": lambda: cluster._assign(X, c, None),
                "kmeans_assign_bias": lambda: cluster._assign(X, c, bias),
                "knn_search_k1": lambda: gsbp_amd.knn_search(X, c, 1),
                "torch_chunked_matmul_argmax": lambda: torch_assign(X, ct),
            }, a.repeats)
            lab32, _ = cluster._assign(X, c, None)
            lab64 = lab32.long()
            agree = float((torch_assign(X, ct) == lab64).double().mean())
            sums = timed_group({
                "stable_sort_of_labels": lambda: torch.sort(lab32, stable=True),
                "cluster_sums_with_its_sort": lambda: cluster._sums(X, lab32, k, None),
                "torch_index_add": lambda: torch_sums(X, lab64, k),
                "field_read_torch_sum": lambda: X.sum(),
            }, a.repeats)

            def step():
                labels, best = cluster._assign(X, c, None)
                s, ws, _ = cluster._sums(X, labels, k, None)
                return cluster.update_centroids(s, ws, c, "cosine")

            def torch_step():
                labels = torch_assign(X, ct)
                s = torch_sums(X, labels, k)
                return s / s.norm(dim=1, keepdim=True)

            whole = timed_group({"lloyd_step": step, "torch_lloyd_step": torch_step}, a.repeats)
            flop_floor = 2.0 * n * k * D / PEAK * 1e3
            read_floor = 4.0 * n * D / HBM * 1e3
            sums_alone = sums["cluster_sums_with_its_sort"]["median_ms"] - sums["stable_sort_of_labels"]["median_ms"]
            row = dict(N=n, D=D, K=k, assign=assign, sums=sums, step=whole, labels_equal_to_torch_fraction=round(agree, 6),
                       assign_floor_ms=round(flop_floor, 3), assign_floor_fraction=round(flop_floor / assign["kmeans_assign"]["median_ms"], 3),
                       assign_over_knn_search=round(assign["kmeans_assign"]["median_ms"] / assign["knn_search_k1"]["median_ms"], 3),
                       read_floor_ms=round(read_floor, 3), sums_kernels_ms=round(sums_alone, 3),
                       sums_kernels_over_read_floor=round(sums_alone / read_floor, 2))
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
            if a.out:  # after every row: a run that is cut short still leaves what it measured
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
        del X
        torch.cuda.empty_cache()
    if a.out:
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
