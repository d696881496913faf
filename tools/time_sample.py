#!/usr/bin/env python3
"""Times the point samples (csrc/sample.hip) and writes profiles/sample.json.

    python tools/time_sample.py [--n 1000000] [--dims 512,1024] [--ks 8,16] [--repeats 3] [--out profiles/sample.json]

Scenes: the first N Gaussians of the C2 synthetic scene with (a) as many points as Gaussians, the means jittered by the median
reach, and (b) 100 000 points scattered uniformly over the scene's box; and (c) the clustered set of tools/time_spatial.py
(spatial.clustered_points: densities over two decades, the dense-cell case) with isotropic scales from init_scales, seeded
quaternions and opacities, points = jittered means.  The radius is suggest_sample_radius at the 0.99 quantile.

Per scene and k, timed with device events, the forms alternating inside one round, one warm-up round, the median over the rounds:
  walk            gwbp_point_gaussians (the entry point alone: grid, pack and the queries' order are built once, outside)
  radius_count    gwbp_radius_count(cap = INT32_MAX) on the same grid, queries, order and radius: the same walk without the weight
  spatial_knn     gwbp_spatial_knn(k) on the same grid, queries and order
  pack            gwbp_gaussian_pack
and per D (a seeded normal field): blend (gwbp_neighbor_blend) against neighbor_mean (gwbp_neighbor_mean) on the walk's index list, both through their
Python wrappers (they include the allocation of the outputs, the caching allocator's after the warm-up round).  The expectation
the blend is reported against: at most 1.25 x neighbor_mean.  No ratio is fixed for the walk; both ratios and the mean `visited` are
recorded.  The form without the kernels -- a chunked torch brute force of the Mahalanobis weights plus topk, and (w[..., None] *
F[idx]).sum(1) / W -- runs on the first --torch-queries points only (the full set would take Q / that many times as long) with
its peak memory.  The file is rewritten after every case.
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
from gsbp_amd import components as comp, sample, spatial, synthetic as syn  # noqa: E402
from gsbp_amd._lib import ptr  # noqa: E402
from gsbp_amd._views import ld, run  # noqa: E402

INT32_MAX = 2 ** 31 - 1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def med(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def rotations(q):
    q = torch.nn.functional.normalize(q.double(), dim=1)
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3).float()


def torch_form(points, gauss, feats, k, radius, alpha_min, chunk=256):
    """(out [Q, D], idx [Q, k], peak bytes): every point against every Gaussian in chunks of points, topk, gather, weighted mean."""
    means, quats, scales, opac = gauss
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    M = rotations(quats).transpose(1, 2) / scales[:, :, None]  # [N, 3, 3]
    outs, ids = [], []
    for a in range(0, points.shape[0], chunk):
        d = points[a:a + chunk, None, :] - means[None, :, :]                # [c, N, 3]
        u = torch.einsum("nab,cnb->cna", M, d)
        w = opac[None, :] * torch.exp(-0.5 * (u * u).sum(-1))
        w = torch.where((w >= alpha_min) & ((d * d).sum(-1) <= radius * radius), w, torch.zeros_like(w))
        tw, ti = torch.topk(w, k, dim=1)
        W = tw.sum(1, keepdim=True)
        outs.append((tw[..., None] * feats[ti]).sum(1) / W.clamp(min=1e-30))
        ids.append(ti)
    torch.cuda.synchronize()
    return torch.cat(outs), torch.cat(ids), torch.cuda.max_memory_allocated() - base


def scenes(n, dev):
    g = torch.Generator().manual_seed(7)
    splats = syn.make_scene(syn.CONFIGS["C2"])
    gauss = tuple(t[:n].float().to(dev).contiguous() for t in syn.activate(splats))
    reach = sample.reach(gauss[2], gauss[3])
    jitter = float(reach[reach > 0].median())
    m = gauss[0].cpu()
    lo, hi = m.quantile(0.01, dim=0) if n <= 2 ** 24 else m.min(0).values, m.quantile(0.99, dim=0) if n <= 2 ** 24 else m.max(0).values
    yield "c2_jittered_means", gauss, (m + jitter * torch.randn(m.shape, generator=g)).to(dev)
    yield "c2_scattered_100k", gauss, (lo + (hi - lo) * torch.rand(100_000, 3, generator=g)).to(dev)
    nc = min(n, 200_000)
    pts = spatial.clustered_points(nc, seed=0).to(dev)
    sc = torch.exp(gsbp_amd.init_scales(pts)).clamp(min=1e-6, max=1.0).contiguous()
    sc = torch.where(torch.isfinite(sc), sc, torch.full_like(sc, 1e-3))
    cl = (pts, torch.randn(nc, 4, generator=g).to(dev), sc, (0.05 + 0.95 * torch.rand(nc, generator=g)).to(dev))
    jit = float(sample.reach(cl[2], cl[3]).median())
    yield "clustered_200k_dense_cells", cl, (pts.cpu() + jit * torch.randn(nc, 3, generator=g)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="512,1024")
    ap.add_argument("--ks", default="8,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--torch-queries", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_sample.py needs a GPU")
    dev = torch.device("cuda")
    a_min = sample.ALPHA_MIN
    res = {"tool": "tools/time_sample.py", "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "repeats": args.repeats, "timing": "device events; the forms alternate inside a round, one warm-up round, median over the rounds; walk, "
           "radius_count, spatial_knn and pack are the entry points alone on one prebuilt grid; blend and neighbor_mean go through their "
           "Python wrappers and include the allocation of their outputs (caching allocator)",
           "expectation": "blend <= 1.25 x neighbor_mean on the same index list; no ratio fixed for the walk", "cases": []}
    dims, ks = [int(s) for s in args.dims.split(",")], [int(s) for s in args.ks.split(",")]
    for name, gauss, points in scenes(args.n, dev):
        means, quats, scales, opac = gauss
        n, nq = means.shape[0], points.shape[0]
        radius = gsbp_amd.suggest_sample_radius(scales, opac)
        r2 = comp._r2(radius)
        grid = comp._plan(means, radius, None, None)
        srt, cell_start, perm = comp._build(means, grid)
        order = spatial.sorted_keys(points, grid)[1]
        pack = torch.empty(n, sample.PACK, dtype=torch.float32, device=dev)
        gargs = spatial.grid_args(grid)

        def do_pack():
            run("gwbp_gaussian_pack", dev, C.c_int64(n), ptr(means), C.c_int64(ld(means)), ptr(quats), C.c_int64(ld(quats)), ptr(scales),
                C.c_int64(ld(scales)), ptr(opac), None, ptr(perm), ptr(pack))

        do_pack()
        count = torch.empty(nq, dtype=torch.int32, device=dev)
        visited = torch.empty(nq, dtype=torch.int32, device=dev)
        for k in ks:
            idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
            w = torch.empty(nq, k, dtype=torch.float32, device=dev)
            kidx, kdist = torch.empty_like(idx), torch.empty_like(w)
            nc = torch.empty(nq, dtype=torch.int32, device=dev)
            forms = {
                "walk": lambda: run("gwbp_point_gaussians", dev, C.c_int64(n), ptr(srt), ptr(cell_start), *gargs, ptr(pack), C.c_float(r2),
                                    C.c_float(a_min), C.c_int64(nq), ptr(points), C.c_int64(ld(points)), ptr(order), k, ptr(idx), ptr(w),
                                    ptr(nc), ptr(visited)),
                "radius_count": lambda: run("gwbp_radius_count", dev, C.c_int64(n), ptr(srt), ptr(cell_start), *gargs, None, C.c_float(r2),
                                            C.c_int64(nq), ptr(points), C.c_int64(ld(points)), ptr(order), None, INT32_MAX, ptr(count), None),
                "spatial_knn": lambda: run("gwbp_spatial_knn", dev, C.c_int64(n), ptr(srt), ptr(cell_start), *gargs, C.c_int64(nq), ptr(points),
                                           C.c_int64(ld(points)), ptr(order), k, ptr(kidx), ptr(kdist)),
                "pack": do_pack,
            }
            times = {}
            for rnd in range(args.repeats + 1):
                for form, fn in forms.items():
                    ms = timed(fn)[0]
                    if rnd:
                        times.setdefault(form, []).append(ms)
            case = {"scene": name, "n": n, "q": nq, "k": k, "radius": radius, "grid": spatial.grid_stats(grid, cell_start)}
            case.update({form: med(v) for form, v in times.items()})
            case["walk_over_radius_count"] = round(case["walk"]["median_ms"] / case["radius_count"]["median_ms"], 3)
            case["walk_over_spatial_knn"] = round(case["walk"]["median_ms"] / case["spatial_knn"]["median_ms"], 3)
            case["visited_mean"] = float(visited.double().mean())
            case["candidates_mean"] = float(count.double().mean())
            case["n_contrib_mean"] = float(nc.double().mean())
            case["valid_share"] = float((nc > 0).double().mean())
            case["truncated_share"] = float((nc > k).double().mean())
            case["blend"] = []
            for d in dims:
                f = torch.randn(n, d, device=dev, generator=torch.Generator(device=dev).manual_seed(d))
                bt = {}
                for rnd in range(args.repeats + 1):
                    for form, fn in (("blend", lambda: sample.neighbor_blend(f, idx, w)), ("neighbor_mean", lambda: spatial.neighbor_mean(f, idx))):
                        ms = timed(fn)[0]
                        if rnd:
                            bt.setdefault(form, []).append(ms)
                row = {"D": d, **{form: med(v) for form, v in bt.items()}}
                row["blend_over_neighbor_mean"] = round(row["blend"]["median_ms"] / row["neighbor_mean"]["median_ms"], 3)
                tq = min(args.torch_queries, nq)
                torch_form(points[:64], gauss, f, k, radius, a_min)  # warm-up
                ms, (lit, lidx, peak) = timed(lambda: torch_form(points[:tq], gauss, f, k, radius, a_min))
                ours = sample.neighbor_blend(f, idx[:tq].contiguous(), w[:tq].contiguous())[0]
                full = (nc[:tq] > 0) & (nc[:tq] <= k)  # rows where both forms blend the same set
                row["torch_form"] = {"queries": tq, "ms": round(ms, 3), "ms_per_million_queries": round(ms * 1e6 / tq, 1), "peak_bytes": int(peak),
                                     "max_abs_difference": float((lit[full] - ours[full]).abs().max()) if bool(full.any()) else 0.0}
                case["blend"].append(row)
                del f, lit, ours
                torch.cuda.empty_cache()
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
