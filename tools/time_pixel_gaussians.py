#!/usr/bin/env python3
"""The per-pixel Gaussian lists at full size (C2 geometry: 1 M Gaussians, 1600 x 1060), all in one run on one device:

  render_px_d4     gwbp_render_pixels with D = 4 on the projected and sorted view: the same walk with four accumulators
  lists_k{1,4,8,16}  gwbp_pixel_gaussians, image form, on the same projected and sorted view
  probe_m{1,256}   gwbp_pixel_gaussians, pixel-list form, k = 4
  torch_pairs_k4   the form without the kernel: a storing blend + dump_pairs + torch sorts, cut to the top 4 per pixel

    timeout -k 10 900 python tools/time_pixel_gaussians.py --out profiles/pixel_gaussians.json

Each view is projected and sorted once; the kernel forms then alternate, --reps launches between one pair of hip events each, and ms
is the median over --views views of the time per launch.  torch_pairs_k4 is timed on --torch-views of them, blend included (it needs
the weight store; the projection and sort are not counted for any form), with its torch.cuda.max_memory_allocated delta.
ratio_over_render_px_d4 is each list form's median over render_px_d4's.  ids_equal: the torch form's lists equal the kernel's.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gsbp_amd  # noqa: E402,F401
import torch  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402
from gsbp_amd.rasterization import get_engine  # noqa: E402

KS = (1, 4, 8, 16)


def torch_lists(eng, view, k, n_pixels):
    """The top-k lists from the weight store's triples in torch: three stable sorts (id, weight descending, pixel), cut at rank k."""
    eng.blend_weights(view)
    gid, pix, w = eng.dump_pairs(view)
    by_id = torch.sort(gid, stable=True).indices
    by_w = by_id[torch.sort(w[by_id], descending=True, stable=True).indices]
    by_pix = torch.sort(pix[by_w].long(), stable=True)
    order = by_w[by_pix.indices]
    p = by_pix.values
    counts = torch.bincount(p, minlength=n_pixels)
    start = torch.cumsum(counts, 0) - counts
    rank = torch.arange(p.shape[0], device=p.device) - start[p]
    keep = rank < k
    ids = torch.full((n_pixels, k), -1, dtype=torch.int32, device=p.device)
    weights = torch.zeros(n_pixels, k, device=p.device)
    ids[p[keep], rank[keep]] = gid[order][keep]
    weights[p[keep], rank[keep]] = w[order][keep]
    return ids, weights, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--torch-views", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pixel_gaussians.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    W, H, n = cfg.width, cfg.height, cfg.n_gaussians
    gauss = tuple(t.to(dev).contiguous() for t in syn.activate(syn.make_scene(cfg)))
    vms, K = syn.make_cameras(cfg, n_views=a.views + a.warmup), syn.intrinsics(cfg)
    eng = get_engine(dev, n, W, H)
    colors = torch.rand(n, 4, generator=torch.Generator().manual_seed(1)).to(dev)
    g = torch.Generator().manual_seed(2)
    xy = torch.stack([torch.randint(0, W, (256,), generator=g), torch.randint(0, H, (256,), generator=g)], 1).to(torch.int32).to(dev)

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps, out

    def front(v, store=False):
        """View v projected and sorted (and, with store, blended) in a workspace that holds it: an overflow grows the workspace."""
        for _ in range(6):
            view = eng.view(vms[v], K, W, H)
            eng.project(view, *gauss)
            eng.bin_sort(view)
            if store:
                eng.blend_weights(view)
            stats = eng.stats()
            if not stats["overflow"]:
                return view
            eng.grow(stats, views=1)
        raise SystemExit("the workspace kept overflowing")

    ms, peak, ids_equal, contrib = {}, 0.0, None, None
    for v in range(a.views + a.warmup):
        view = front(v, store=a.warmup <= v < a.warmup + a.torch_views)  # (sized for the storing blend before anything is timed)
        forms = {"render_px_d4": lambda: eng.render_pixels(view, colors)}
        forms.update({f"lists_k{k}": (lambda k=k: eng.pixel_gaussians(view, k)) for k in KS})
        forms.update({f"probe_m{m}": (lambda m=m: eng.pixel_gaussians(view, 4, xy[:m])) for m in (1, 256)})
        last = {}
        for name, fn in forms.items():
            t, last[name] = timed(fn, a.reps)
            if v >= a.warmup:
                ms.setdefault(name, []).append(t)
        if a.warmup <= v < a.warmup + a.torch_views:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t, (ids, weights, counts) = timed(lambda: torch_lists(eng, view, 4, W * H), 1)
            ms.setdefault("torch_pairs_k4", []).append(t)
            peak = max(peak, (torch.cuda.max_memory_allocated() - base) / 2 ** 20)
            k4 = last["lists_k4"]
            ids_equal = bool(torch.equal(ids, k4[0].reshape(-1, 4)) and torch.equal(weights, k4[1].reshape(-1, 4))
                             and torch.equal(counts.int(), k4[2].reshape(-1)))
            contrib = dict(mean=round(float(counts.float().mean()), 2), max=int(counts.max()), pairs=int(counts.sum()))
            del ids, weights, counts
            torch.cuda.empty_cache()
    res = dict(tool="tools/time_pixel_gaussians.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"),
               config=a.config, n_gaussians=n, width=W, height=H, views=a.views, torch_views=a.torch_views, warmup=a.warmup,
               reps=a.reps, n_contrib=contrib, forms={})
    base_ms = statistics.median(ms["render_px_d4"])
    for name, ts in ms.items():
        row = dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), views=len(ts))
        if name.startswith("lists_k") or name == "torch_pairs_k4":
            row["ratio_over_render_px_d4"] = round(statistics.median(ts) / base_ms, 3)
        if name == "torch_pairs_k4":
            row["peak_extra_mib"], row["ids_equal"] = round(peak, 1), ids_equal
        res["forms"][name] = row
        print(name, json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
