#!/usr/bin/env python3
"""The label render and its score at full size (C2 geometry: 1 M Gaussians, 1600 x 1060) for K = 8 and K = 150 classes, beside the
two forms it replaces, all in one run on one device:

  (a) fused_counts   project + bin_sort + gwbp_render_labels with counts only (what score_label_views runs per view)
  (b) fused_maps     the same with the [H, W, K] maps and the alpha map written as well
  (c) one_hot_torch  rasterization() of the one-hot [N, K] table, then the same threshold and counts in torch on the device
  (d) reference      the reference's literal form (demo_affordance_transfer.py:1555-1580): per class 1 .. K-1 a 3-channel
                     indicator render, copied to the host, thresholded and counted in numpy

    timeout -k 10 1100 python tools/time_label_eval.py --out profiles/label_eval.json

Every form takes a whole view from nothing (its own projection and sort; the front cache is dropped before each call), is warmed up
on the first views and timed with hip events around one whole view; the forms alternate view by view, and ms is the median over
--views views ((d) is timed on --reference-views of them: it costs K - 1 renders and copies per view).  peak_extra_mib is the
torch.cuda.max_memory_allocated delta of one view, outputs and the one-hot table included.  counts_equal says whether (a), (c) and
(d) counted the same on the last view they share.
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
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402
from gsbp_amd.rasterization import get_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--classes", default="8,150")
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--reference-views", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cut", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_label_eval.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    W, H, n = cfg.width, cfg.height, cfg.n_gaussians
    gauss = tuple(t.to(dev).contiguous() for t in syn.activate(syn.make_scene(cfg)))
    vms, K = syn.make_cameras(cfg, n_views=a.views + a.warmup).to(dev), syn.intrinsics(cfg).to(dev)
    vm_host, K_host = vms.cpu(), K.cpu()
    eng = get_engine(dev, n, W, H)
    res = dict(tool="tools/time_label_eval.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), config=a.config,
               n_gaussians=n, width=W, height=H, views=a.views, reference_views=a.reference_views, warmup=a.warmup, cut=a.cut, rows=[])
    thr = float(a.cut + 1)

    def measure(fn, v):
        eng.front_cache = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn(v)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out

    for k in [int(x) for x in a.classes.split(",")]:
        labels = torch.randint(0, k, (n,), generator=torch.Generator().manual_seed(k), dtype=torch.int32).to(dev)
        gts = [syn.make_label_map(cfg, v, k, device=dev) for v in range(a.views + a.warmup)]

        def fused(v, maps):
            view = eng.view(vm_host[v], K_host, W, H)
            eng.project(view, *gauss)
            eng.bin_sort(view)
            eng.holds_new_view()
            return eng.render_labels(view, labels, k, want_maps=maps, want_alphas=maps, gt=gts[v], cut=a.cut)[3]

        def one_hot_torch(v):
            table = torch.zeros(n, k, device=dev)
            table.scatter_(1, labels.long()[:, None], 1.0)
            with torch.no_grad():
                maps = gsbp_amd.rasterization(*gauss, table, vms[v:v + 1], K[None], W, H, want_meta=False)[0][0]
            pred = (maps.clamp(0.0, 1.0) * 255.0) >= thr
            truth = gts[v][..., None] == torch.arange(k, device=dev)
            return torch.stack([(pred & truth).sum(dim=(0, 1)), pred.sum(dim=(0, 1)), truth.sum(dim=(0, 1))], dim=1)

        def reference(v):
            counts = np.zeros((k, 3), np.int64)
            gt_label = gts[v].cpu().numpy()
            for i in range(1, k):
                colors = (labels == i).float()[:, None].expand(n, 3).contiguous()
                with torch.no_grad():
                    out = gsbp_amd.rasterization(*gauss, colors, vms[v:v + 1], K[None], W, H, want_meta=False,
                                                 backgrounds=torch.zeros(1, 3, device=dev))[0][0]
                output_cv = (out.clamp(0.0, 1.0) * 255.0).to(torch.uint8).cpu().numpy()
                gt_mask, mask = gt_label == i, output_cv[..., 0] > a.cut
                counts[i] = (np.logical_and(gt_mask, mask).sum(), mask.sum(), gt_mask.sum())
            return counts

        forms = dict(fused_counts=lambda v: fused(v, False), fused_maps=lambda v: fused(v, True), one_hot_torch=one_hot_torch,
                     reference=reference)
        ms = {name: [] for name in forms}
        peak, last = {}, {}
        for v in range(a.views + a.warmup):
            for name, fn in forms.items():
                if name == "reference" and v >= a.warmup + a.reference_views:
                    continue
                t, mem, out = measure(fn, v)
                if v >= a.warmup:
                    ms[name].append(t)
                    peak[name] = max(peak.get(name, 0.0), mem)
                    if v == a.warmup + min(a.reference_views, a.views) - 1:
                        last[name] = np.asarray(out.cpu() if torch.is_tensor(out) else out)
        row = dict(num_classes=k)
        for name in forms:
            row[name] = dict(median_ms=round(statistics.median(ms[name]), 3), min_ms=round(min(ms[name]), 3),
                             max_ms=round(max(ms[name]), 3), views=len(ms[name]), peak_extra_mib=round(peak[name], 1))
        row["counts_equal"] = dict(fused_vs_one_hot_torch=bool(np.array_equal(last["fused_counts"], last["one_hot_torch"])),
                                   fused_vs_reference_classes_1_up=bool(np.array_equal(last["fused_counts"][1:], last["reference"][1:])))
        row["one_hot_torch_over_fused_counts"] = round(row["one_hot_torch"]["median_ms"] / row["fused_counts"]["median_ms"], 2)
        row["reference_over_fused_counts"] = round(row["reference"]["median_ms"] / row["fused_counts"]["median_ms"], 2)
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        del labels, gts
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
