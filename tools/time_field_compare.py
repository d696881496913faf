#!/usr/bin/env python3
"""The field comparison at full size (C2 geometry: 1 M Gaussians, 1600 x 1060) beside the render it shares its walk with and the
literal form it replaces, all in one run on one device.  Two shapes: D = 512 with a full-resolution map, and the dino shape,
D = 1024 with a 64 x 64 map read through nearest upsampling.

  (r) render         gwbp_render of the field alone: the figure to measure the fused forms against (the same walk, a store of the
                     [H, W, D] image where they read the map)
  (a) fused_table    gwbp_field_compare, table only (what score_field_views runs per view)
  (b) fused_planes   the same with the six [H, W] planes written
  (c) literal        gwbp_render, then the five sums and the cosine as torch expressions on the [H, W, D] image (a low-resolution map
                     is expanded with F.interpolate first, as the literal form has to)

    timeout -k 10 1100 python tools/time_field_compare.py --out profiles/field_compare.json

Every view is projected, sorted and blended once, untimed; the forms then run on that view's weight store one after the other, in an
order that rotates from view to view, each between two hip events.  ms is the median over --views views after --warmup;
peak_extra_mib is the torch.cuda.max_memory_allocated delta of one call, its outputs included.  map_read_ms_at_hbm_peak is the
time of one read of the map at the device's peak HBM rate (--hbm-tbs): the allowance the fused table-only form has over the render.
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

SHAPES = (dict(name="full_512", dim=512, lowres=None), dict(name="dino_1024_64x64", dim=1024, lowres=(64, 64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="peak HBM rate in TB/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_field_compare.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    W, H, n = cfg.width, cfg.height, cfg.n_gaussians
    gauss = tuple(t.to(dev).contiguous() for t in syn.activate(syn.make_scene(cfg)))
    vms, K = syn.make_cameras(cfg, n_views=a.views + a.warmup), syn.intrinsics(cfg)
    eng = get_engine(dev, n, W, H)
    res = dict(tool="tools/time_field_compare.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"),
               config=a.config, n_gaussians=n, width=W, height=H, views=a.views, warmup=a.warmup, hbm_tbs=a.hbm_tbs, rows=[])

    def measure(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out

    for shape in SHAPES:
        dim, lowres = shape["dim"], shape["lowres"]
        g = torch.Generator(device=dev).manual_seed(dim)
        field = torch.nn.functional.normalize(torch.randn(n, dim, generator=g, device=dev), dim=1)
        mh, mw = lowres if lowres else (H, W)
        fmap = torch.randn(mh, mw, dim, generator=g, device=dev)
        fmap /= fmap.norm(dim=-1, keepdim=True)
        index = eng.nearest_maps(mh, mw, H, W) if lowres else None
        state = {}

        def literal():
            r = eng.render(state["view"], field)
            m = fmap
            if lowres:
                m = torch.nn.functional.interpolate(fmap.permute(2, 0, 1)[None], size=(H, W), mode="nearest")[0].permute(1, 2, 0)
            dot, rr, mm = (r * m).sum(-1), (r * r).sum(-1), (m * m).sum(-1)
            d = r - m
            l1, l2 = d.abs().sum(-1), (d * d).sum(-1)
            return torch.stack([dot, rr, mm, l1, l2, dot / (rr * mm).sqrt()])

        forms = dict(render=lambda: eng.render(state["view"], field),
                     fused_table=lambda: eng.field_compare(state["view"], field, fmap, index=index, want_planes=False)[1],
                     fused_planes=lambda: eng.field_compare(state["view"], field, fmap, index=index)[0],
                     literal=literal)
        names = list(forms)
        ms = {name: [] for name in names}
        peak, last = {}, {}
        for v in range(a.views + a.warmup):
            view = eng.view(vms[v], K, W, H)
            eng.project(view, *gauss)
            eng.bin_sort(view)
            eng.blend_weights(view)
            eng.holds_new_view()
            state["view"] = view
            for i in range(len(names)):
                name = names[(i + v) % len(names)]
                t, mem, out = measure(forms[name])
                if v >= a.warmup:
                    ms[name].append(t)
                    peak[name] = max(peak.get(name, 0.0), mem)
                last[name] = out if name in ("fused_planes", "literal") else None
                del out
        st = eng.stats()
        if st["overflow"]:
            raise SystemExit(f"workspace overflow (flags {st['overflow']}): the timings are void")
        row = dict(shape=shape["name"], D=dim, map_shape=[mh, mw, dim], map_mib=round(fmap.numel() * 4 / 2 ** 20, 1))
        for name in names:
            row[name] = dict(median_ms=round(statistics.median(ms[name]), 3), min_ms=round(min(ms[name]), 3),
                             max_ms=round(max(ms[name]), 3), views=len(ms[name]), peak_extra_mib=round(peak[name], 1))
        row["map_read_ms_at_hbm_peak"] = round(fmap.numel() * 4 / (a.hbm_tbs * 1e12) * 1e3, 3)
        row["fused_table_minus_render_ms"] = round(row["fused_table"]["median_ms"] - row["render"]["median_ms"], 3)
        row["literal_over_fused_table"] = round(row["literal"]["median_ms"] / row["fused_table"]["median_ms"], 2)
        a5, b5 = last["fused_planes"][:5].double(), last["literal"][:5].double()
        row["max_rel_diff_fused_vs_literal"] = float(((a5 - b5).abs() / b5.abs().clamp_min(1e-6)).max())
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        del field, fmap, last
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
