#!/usr/bin/env python3
"""Per-pixel weight maps (create_feature_field(pixel_weight_fn=...)) at full size: ms per view of the default schedule with no
map and with each of the maps below, the variants of one config ALTERNATING inside every round so that drift hits them alike.

    timeout -k 10 1500 python tools/time_pixel_weights.py --configs C2,DINO64,LSEG480 --out profiles/pixel_weights.json

Maps (one object for every view, made before the timed calls):
  none          no pixel_weight_fn
  ones_f32      all-ones float32
  ones_u8       all-ones uint8
  border5       bool: a band of 5 % of the smaller side along the edges is 0
  half          bool: the right half of the image is 0
  workaround    (low-resolution configs) what a caller does without the feature: the materialised c * upsample(f) map
                through the pixel-slab scatter, plus a second job on the one-channel map c for d (F.interpolate inside the
                timed region, once per view)
Each entry: create_feature_field over --views views, hip events around the whole call after one untimed call; the last of
--rounds rounds is reported, with the ratio to "none" of the same round.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gsbp_amd  # noqa: E402  (before the first HIP call: hardware queues)
import torch  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402


def _events(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def _maps(cfg, dev):
    H, W = cfg.height, cfg.width
    border = torch.zeros(H, W, dtype=torch.bool, device=dev)
    b = int(0.05 * min(H, W))
    border[b:H - b, b:W - b] = True
    half = torch.zeros(H, W, dtype=torch.bool, device=dev)
    half[:, : W // 2] = True
    return {"ones_f32": torch.ones(H, W, device=dev), "ones_u8": torch.ones(H, W, dtype=torch.uint8, device=dev),
            "border5": border, "half": half}


def run_config(name, views, rounds, dev):
    cfg = syn.CONFIGS[name]
    g = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    vms, K = syn.make_cameras(cfg, n_views=views), syn.intrinsics(cfg)
    feats = syn.make_feature_map(cfg, 0, device=dev)
    args = (*g, vms, K, cfg.width, cfg.height)
    kw = dict(upsample=cfg.upsample, reduction=cfg.reduction)
    maps = _maps(cfg, dev)
    jobs = {"none": lambda: gsbp_amd.create_feature_field(*args, lambda v: feats, cfg.feat_dim, **kw)}
    for k, c in maps.items():
        jobs[k] = (lambda c: lambda: gsbp_amd.create_feature_field(*args, lambda v: feats, cfg.feat_dim, pixel_weight_fn=lambda v: c,
                                                                   **kw))(c)
    if cfg.upsample is not None:
        c = maps["half"].float()

        def workaround():
            up = lambda v: syn.upsample_map(cfg, feats) * c[..., None]  # noqa: E731
            gsbp_amd.create_feature_field(*args, up, cfg.feat_dim, reduction=cfg.reduction)
            gsbp_amd.create_feature_field(*args, lambda v: c[..., None], 1, reduction="sum")
        jobs["workaround"] = workaround
    rows = {}
    for r in range(rounds):
        for k, fn in jobs.items():
            fn()
            ms = _events(fn) / views
            rows[k] = dict(config=name, map=k, ms_view=round(ms, 4), round=r)
        for k in rows:
            rows[k]["vs_none"] = round(rows[k]["ms_view"] / rows["none"]["ms_view"], 4)
        print(json.dumps(list(rows.values())), flush=True)
    del feats
    torch.cuda.empty_cache()
    return list(rows.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,DINO64,LSEG480")
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name in a.configs.split(","):
        rows += run_config(name, a.views, a.rounds, dev)
    res = dict(tool="tools/time_pixel_weights.py", device=torch.cuda.get_device_name(0), views=a.views, rounds=a.rounds,
               date=time.strftime("%Y-%m-%d"), rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
