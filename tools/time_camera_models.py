#!/usr/bin/env python3
"""ms/view of the field build at C2 geometry (1M Gaussians, 1600 x 1060, D = 512) under the camera settings of
gwbp_project_camera, and a projection-only loop for kernel statistics.

    python tools/time_camera_models.py --views 20 --out profiles/camera_models_C2.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_camera_models.py --project-only fisheye:antialiased

The field build is create_feature_field (the product path: view pipeline, tight binning) with hip events around the whole
view loop; one untimed build first.  The feature map is one fixed [H, W, 512] tensor handed out for every view, so the time is
the back-projection's.  Pair counts differ between camera models (a fisheye view sees more of the scene), so every line
reports n_pairs beside its time.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gsbp_amd  # noqa: E402  (before the first HIP call: hardware queues)
import torch  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402

SETTINGS = ["pinhole:classic", "fisheye:classic", "pinhole:antialiased", "fisheye:antialiased"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--settings", nargs="*", default=SETTINGS, help="model:mode pairs")
    ap.add_argument("--project-only", default=None, metavar="MODEL:MODE",
                    help="run only the projection, --views times, for rocprofv3 kernel statistics")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = syn.CONFIGS[args.config]
    dev = torch.device("cuda:0")
    means, quats, scales, opac = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    vms, K = syn.make_cameras(cfg, n_views=args.views), syn.intrinsics(cfg)

    if args.project_only:
        model, mode = args.project_only.split(":")
        eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, tight_binning=True)
        for v in range(args.views):
            view = eng.view(vms[v], K, cfg.width, cfg.height, camera_model=model, rasterize_mode=mode)
            eng.project(view, means, quats, scales, opac)
        torch.cuda.synchronize()
        print(json.dumps({"project_only": args.project_only, "views": args.views}))
        return

    feats = syn.make_feature_map(cfg, 0, device=dev)
    results = []
    for s in args.settings:
        model, mode = s.split(":")

        def build():
            return gsbp_amd.create_feature_field(means, quats, scales, opac, vms.to(dev), K.to(dev), cfg.width, cfg.height,
                                                 lambda v: feats, cfg.feat_dim, return_partials=True, camera_model=model,
                                                 rasterize_mode=mode)

        build()  # warm-up (and capacity growth, if any)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _, _, _, st = build()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.views
        line = {"config": args.config, "camera_model": model, "rasterize_mode": mode, "views": args.views,
                "ms_per_view": round(ms, 4), "n_pairs_per_view": int(st["n_pairs"]) // args.views,
                "n_visible_per_view": int(st["n_visible"]) // args.views, "overflow": int(st["overflow"])}
        print(json.dumps(line), flush=True)
        results.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
