#!/usr/bin/env python3
"""fp32 vs fp16 / bf16 feature maps: the dominant kernel's time and the step time per view, on the synthetic scenes of bench.py.

    timeout -k 10 900 python tools/time_half_maps.py --out profiles/half_maps.json

Configurations: C2 (full resolution, D = 512: the 256-channel kernel), LSEG480 (a 480 x 480 x 512 map, bilinear), DINO64
(64 x 64 x 1024 tokens: token space).  Variants of the same values:
  fp32       the map as float32
  f16, bf16  the map as float16 / bfloat16, read natively (the typed entry points)
  bf16_copy  a bfloat16 map that the caller widens with .float() before every view, then the fp32 path: what a caller had to do
             before half maps were accepted
Kernel: view 0 projected, sorted and blended once, then its scatter (scatter_tokens for DINO64) timed alone with hip events,
--reps times (the bf16_copy kernel time is that of the fp32 kernel on the copy; the copy is timed on its own as copy_ms).
Step: create_feature_field over --views views (the product path), hip events around the whole call after one untimed build;
every view gets the same map object, so the step time is the back-projection's plus, for bf16_copy, the copy.
Every configuration runs all variants --rounds times in turn and reports the last round (the first round of the first variant
carries the process's warm-up: allocations, code loading).
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

CONFIGS = ["C2", "LSEG480", "DINO64"]
VARIANTS = ["fp32", "f16", "bf16", "bf16_copy"]


def _events(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def run_config(name, views, reps, rounds, dev):
    cfg = syn.CONFIGS[name]
    g = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    vms, K = syn.make_cameras(cfg, n_views=views), syn.intrinsics(cfg)
    base = syn.make_feature_map(cfg, 0, device=dev)
    maps = {"fp32": base, "f16": base.half(), "bf16": base.bfloat16()}
    maps["bf16_copy"] = maps["bf16"]
    tokens = cfg.upsample == "nearest"
    upsample = None if tokens else cfg.upsample
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev, tight_binning=True)
    view = eng.view(vms[0], K, cfg.width, cfg.height)
    eng.project(view, *g)
    eng.bin_sort(view)
    if tokens:
        eng.blend_tokens(view, base.shape[0], base.shape[1])
    else:
        eng.blend_weights(view)
    F = torch.zeros(cfg.n_gaussians, cfg.feat_dim, device=dev)
    out = []
    for var in [v for _ in range(rounds) for v in VARIANTS]:
        m = maps[var]
        km = m.float() if var == "bf16_copy" else m
        if tokens:
            def kern():
                eng.scatter_tokens(view, km, F, None)
        else:
            def kern():
                eng.scatter(view, km, F, None, upsample=upsample)
        kern()
        torch.cuda.synchronize()
        kernel_ms = _events(kern, reps)
        copy_ms = _events(lambda: m.float(), reps) if var == "bf16_copy" else 0.0
        fn = (lambda v: m.float()) if var == "bf16_copy" else (lambda v: m)

        def build():
            return gsbp_amd.create_feature_field(*g, vms.to(dev), K.to(dev), cfg.width, cfg.height, fn, cfg.feat_dim,
                                                 return_partials=True, upsample=cfg.upsample, reduction=cfg.reduction)
        build()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _, _, _, st = build()
        t1.record()
        torch.cuda.synchronize()
        line = {"config": name, "variant": var, "map_dtype": str(m.dtype).replace("torch.", ""),
                "map_shape": list(m.shape), "kernel_ms": round(kernel_ms, 4), "copy_ms": round(copy_ms, 4),
                "step_ms_per_view": round(t0.elapsed_time(t1) / views, 4), "views": views,
                "n_pairs_per_view": int(st["n_pairs"]) // views, "overflow": int(st["overflow"])}
        print(json.dumps(line), flush=True)
        out.append(line)
    return out[-len(VARIANTS):]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=CONFIGS)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20, help="kernel launches timed per variant")
    ap.add_argument("--rounds", type=int, default=2, help="passes over the variants; the last one is reported")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []
    for name in args.configs:
        results += run_config(name, args.views, args.reps, args.rounds, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
