#!/usr/bin/env python3
"""The SH colours of a training step at full size (C2 geometry: 1 000 000 Gaussians, 1600 x 1060, SH degree 3) in one run on one
device, the forms of each comparison alternating inside every repeat:

  sh_torch     projection.sh_colors_torch on the concatenated [N, 16, 3] table (the cat included, as render_splats ran it) and its
               autograd backward to the coefficients and the means
  sh_kernels   sh.sh_colors on features_dc and features_rest as they are stored: k_sh_eval and k_sh_eval_bwd
  step_torch   polish_scene's training step (render -> photometric_loss -> backward -> Adam step) under set_sh_kernel(False)
  step_kernels the same step under set_sh_kernel(True)

    timeout -k 10 900 python tools/time_sh_grad.py --out profiles/sh_grad.json

Each form is timed between one pair of hip events around work that ends in a synchronise; ms is the median over --repeats, with min and
max.  peak_mib is torch.cuda.max_memory_allocated over the form, above what was allocated before it.  The kernel pair is also held
against its byte floor (forward reads 12 + 12 K B and writes 12 B per Gaussian, backward reads 24 + 12 K B and writes 12 K + 12 B) at
6.29 TB/s.  "errors": every case of tests/test_gpu_sh_grad.py's floor rule, measured with that file's own functions; FACTOR there is
ceil(2 x the largest ratio).  Nothing is asserted on the timings.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gsbp_amd  # noqa: E402,F401
import torch  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402
from gsbp_amd.polish import DEFAULT_LRS, PARAM_KEYS, render_splats  # noqa: E402
from gsbp_amd.rasterization import set_sh_kernel  # noqa: E402

HBM_TBPS = 6.29


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return out, t0.elapsed_time(t1), (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def make_splats(cfg, dev, degree=3):
    s = {k: t.contiguous().to(dev) for k, t in syn.make_scene(cfg).items()}
    n = s["means"].shape[0]
    gen = torch.Generator().manual_seed(syn.SH_SEED)
    s["features_dc"] = ((torch.rand(n, 1, 3, generator=gen) - 0.5) / 0.28209479177387814).to(dev)
    s["features_rest"] = (0.05 * torch.randn(n, (degree + 1) ** 2 - 1, 3, generator=gen)).to(dev)
    return s


def measure_errors(dev):
    import test_gpu_sh_grad as cases  # noqa: E402  (the test file's cases and its two sides)
    rows, top, worst = [], 0.0, None
    for n, d, k, name, k_head, shifted in cases.gradient_cases():
        r = cases.measure(dev, n, d, k, k_head, shifted)
        if not r:  # (N = 1: the Gaussian at the camera centre alone, checked on its own)
            continue
        key = max(r, key=r.get)  # one row per case: its largest ratio over 3 tensors x 2 figures
        rows.append(dict(n=n, degree=d, K=k, layout=name, tensor=key[0], figure=key[1], ratio=round(r[key], 4)))
        if r[key] > top:
            top, worst = r[key], rows[-1]
    return dict(cases=len(rows), figures=6 * len(rows), largest=round(top, 4), worst=worst, factor=math.ceil(2 * top),
                factor_in_test=cases.FACTOR, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sh_grad.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    errors = measure_errors(dev)
    print("errors", json.dumps({k: v for k, v in errors.items() if k != "rows"}), flush=True)
    cfg = syn.CONFIGS[a.config]
    W, H = cfg.width, cfg.height
    K, vms = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg, n_views=2).to(dev)
    full = make_splats(cfg, dev)
    n, k = full["means"].shape[0], 16
    with torch.no_grad():
        images = [render_splats(full, vms[v], K, W, H).clamp(0.0, 1.0) for v in range(2)]
    gen = torch.Generator().manual_seed(11)
    work = {key: (t + 0.01 * torch.randn(t.shape, generator=gen).to(dev)).requires_grad_(True) for key, t in full.items()}
    opt = torch.optim.Adam([dict(params=[work[PARAM_KEYS[name]]], lr=DEFAULT_LRS[name]) for name in PARAM_KEYS], eps=1e-15)
    campos = [(-(vm[:3, :3].T @ vm[:3, 3])).tolist() for vm in vms.cpu()]
    v_colors = torch.randn(n, 3, generator=gen).to(dev)
    leaves = (work["means"], work["features_dc"], work["features_rest"])

    def sh_pair(kernels, v):
        if kernels:
            out = gsbp_amd.sh_colors(3, leaves[0], leaves[1], campos[v], rest=leaves[2])
        else:
            out = gsbp_amd.sh_colors_torch(3, leaves[0], torch.cat([leaves[1], leaves[2]], dim=1), campos[v])
        return torch.autograd.grad(out, leaves, v_colors)

    def step(kernels, v):
        set_sh_kernel(kernels)
        opt.zero_grad(set_to_none=True)
        gsbp_amd.photometric_loss(render_splats(work, vms[v], K, W, H), images[v]).backward()
        opt.step()

    forms = dict(sh_torch=lambda v: sh_pair(False, v), sh_kernels=lambda v: sh_pair(True, v), step_torch=lambda v: step(False, v),
                 step_kernels=lambda v: step(True, v))
    ms = {name: [] for name in forms}
    peak = {name: 0.0 for name in forms}
    try:
        for rep in range(a.repeats + a.warmup):
            for name, fn in forms.items():
                _, t, p = timed(lambda: fn(rep % 2))
                if rep >= a.warmup:
                    ms[name].append(t)
                    peak[name] = max(peak[name], p)
    finally:
        set_sh_kernel(True)
    # the two pairs computed the same thing: a timing of a wrong result is no timing
    got, want = sh_pair(True, 0), sh_pair(False, 0)
    for g, w in zip(got, want):
        assert float((g - w).norm()) <= 1e-5 * float(w.norm()), "the kernel pair and the torch chain disagree"
    timing = dict(tool="tools/time_sh_grad.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), config=a.config,
                  n_gaussians=n, width=W, height=H, sh_degree=3, repeats=a.repeats, warmup=a.warmup, forms={})
    for name, ts in ms.items():
        timing["forms"][name] = dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                                     peak_mib=round(peak[name], 1))
        print(name, json.dumps(timing["forms"][name]), flush=True)
    f = timing["forms"]
    floor_bytes = n * ((12 + 12 * k + 12) + (24 + 12 * k + 12 * k + 12))
    floor_ms = floor_bytes / (HBM_TBPS * 1e12) * 1e3
    timing["sh_torch_over_sh_kernels"] = round(f["sh_torch"]["median_ms"] / f["sh_kernels"]["median_ms"], 3)
    timing["step_torch_over_step_kernels"] = round(f["step_torch"]["median_ms"] / f["step_kernels"]["median_ms"], 4)
    timing["byte_floor"] = dict(bytes=floor_bytes, tb_per_s=HBM_TBPS, floor_ms=round(floor_ms, 4),
                                sh_kernels_over_floor=round(f["sh_kernels"]["median_ms"] / floor_ms, 3))
    timing["kernel_route_is_default"] = f["step_kernels"]["median_ms"] <= f["step_torch"]["median_ms"]
    print("timing", json.dumps({key: v for key, v in timing.items() if key != "forms"}), flush=True)
    timing["errors"] = errors
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(timing, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
