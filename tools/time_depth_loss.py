#!/usr/bin/env python3
"""Times the depth losses (csrc/depth_loss.hip) on one GPU and writes profiles/depth_loss.json.

  * the point term at M points and the map term (both kinds), forward + backward to the render and alpha leaves, at --width x --height
    with a 4-channel render: the fused kernels against the literal torch float32 statement (ED division, grid_sample, where, l1_loss),
    the two alternating inside every repeat; medians of --repeats event-timed runs with min and max;
  * one train_scene step with and without depth_fn at --config, from the difference of two run lengths, each measured --train-repeats
    times (six by default: median, min and max), the two alternating.  The run without the keyword is the code path the parent
    commit has; check out the parent and run this tool with --train-only to put its figure beside this one (the tool then leaves
    the depth part out).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gsbp_amd  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402
from gsbp_amd.polish import render_splats  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def summary(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), runs=len(ts))


def literal_points(render, alpha, points, depths):
    H, W = render.shape[:2]
    ed = (render[..., 3:4] / alpha[..., None].clamp_min(1e-10))[None]
    grid = torch.stack([points[:, 0] / (W - 1) * 2 - 1, points[:, 1] / (H - 1) * 2 - 1], dim=-1)[None, :, None, :]
    d = torch.nn.functional.grid_sample(ed.permute(0, 3, 1, 2), grid, align_corners=True).squeeze(3).squeeze(1)
    disp = torch.where(d > 0.0, 1.0 / d, torch.zeros_like(d))
    return torch.nn.functional.l1_loss(disp, 1.0 / depths[None])


def literal_map(render, alpha, depth, kind):
    e = render[..., 3] / alpha.clamp_min(1e-10)
    valid = depth > 0
    if kind == "depth":
        t = (e - depth).abs()
    else:
        t = (torch.where(e > 0, 1.0 / e, torch.zeros_like(e)) - 1.0 / torch.where(valid, depth, torch.ones_like(depth))).abs()
    return torch.where(valid, t, torch.zeros_like(t)).sum() / valid.sum()


def time_losses(dev, W, H, M, repeats, warmup):
    gen = torch.Generator().manual_seed(3)
    alpha = (0.2 + 0.8 * torch.rand(H, W, generator=gen)).to(dev)
    render = torch.rand(H, W, 4, generator=gen).to(dev)
    render[..., 3] = (0.5 + 7.5 * torch.rand(H, W, generator=gen)).to(dev) * alpha
    points = (torch.rand(M, 2, generator=gen) * torch.tensor([W - 1.0, H - 1.0])).to(dev)
    depths = (0.5 + 7.5 * torch.rand(M, generator=gen)).to(dev)
    depth_map = (0.5 + 7.5 * torch.rand(H, W, generator=gen)).to(dev)

    def both(loss_fn):
        def run():
            r, a = render.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
            loss_fn(r, a).backward()
        return run

    forms = {
        "points_fused": both(lambda r, a: gsbp_amd.depth_point_loss(r, a, points, depths)),
        "points_torch": both(lambda r, a: literal_points(r, a, points, depths)),
        "leaf_clones_only": both(lambda r, a: (r[0, 0, 0] + a[0, 0])),
    }
    for kind in ("disparity", "depth"):
        forms[f"map_{kind}_fused"] = both(lambda r, a, kind=kind: gsbp_amd.depth_map_loss(r, a, depth_map, kind=kind))
        forms[f"map_{kind}_torch"] = both(lambda r, a, kind=kind: literal_map(r, a, depth_map, kind))
    ms = {k: [] for k in forms}
    for rep in range(warmup + repeats):
        for name, fn in forms.items():  # the forms alternate inside every repeat
            t = timed(fn)
            if rep >= warmup:
                ms[name].append(t)
    rows = {k: summary(v) for k, v in ms.items()}
    for k in list(rows):
        if k.endswith("_fused"):
            rows[k]["torch_over_fused"] = round(rows[k[:-6] + "_torch"]["median_ms"] / rows[k]["median_ms"], 2)
    return dict(width=W, height=H, channels=4, points=M, note="each run includes the clones that make the two leaves (leaf_clones_only)",
                forward_backward=rows)


def time_train(cfg, dev, train_steps, repeats, with_depth):
    W, H, n = cfg.width, cfg.height, cfg.n_gaussians
    scene = {k: t.to(dev) for k, t in syn.make_scene(cfg).items()}
    gen = torch.Generator().manual_seed(syn.SH_SEED)
    scene["features_dc"] = ((torch.rand(n, 1, 3, generator=gen) - 0.5) / 0.28209479177387814).to(dev)
    scene["features_rest"] = torch.zeros(n, 0, 3, device=dev)
    vms, K = syn.make_cameras(cfg, n_views=8).to(dev), syn.intrinsics(cfg).to(dev)
    with torch.no_grad():
        image = render_splats(scene, vms[0], K, W, H).clamp(0.0, 1.0)
    settings = {"without_depth_fn": {}}
    if with_depth:
        points = (torch.rand(2000, 2, generator=gen) * torch.tensor([W - 1.0, H - 1.0])).to(dev)
        depths = (0.5 + 7.5 * torch.rand(2000, generator=gen)).to(dev)
        settings["with_depth_fn"] = dict(depth_fn=lambda v: (points, depths))

    def run(steps, **kw):
        torch.cuda.synchronize()
        t0 = time.time()
        gsbp_amd.train_scene(scene, vms, K, W, H, lambda v: image, steps, seed=1, **kw)
        torch.cuda.synchronize()
        return (time.time() - t0) * 1e3

    rows = {k: [] for k in settings}
    for _ in range(repeats):
        for label, kw in settings.items():
            run(2, **kw)  # (warm: code objects, workspaces)
            short = run(2, **kw)
            long = run(2 + train_steps, **kw)
            rows[label].append(round((long - short) / train_steps, 3))
            print(label, rows[label], flush=True)
    return dict(config=cfg.name if hasattr(cfg, "name") else None, gaussians=n, width=W, height=H, steps=train_steps,
                step_ms={k: dict(median=round(statistics.median(v), 3), min=min(v), max=max(v), runs=v) for k, v in rows.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1060)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="C2")
    ap.add_argument("--train-steps", type=int, default=8, help="steps whose time is measured (0: skip the train_scene part)")
    ap.add_argument("--train-repeats", type=int, default=6, help="measurements per setting; median, min and max are reported")
    ap.add_argument("--train-only", action="store_true", help="only the train_scene step without depth_fn (runs on the parent commit too)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_depth_loss.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0))
    if not a.train_only:
        result["losses"] = time_losses(dev, a.width, a.height, a.points, a.repeats, a.warmup)
        print(json.dumps(result["losses"]), flush=True)
    if a.train_steps > 0:
        result["train_step"] = time_train(syn.CONFIGS[a.config], dev, a.train_steps, a.train_repeats, not a.train_only)
    line = json.dumps(result, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
