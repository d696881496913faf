#!/usr/bin/env python3
"""Densification at full size (C2 geometry: 1 000 000 Gaussians, 1600 x 1060, SH degree 3) in one run on one device, the forms of each
comparison alternating inside every repeat:

  step_fixed       polish_scene's training step: render -> photometric_loss -> backward -> Adam step
  step_densify     the same step with means2d_grad=True and DensifyState.update behind the backward (what train_scene runs)
  round_kernels    one densify() round: plan + emit + gather of the six parameters and their Adam moments, its one host read included
  round_torch      the literal two steps of tests/densify_ref.py ported to device tensors: duplicate, split, prune with boolean masks,
                   index_select and cat over the same parameters and moments, as gsplat's strategy runs them

    timeout -k 10 900 python tools/time_densify.py --out profiles/densify.json

Each form is timed between one pair of hip events around work that ends in a synchronise; ms is the median over --repeats.  peak_mib is
torch.cuda.max_memory_allocated over the form, above what was allocated before it.  Also recorded: the share of split rows whose mean
is not bit-equal to the numpy restatement (the device's expf against the once-rounded exponential) with the largest error over the
bound, and PSNR after equal steps of train_scene and of polish_scene on T1 from every second Gaussian (recorded, not asserted).
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
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402
from gsbp_amd.densify import emit, plan  # noqa: E402
from gsbp_amd.polish import DEFAULT_LRS, PARAM_KEYS, render_splats  # noqa: E402

import densify_ref as ref  # noqa: E402

KEYS = ("means", "scaling", "rotation", "opacity", "features_dc", "features_rest")


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


def make_splats(cfg, dev, degree=3, stride=1):
    s = {k: t[::stride].contiguous().to(dev) for k, t in syn.make_scene(cfg).items()}
    n = s["means"].shape[0]
    gen = torch.Generator().manual_seed(syn.SH_SEED)
    s["features_dc"] = ((torch.rand(n, 1, 3, generator=gen) - 0.5) / 0.28209479177387814).to(dev)
    s["features_rest"] = (0.05 * torch.randn(n, (degree + 1) ** 2 - 1, 3, generator=gen)).to(dev)
    return s


def optimizer_of(work):
    return torch.optim.Adam([dict(params=[work[PARAM_KEYS[name]]], lr=DEFAULT_LRS[name]) for name in PARAM_KEYS], eps=1e-15)


def literal_torch(tables, moments, grad2d, count, th, prune_big, noise):
    """gsplat's duplicate -> split -> prune on device tensors (densify_ref.literal_two_steps), every parameter and both of its Adam
    moments moved by index_select and cat at each of the three steps."""
    t_grad, t_small, t_big, t_opa, log16 = th
    g = grad2d / count.clamp_min(1)
    high = g > t_grad
    small = tables["scaling"].max(dim=1).values <= t_small
    sel = torch.where(high & small)[0]
    tables = {k: torch.cat([v, v[sel]]) for k, v in tables.items()}
    moments = {k: [torch.cat([m, torch.zeros((len(sel),) + tuple(m.shape[1:]), device=m.device)]) for m in ms] for k, ms in moments.items()}
    is_split = torch.cat([high & ~small, torch.zeros(len(sel), dtype=torch.bool, device=high.device)])
    sel, rest = torch.where(is_split)[0], torch.where(~is_split)[0]
    q = torch.nn.functional.normalize(tables["rotation"][sel], dim=1)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    scales = torch.exp(tables["scaling"][sel])
    samples = torch.einsum("nij,nj,bnj->bni", R, scales, noise[sel].transpose(0, 1))
    new = {}
    for k, v in tables.items():
        if k == "means":
            kids = (v[sel] + samples).reshape(-1, 3)
        elif k == "scaling":
            kids = (v[sel] - log16).repeat(2, 1)
        else:
            kids = v[sel].repeat(2, *[1] * (v.dim() - 1))
        new[k] = torch.cat([v[rest], kids])
    moments = {k: [torch.cat([m[rest], torch.zeros((2 * len(sel),) + tuple(m.shape[1:]), device=m.device)]) for m in ms]
               for k, ms in moments.items()}
    prune = new["opacity"] < t_opa
    if prune_big:
        prune = prune | (new["scaling"].max(dim=1).values > t_big)
    keep = torch.where(~prune)[0]
    return {k: v[keep] for k, v in new.items()}, {k: [m[keep] for m in ms] for k, ms in moments.items()}


def split_share(dev, n=100_000, seed=3):
    """The share of split rows whose mean is not the numpy restatement's bits, and the largest error over the float64 bound."""
    r = np.random.default_rng(seed)
    scaling, opacity = ref.f32(math.log(0.05) + 0.7 * r.normal(size=(n, 3))), ref.f32(2.0 * r.normal(size=n))
    means, rotation, noise = ref.f32(r.normal(size=(n, 3)) * 2.0), ref.f32(r.normal(size=(n, 4))), ref.f32(r.normal(size=(n, 2, 3)))
    ones = np.ones(n, np.float32)
    log16 = float(np.float32(math.log(1.6)))
    th = (0.5, -math.inf, math.inf, -math.inf, log16)  # everybody splits
    d = [torch.from_numpy(a).to(dev) for a in (ones, ones, scaling, opacity, means, rotation, noise)]
    kind, offsets = plan(d[0], d[1], d[2], d[3], th, False)
    new = emit(kind, offsets, 2 * n, d[4], d[2], d[5], d[3], d[6], log16)
    got = new["means"].cpu().numpy().reshape(n, 2, 3)
    rows = 0
    same = 0
    worst = 0.0
    for c in range(2):
        want = ref.split_means(means, scaling, rotation, noise[:, c])
        m64 = ref.split_means(means, scaling, rotation, noise[:, c], dtype=np.float64)
        same += int((got[:, c].view(np.uint32) == want.view(np.uint32)).all(axis=1).sum())
        rows += n
        worst = max(worst, float((np.abs(got[:, c].astype(np.float64) - m64) / ref.split_bound(means, scaling, noise[:, c])).max()))
    return dict(split_rows=rows, bit_equal=same, share_not_bit_equal=round(1.0 - same / rows, 6), largest_error_over_bound=round(worst, 4))


def growth_against_fixed(dev, name="T1", steps=200):
    """PSNR after `steps` steps of train_scene and of polish_scene from every second Gaussian of a seeded scene (its own renders as
    the targets): whether growing the set beats touching up the fixed one.  Recorded, not asserted."""
    cfg = syn.CONFIGS[name]
    full = make_splats(cfg, dev, degree=0)
    K, vms = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg).to(dev)
    with torch.no_grad():
        images = [render_splats(full, vms[v], K, cfg.width, cfg.height).clamp(0.0, 1.0) for v in range(vms.shape[0])]
    start = {k: t[::2].contiguous() for k, t in full.items()}
    before = gsbp_amd.score_image_views(start, vms, K, cfg.width, cfg.height, lambda v: images[v])["mean"]["psnr"]
    dcfg = gsbp_amd.DensifyConfig(refine_start_iter=20, refine_every=20, grow_scale3d=cfg.log_scale0, prune_scale3d=10 * cfg.log_scale0)
    grown, hist = gsbp_amd.train_scene(start, vms, K, cfg.width, cfg.height, lambda v: images[v], steps, dcfg)
    fixed, _ = gsbp_amd.polish_scene(start, vms, K, cfg.width, cfg.height, lambda v: images[v], params=tuple(PARAM_KEYS), steps=steps)
    score = lambda s: gsbp_amd.score_image_views(s, vms, K, cfg.width, cfg.height, lambda v: images[v])["mean"]["psnr"]  # noqa: E731
    return dict(config=name, steps=steps, n_start=start["means"].shape[0], n_trained=grown["means"].shape[0], rounds=len(hist["rounds"]),
                psnr_start=round(before, 3), psnr_train_scene=round(score(grown), 3), psnr_polish_scene=round(score(fixed), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_densify.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    W, H = cfg.width, cfg.height
    K, vms = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg, n_views=2).to(dev)
    full = make_splats(cfg, dev)
    n = full["means"].shape[0]
    with torch.no_grad():
        images = [render_splats(full, vms[v], K, W, H).clamp(0.0, 1.0) for v in range(2)]
    gen = torch.Generator().manual_seed(11)
    work = {k: (t + 0.01 * torch.randn(t.shape, generator=gen).to(dev)).requires_grad_(True) for k, t in full.items()}
    opt = optimizer_of(work)
    state = gsbp_amd.DensifyState(n, dev)

    def step(densify_on, v):
        opt.zero_grad(set_to_none=True)
        if densify_on:
            image, meta = render_splats(work, vms[v], K, W, H, return_meta=True, means2d_grad=True)
        else:
            image = render_splats(work, vms[v], K, W, H)
        gsbp_amd.photometric_loss(image, images[v]).backward()
        if densify_on:
            state.update(meta)
        opt.step()

    ms = {k: [] for k in ("step_fixed", "step_densify", "round_kernels", "round_torch")}
    peak = {k: 0.0 for k in ms}
    for rep in range(a.repeats + a.warmup):
        for name in ("step_fixed", "step_densify"):
            _, t, p = timed(lambda: step(name == "step_densify", rep % 2))
            if rep >= a.warmup:
                ms[name].append(t)
                peak[name] = max(peak[name], p)
    # one round on the statistics those steps left, with thresholds at the data's medians (everything happens), both forms on copies
    seen = state.count > 0
    grow = float(torch.median((state.grad2d / state.count.clamp_min(1))[seen]))
    m = work["scaling"].detach().max(dim=1).values
    dcfg = gsbp_amd.DensifyConfig(grow_grad2d=grow, grow_scale3d=float(torch.exp(torch.median(m))), prune_scale3d=float(torch.exp(torch.quantile(m[::16], 0.9))),
                                  prune_opa=float(torch.quantile(torch.sigmoid(work["opacity"].detach()[::16]), 0.1)))
    th = dcfg.thresholds()
    step_no = dcfg.reset_every + 100
    noise = torch.randn(n, 2, 3, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    grad2d, count = state.grad2d.clone(), state.count.clone()
    sizes = {}
    for rep in range(a.repeats + a.warmup):
        for name in ("round_kernels", "round_torch"):
            params = {k: work[k].detach().clone().requires_grad_(True) for k in KEYS}
            o = optimizer_of(params)
            for k in KEYS:  # the moments the steps above left, copied: every repeat starts from the same optimiser state
                o.state[params[k]] = {kk: vv.clone() for kk, vv in opt.state[work[k]].items()}
            st = gsbp_amd.DensifyState(n, dev)
            st.grad2d, st.count = grad2d.clone(), count.clone()
            if name == "round_kernels":
                (new, info), t, p = timed(lambda: gsbp_amd.densify(params, st, dcfg, step_no, optimizer=o,
                                                                   generator=torch.Generator(device=dev).manual_seed(5)))
                sizes[name] = info["n_after"]
                counts = {k: info[k] for k in ("pruned", "kept", "cloned", "split")}
            else:
                tables = {k: params[k].detach() for k in KEYS}
                moments = {k: [o.state[params[k]]["exp_avg"], o.state[params[k]]["exp_avg_sq"]] for k in KEYS}
                (new, _), t, p = timed(lambda: literal_torch(tables, moments, st.grad2d, st.count, th, True, noise))
                sizes[name] = new["means"].shape[0]
            if rep >= a.warmup:
                ms[name].append(t)
                peak[name] = max(peak[name], p)
            del new, params, o, st
    assert sizes["round_kernels"] == sizes["round_torch"], sizes  # a timing of a wrong result is no timing
    timing = dict(tool="tools/time_densify.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), config=a.config,
                  n_gaussians=n, width=W, height=H, sh_degree=3, repeats=a.repeats, warmup=a.warmup, round=dict(counts, n_after=sizes["round_kernels"]),
                  forms={})
    for name, ts in ms.items():
        timing["forms"][name] = dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                                     peak_mib=round(peak[name], 1))
        print(name, json.dumps(timing["forms"][name]), flush=True)
    f = timing["forms"]
    timing["step_densify_over_step_fixed"] = round(f["step_densify"]["median_ms"] / f["step_fixed"]["median_ms"], 4)
    timing["round_torch_over_round_kernels"] = round(f["round_torch"]["median_ms"] / f["round_kernels"]["median_ms"], 3)
    del work, opt, state, full, images
    torch.cuda.empty_cache()
    timing["split_means"] = split_share(dev)
    timing["growth_against_fixed"] = growth_against_fixed(dev)
    print("timing", json.dumps({k: v for k, v in timing.items() if k != "forms"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(timing, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
