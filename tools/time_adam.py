#!/usr/bin/env python3
"""The optimiser step of training at full size (C2 geometry: 1 000 000 Gaussians, SH degree 3) in one run on one device, the forms of
each comparison alternating inside every repeat.  Two cases: the six splat tables (59 floats per Gaussian), and the same with an
[N, 128] latent table (187 floats).

  torch            torch.optim.Adam as polish.trainable builds it (one tensor per group, eps 1e-15): torch's multi-tensor route
  torch_fused      torch.optim.Adam(fused=True) over the same groups: the yardstick of the dense kernel
  splat_dense      SplatAdam.step(): k_adam_step once per table, no mask
  splat_view       SplatAdam.step(visible=radii of a C2 view); the view's visible share is recorded
  splat_runs_25, splat_runs_50, splat_scatter_25, splat_scatter_50
                   SplatAdam under synthetic masks of 25 % and 50 % visible rows: runs of 4096 rows, or a seeded random scatter

  per_width        k_adam_step alone on one [N, w] table, w in 1, 3, 4, 45, 128, under each of the masks above (50 launches per timing):
                   whether skipping rows saves traffic at that width ("none": a mask of zeros, the price of a launch and the mask)
  train_step       one gsbp_amd.train_scene step under adam = "torch", "fused", "visible", with and without the feature term, from
                   the difference of a long and a short call

    timeout -k 10 900 python tools/time_adam.py --out profiles/adam.json

Each form is timed between one pair of hip events around work that ends in a synchronise; ms is the median over --repeats, with min and
max.  Beside each figure stands its byte floor at 6.29 TB/s: 28 B per float of a stepped row (p, g, m, v read; p, m, v written) plus one
mask byte per row and table; for a masked form that is the floor of an ideal kernel that moves no byte of an invisible row.  Nothing is
asserted on the timings; the forms' results are compared before they are timed (a timing of a wrong result is no timing).
"""
import argparse
import ctypes as C
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
from gsbp_amd import _lib  # noqa: E402
from gsbp_amd._lib import ptr  # noqa: E402
from gsbp_amd.polish import DEFAULT_LRS, PARAM_KEYS, render_splats  # noqa: E402
from gsbp_amd.rasterization import release_engines  # noqa: E402

HBM_TBPS = 6.29
WIDTHS = (1, 3, 4, 45, 128)
RUN = 4096


def timed(fn):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def summary(ts, floor_bytes):
    floor_ms = floor_bytes / (HBM_TBPS * 1e12) * 1e3
    med = statistics.median(ts)
    return dict(median_ms=round(med, 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), floor_ms=round(floor_ms, 4),
                over_floor=round(med / floor_ms, 3))


def make_masks(n, dev, radii):
    rows = torch.arange(n, device=dev)
    gen = torch.Generator().manual_seed(5)
    u = torch.rand(n, generator=gen).to(dev)
    return dict(view=(radii > 0).any(0).contiguous(), runs_25=(rows // RUN) % 4 == 0, runs_50=(rows // RUN) % 2 == 0,
                scatter_25=u < 0.25, scatter_50=u < 0.5)


def tables_of(n, dev, with_latents):
    shapes = dict(means=(3,), scaling=(3,), rotation=(4,), opacity=(), features_dc=(1, 3), features_rest=(15, 3))
    lrs = {PARAM_KEYS[name]: lr for name, lr in DEFAULT_LRS.items()}
    if with_latents:
        shapes["features"], lrs["features"] = (128,), 2.5e-3
    gen = torch.Generator().manual_seed(3)
    start = {k: torch.randn((n,) + tail, generator=gen).to(dev) for k, tail in shapes.items()}
    grads = {k: (1e-3 * torch.randn((n,) + tail, generator=gen)).to(dev) for k, tail in shapes.items()}
    return start, grads, lrs


def optimiser(cls, start, grads, lrs, **kw):
    params = {k: t.clone().requires_grad_(True) for k, t in start.items()}
    for k, p in params.items():
        p.grad = grads[k]
    return params, cls([dict(params=[params[k]], lr=lrs[k]) for k in params], eps=1e-15, **kw)


def time_case(n, dev, with_latents, masks, repeats, warmup):
    start, grads, lrs = tables_of(n, dev, with_latents)
    floats = sum(t[0].numel() for t in start.values())
    sets = dict(torch=optimiser(torch.optim.Adam, start, grads, lrs), torch_fused=optimiser(torch.optim.Adam, start, grads, lrs, fused=True),
                splat=optimiser(gsbp_amd.SplatAdam, start, grads, lrs))
    # one step of each from the same start: the three must agree before any is timed
    for params, opt in sets.values():
        opt.step()
    for k in start:
        want = sets["torch"][0][k].detach()
        for name in ("torch_fused", "splat"):
            err = float((sets[name][0][k].detach() - want).abs().max())
            assert err <= 1e-6 * float(want.abs().max()), f"{name} and torch.optim.Adam disagree on {k}: {err}"
    splat = sets["splat"][1]
    forms = dict(torch=sets["torch"][1].step, torch_fused=sets["torch_fused"][1].step, splat_dense=splat.step)
    for name, mask in masks.items():
        forms["splat_" + name] = (lambda m: lambda: splat.step(visible=m))(mask)
    ms = {name: [] for name in forms}
    for rep in range(repeats + warmup):
        for name, fn in forms.items():
            t = timed(fn)
            if rep >= warmup:
                ms[name].append(t)
    out = dict(floats_per_gaussian=floats, tables=len(start), forms={})
    for name, ts in ms.items():
        mask = masks.get(name[len("splat_"):]) if name.startswith("splat_") else None
        seen = n if mask is None else int(mask.sum())
        out["forms"][name] = summary(ts, 28 * floats * seen + (0 if mask is None else n * len(start)))
        print(("187" if with_latents else "59"), name, json.dumps(out["forms"][name]), flush=True)
    f = out["forms"]
    out["splat_dense_over_torch_fused"] = round(f["splat_dense"]["median_ms"] / f["torch_fused"]["median_ms"], 3)
    out["splat_dense_over_torch"] = round(f["splat_dense"]["median_ms"] / f["torch"]["median_ms"], 3)
    return out


def time_widths(n, dev, masks, repeats, warmup, inner=50):
    """(the C entry point called directly with prepared arguments: at w <= 4 a launch is as long as the kernel, and the form "none", a
    mask of zeros, is the price of a launch that reads the mask and nothing else)"""
    fn = _lib.lib().gwbp_adam_step
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator().manual_seed(7)
    rows = {}
    for w in WIDTHS:
        p, m = torch.randn(n, w, generator=gen).to(dev), torch.zeros(n, w, device=dev)
        g, v = (1e-3 * torch.randn(n, w, generator=gen)).to(dev), torch.zeros(n, w, device=dev)
        forms = dict(dense=None, **masks, none=torch.zeros(n, dtype=torch.bool, device=dev))
        ms = {name: [] for name in forms}
        for rep in range(repeats + warmup):
            for name, mask in forms.items():
                args = (C.c_int64(n), w, ptr(p), ptr(g), ptr(m), ptr(v), ptr(mask), C.c_float(1e-3), C.c_float(0.0316), C.c_double(0.9),
                        C.c_double(0.999), C.c_float(1e-15), stream)

                def launches():
                    for _ in range(inner):
                        _lib.check(fn(*args), "gwbp_adam_step")
                t = timed(launches) / inner
                if rep >= warmup:
                    ms[name].append(t)
        rows[str(w)] = {name: summary(ts, 28 * w * (n if forms[name] is None else int(forms[name].sum())) + (0 if forms[name] is None else n))
                        for name, ts in ms.items()}
        for name in forms:
            rows[str(w)][name]["over_dense"] = round(rows[str(w)][name]["median_ms"] / rows[str(w)]["dense"]["median_ms"], 3)
        print("width", w, json.dumps({k: (r["median_ms"], r["over_dense"]) for k, r in rows[str(w)].items()}), flush=True)
    return rows


def time_train(cfg, dev, train_steps, feature_dim):
    W, H, n = cfg.width, cfg.height, cfg.n_gaussians
    scene = {k: t.to(dev) for k, t in syn.make_scene(cfg).items()}
    gen = torch.Generator().manual_seed(syn.SH_SEED)
    scene["features_dc"] = ((torch.rand(n, 1, 3, generator=gen) - 0.5) / 0.28209479177387814).to(dev)
    scene["features_rest"] = (0.05 * torch.randn(n, 15, 3, generator=gen)).to(dev)
    vms, K = syn.make_cameras(cfg, n_views=8).to(dev), syn.intrinsics(cfg).to(dev)
    with torch.no_grad():
        image = render_splats(scene, vms[0], K, W, H).clamp(0.0, 1.0)
    fmap = torch.rand(H, W, feature_dim, generator=gen).to(dev)

    def run(steps, **kw):
        torch.cuda.synchronize()
        t0 = time.time()
        gsbp_amd.train_scene(scene, vms, K, W, H, lambda v: image, steps, seed=1, **kw)
        torch.cuda.synchronize()
        return (time.time() - t0) * 1e3

    feature = dict(feature_fn=lambda v: fmap, feature_dim=feature_dim, latent_dim=128)
    rows = {}
    for label, extra in (("colour_only", {}), ("with_feature_term", feature)):
        for rnd in range(2):  # each setting twice, the three alternating
            for adam in ("torch", "fused", "visible"):
                kw = dict(extra, adam=adam)
                run(2, **kw)  # (warm: code objects, workspaces)
                short = run(2, **kw)
                long = run(2 + train_steps, **kw)
                rows.setdefault(f"{label}_{adam}", []).append(round((long - short) / train_steps, 3))
                print(label, adam, rows[f"{label}_{adam}"], flush=True)
    return dict(steps=train_steps, feature_dim=feature_dim, latent_dim=128, sh_degree=3, step_ms=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--train-steps", type=int, default=8, help="steps whose time is measured (0: skip the train_scene part)")
    ap.add_argument("--feature-dim", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_adam.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    n = cfg.n_gaussians
    full = {k: t.contiguous().to(dev) for k, t in syn.make_scene(cfg).items()}
    full["features_dc"], full["features_rest"] = torch.zeros(n, 1, 3, device=dev), torch.zeros(n, 0, 3, device=dev)
    vm, K = syn.make_cameras(cfg, n_views=1).to(dev)[0], syn.intrinsics(cfg).to(dev)
    _, meta = render_splats(full, vm, K, cfg.width, cfg.height, return_meta=True, means2d_grad=True)
    radii = meta["radii"].clone()
    del meta, full
    release_engines(dev)
    masks = make_masks(n, dev, radii)
    res = dict(tool="tools/time_adam.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), config=a.config,
               n_gaussians=n, repeats=a.repeats, warmup=a.warmup, hbm_tb_per_s=HBM_TBPS, run_rows=RUN,
               visible_share={name: round(float(m.float().mean()), 4) for name, m in masks.items()})
    print("visible", json.dumps(res["visible_share"]), flush=True)
    res["splat_tables"] = time_case(n, dev, False, masks, a.repeats, a.warmup)
    torch.cuda.empty_cache()
    res["splat_and_latent_tables"] = time_case(n, dev, True, masks, a.repeats, a.warmup)
    torch.cuda.empty_cache()
    res["per_width"] = time_widths(n, dev, masks, a.repeats, a.warmup)
    torch.cuda.empty_cache()
    if a.train_steps > 0:
        res["train_step"] = time_train(cfg, dev, a.train_steps, a.feature_dim)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
