#!/usr/bin/env python3
"""The geometry backward of a 128-channel latent render at full size (C2 geometry: 1 M Gaussians, 1600 x 1060), in one run on one device:

  dots                gwbp_render_dots_backward (k_render_dots_bwd): v_g2d of the whole table in one call
  sliced              the route there was before it: four gwbp_render_pixels_backward calls on 32-channel slices of the table and of
                      v_out (want_colors=False, v_alpha with the first), summed; the slices of v_out are cut outside the timed span
  pieces              what else a step's feature term runs: the front with the weight store (project + bin_sort + blend_weights), the
                      wide render, the scatter of v_out into the table's gradient, the projection backward, and decoded_loss forward
                      + backward on the rendered map (--feature-dim channels)
  train_step          one gsbp_amd.train_scene step with and without the feature term (latent_dim 128, --feature-dim channels), from
                      the difference of two runs of different length, and the peak memory of each

    timeout -k 10 1100 python tools/time_latent_grad.py --out profiles/latent_grad.json

The two forms are timed alternately on every view between one pair of hip events each; median, min and max over --views views
(at least 6).  wins = the slowest dots call is faster than the fastest sliced one.  fma_floor_ms = pairs x D FMAs over the chip's
f32 FMA peak (256 CUs x 128 lanes x 2.4 GHz); byte_floor_ms = the bytes the kernel cannot avoid -- v_out once, a colour row and a
record per tile intersection, v_g2d -- over 6.29 TB/s.
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
from gsbp_amd.rasterization import get_engine, release_engines  # noqa: E402

D = 128
FMA_PER_S = 256 * 128 * 2.4e9
BYTES_PER_S = 6.29e12  # the copy rate the other records of this directory divide by


def summary(xs):
    return dict(median_ms=round(statistics.median(xs), 3), min_ms=round(min(xs), 3), max_ms=round(max(xs), 3), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--feature-dim", type=int, default=512)
    ap.add_argument("--train-steps", type=int, default=8, help="steps whose time is measured (0: skip the train_scene part)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_latent_grad.py measures on a GPU; there is nothing to report without one")
    if a.views < 6:
        raise SystemExit("--views must be at least 6")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    W, H, n = cfg.width, cfg.height, cfg.n_gaussians
    scene = {k: t.to(dev) for k, t in syn.make_scene(cfg).items()}
    gauss = tuple(t.to(dev).contiguous() for t in syn.activate(syn.make_scene(cfg)))
    vms, K = syn.make_cameras(cfg, n_views=a.views + a.warmup), syn.intrinsics(cfg)
    eng = get_engine(dev, n, W, H)
    g = torch.Generator().manual_seed(1)
    table = torch.rand(n, D, generator=g).to(dev)
    v_out = torch.randn(H, W, D, generator=g).to(dev)
    v_alpha = torch.randn(H, W, generator=g).to(dev)
    slices = [v_out[..., c:c + 32].contiguous() for c in range(0, D, 32)]

    def timed(fn):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    def front(view):
        for _ in range(6):
            eng.project(view, *gauss)
            eng.bin_sort(view)
            eng.blend_weights(view)
            stats = eng.stats()
            if not stats["overflow"]:
                return stats
            eng.grow(stats, views=1)
        raise SystemExit("the workspace kept overflowing")

    def sliced(view):
        total = None
        for k, vo in enumerate(slices):
            _, v = eng.render_pixels_backward(view, table[:, 32 * k:32 * k + 32], vo, v_alpha if k == 0 else None, want_colors=False)
            total = v if total is None else total.add_(v)
        return total

    ms = {k: [] for k in ("dots", "sliced", "front_with_store", "wide_render", "scatter", "project_backward", "decoded_loss")}
    fmap = torch.rand(H, W, a.feature_dim, generator=g).to(dev)
    decoder = torch.rand(D, a.feature_dim, generator=g).to(dev).requires_grad_(True)

    def decode(rendered):
        rendered = rendered.detach().requires_grad_(True)
        gsbp_amd.decoded_loss(rendered, decoder, fmap).backward()
        return rendered.grad
    pairs, isect, agree = [], [], []
    for v in range(a.views + a.warmup):
        view = eng.view(vms[v], K, W, H)
        stats = front(view)
        t_front, _ = timed(lambda: front(view))
        t_render, rendered = timed(lambda: eng.render(view, table))
        t_decode, _ = timed(lambda: decode(rendered))
        del rendered
        acc = torch.zeros(n, D, device=dev)
        t_scatter, _ = timed(lambda: eng.scatter(view, v_out, acc, None))
        order = ("dots", "sliced") if v % 2 == 0 else ("sliced", "dots")
        got = {}
        for name in order:
            t, got[name] = timed((lambda: eng.render_dots_backward(view, table, v_out, v_alpha)) if name == "dots" else (lambda: sliced(view)))
            if v >= a.warmup:
                ms[name].append(t)
        t_proj, _ = timed(lambda: eng.project_backward(view, *gauss, got["dots"]))
        if v >= a.warmup:
            ms["front_with_store"].append(t_front), ms["wide_render"].append(t_render), ms["scatter"].append(t_scatter)
            ms["project_backward"].append(t_proj), ms["decoded_loss"].append(t_decode)
            pairs.append(stats["n_pairs"]), isect.append(stats["n_isect"])
            diff = (got["dots"].double() - got["sliced"].double()).norm(dim=0) / got["sliced"].double().norm(dim=0).clamp_min(1e-300)
            agree.append(float(diff.max()))
        print(f"view {v}: pairs {stats['n_pairs']}, isect {stats['n_isect']}", flush=True)
    res = dict(tool="tools/time_latent_grad.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), config=a.config,
               n_gaussians=n, width=W, height=H, channels=D, views=a.views, warmup=a.warmup,
               forms={k: summary(xs) for k, xs in ms.items()})
    p, i = statistics.median(pairs), statistics.median(isect)
    res["pairs_median"], res["isect_median"] = p, i
    res["fma_floor_ms"] = round(p * D / FMA_PER_S * 1e3, 3)
    res["byte_floor_ms"] = round((H * W * D * 4 + i * (D * 4 + 32 + 4) + n * 24) / BYTES_PER_S * 1e3, 3)
    res["wins"] = res["forms"]["dots"]["max_ms"] < res["forms"]["sliced"]["min_ms"]
    res["speedup_median"] = round(res["forms"]["sliced"]["median_ms"] / res["forms"]["dots"]["median_ms"], 2)
    res["dots_against_sliced_column_error_max"] = float(f"{max(agree):.3e}")  # largest Frobenius-relative difference of a column of v_g2d
    print(json.dumps(res, indent=1), flush=True)

    if a.train_steps > 0:
        del table, v_out, slices, acc, got, decoder
        release_engines(dev)
        torch.cuda.empty_cache()
        gen = torch.Generator().manual_seed(syn.SH_SEED)
        scene["features_dc"] = ((torch.rand(n, 1, 3, generator=gen) - 0.5) / 0.28209479177387814).to(dev)
        scene["features_rest"] = torch.zeros(n, 0, 3, device=dev)
        vm_dev, K_dev = vms[:a.views].to(dev), K.to(dev)
        with torch.no_grad():
            image = gsbp_amd.polish.render_splats(scene, vm_dev[0], K_dev, W, H).clamp(0.0, 1.0)

        def run(steps, **kw):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.time()
            gsbp_amd.train_scene(scene, vm_dev, K_dev, W, H, lambda v: image, steps, seed=1, **kw)
            torch.cuda.synchronize()
            return (time.time() - t0) * 1e3, torch.cuda.max_memory_allocated() / 2 ** 20

        feature = dict(feature_fn=lambda v: fmap, feature_dim=a.feature_dim, latent_dim=D)
        rows = {}
        for name, kw in (("colour_only", {}), ("with_feature_term", feature), ("colour_only_again", {}), ("with_feature_term_again", feature)):
            run(2, **kw)  # (warm: code objects, workspaces)
            short, _ = run(2, **kw)
            long, peak = run(2 + a.train_steps, **kw)
            rows[name] = dict(step_ms=round((long - short) / a.train_steps, 3), peak_mib=round(peak, 1))
            print(name, rows[name], flush=True)
        res["train_step"] = dict(steps=a.train_steps, feature_dim=a.feature_dim, latent_dim=D, **rows,
                                 note="projection and sort run once per render and once more in the backward of the render whose "
                                      "workspace the other has taken: the two renders of a step share one engine")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
