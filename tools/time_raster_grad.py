#!/usr/bin/env python3
"""The geometry gradients of rasterization() at full size (C2 geometry: 1 M Gaussians, 1600 x 1060), D = 3 and D = 16, and the error
figures of tests/test_gpu_raster_grad.py, in one run on one device:

  render_pixels            gwbp_render_pixels on the projected and sorted view (the forward the backward is compared with)
  render_pixels_backward   gwbp_render_pixels_backward: k_render_px_bwd with v_out, v_alpha, v_colors and v_g2d
  project_torch            projection.project_torch forward + torch.autograd.grad to means / quats / scales / opacities on the
                           visible rows, in float64: the chain rasterization()'s backward ran before it had a kernel for it
  project_backward         gwbp_project_backward (k_project_bwd) on the same v_g2d: the four per-Gaussian gradients
  project_backward_viewmat the same call with want_viewmat: + the 12 view sums (k_project_bwd_sum)
  errors                   per case and gradient tensor of the test file: the float32 restatement's error against float64 (the
                           floor) and the kernel path's, Frobenius-relative and max-abs relative to the truth's max-abs

    timeout -k 10 900 python tools/time_raster_grad.py --out profiles/raster_grad.json --project-out profiles/project_backward.json

--project-out: the projection backward by itself -- its two timings against project_torch's from this run, the kernel-alone errors
against float64 autograd and the six-tensor error rows of tests/test_gpu_camera_grad.py, and what the pose refiner reaches on that
file's case: the float64 dense yardstick on the CPU and refine_pose on the device, under the same Adam loop.

Each view is projected and sorted once; every form is then timed between one pair of hip events, and ms is the median over --views
views.  ratio_backward_over_forward is the backward's median over the forward's, as measured: no bound is set on it.  peak_mib is
torch.cuda.max_memory_allocated over the timed backward + chain of a view, above what was allocated before it.
"""
import argparse
import json
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
from gsbp_amd.projection import project_torch  # noqa: E402
from gsbp_amd.rasterization import get_engine  # noqa: E402

DIMS = (3, 16)
FORMS = ("render_pixels", "render_pixels_backward", "project_torch", "project_backward", "project_backward_viewmat")


def _rounded(rows):
    return [{k: (float(f"{x:.3e}") if isinstance(x, float) else x) for k, x in r.items()} for r in rows]


def project_report(dev, res):
    """The projection backward by itself: timings out of `res`, the kernel alone against float64 autograd, rasterization(camera_grad=
    True) against the six-tensor yardstick, and the refiner."""
    import camera_grad_ref as cg  # noqa: E402
    import test_gpu_camera_grad as cam  # noqa: E402  (the test file's cases and its two sides)
    out = dict(tool=res["tool"], device=res["device"], date=res["date"], config=res["config"], n_gaussians=res["n_gaussians"],
               views=res["views"], warmup=res["warmup"], timing={}, kernel_alone=[], errors=[])
    for D, row in res["forms"].items():
        out["timing"][D] = {k: row[k] for k in ("project_torch", "project_backward", "project_backward_viewmat")}
        out["timing"][D]["speedup_over_project_torch"] = round(row["project_torch"]["median_ms"] / row["project_backward"]["median_ms"], 1)
    for model in ("pinhole", "ortho", "fisheye"):
        for mode in ("classic", "antialiased"):
            sc = cg.scene(model)
            v_g2d = cg.random_v_g2d(sc["inputs"][0].shape[0])
            (got,), vis, eps2d = cam.project_and_backward(dev, sc, model, mode, v_g2d)
            fig = cam.against_autograd(sc, model, mode, got, vis, eps2d, v_g2d, f"{model} {mode}")
            out["kernel_alone"].append(dict(camera_model=model, rasterize_mode=mode, visible=int(vis.sum()),
                                            **{k: float(f"{x:.3e}") for k, x in fig.items()}))
    out["bounds"] = dict(viewmat=cam.BOUND_VIEW, per_gaussian=cam.BOUND_ROW, factor=cam.FACTOR)
    for name in cam.CASES:
        out["errors"] += _rounded(cam.run_case(dev, name)[0])
    case = cg.pose_case()
    ref, got = cg.yardstick_refine(case), cam.gpu_refine(dev, case)
    names = ("loss", "angle", "distance")
    out["refine_pose"] = dict(twist0=list(cg.POSE_TWIST0), lr=cg.POSE_LR, steps=cg.POSE_STEPS,
                              start=dict(zip(("angle_rad", "distance"), cam.pose_error(case["vm0"], case["vm_true"]))),
                              factors_yardstick_float64=dict(zip(names, (round(x, 5) for x in cg.pose_factors(ref, case)))),
                              factors_kernels=dict(zip(names, (round(x, 5) for x in cg.pose_factors(got, case)))))
    print("refine_pose", json.dumps(out["refine_pose"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-errors", action="store_true", help="skip the test file's error figures")
    ap.add_argument("--out", default=None)
    ap.add_argument("--project-out", default=None, help="write the projection backward's figures here (see above)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_raster_grad.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    W, H, n = cfg.width, cfg.height, cfg.n_gaussians
    gauss = tuple(t.to(dev).contiguous() for t in syn.activate(syn.make_scene(cfg)))
    vms, K = syn.make_cameras(cfg, n_views=a.views + a.warmup), syn.intrinsics(cfg)
    eng = get_engine(dev, n, W, H)
    g = torch.Generator().manual_seed(1)
    tables = {D: torch.rand(n, D, generator=g).to(dev) for D in DIMS}
    v_outs = {D: torch.randn(H, W, D, generator=g).to(dev) for D in DIMS}
    v_alpha = torch.randn(H, W, generator=g).to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    def front(v):
        for _ in range(6):
            view = eng.view(vms[v], K, W, H)
            proj = eng.project(view, *gauss, want_outputs=True)
            eng.bin_sort(view)
            stats = eng.stats()
            if not stats["overflow"]:
                return view, proj["radii"] > 0, stats
            eng.grow(stats, views=1)
        raise SystemExit("the workspace kept overflowing")

    def chain(view, visible, v_g2d):
        ins = [t.detach().double().requires_grad_(True) for t in gauss]
        out = project_torch(*ins, vms[0].new_tensor(list(view.viewmat)).reshape(4, 4), K, W, H, float(view.eps2d), "pinhole",
                            "classic", visible)
        v = v_g2d.double()
        return torch.autograd.grad(out, ins, (v[:, :2], v[:, 2:5], v[:, 5]))

    ms, peak, isect = {}, {D: 0.0 for D in DIMS}, []
    for v in range(a.views + a.warmup):
        view, visible, stats = front(v)
        for D in DIMS:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t_f, _ = timed(lambda: eng.render_pixels(view, tables[D]))
            t_b, (_, v_g2d) = timed(lambda: eng.render_pixels_backward(view, tables[D], v_outs[D], v_alpha))
            t_c, _ = timed(lambda: chain(view, visible, v_g2d))
            t_p, _ = timed(lambda: eng.project_backward(view, *gauss, v_g2d))
            t_v, _ = timed(lambda: eng.project_backward(view, *gauss, v_g2d, want_viewmat=True))
            if v >= a.warmup:
                for name, t in (("render_pixels", t_f), ("render_pixels_backward", t_b), ("project_torch", t_c),
                                ("project_backward", t_p), ("project_backward_viewmat", t_v)):
                    ms.setdefault((name, D), []).append(t)
                peak[D] = max(peak[D], (torch.cuda.max_memory_allocated() - base) / 2 ** 20)
        if v >= a.warmup:
            isect.append(stats["n_isect"])
    res = dict(tool="tools/time_raster_grad.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), config=a.config,
               n_gaussians=n, width=W, height=H, views=a.views, warmup=a.warmup, median_intersections=int(statistics.median(isect)),
               forms={}, errors=[])
    for D in DIMS:
        row = {}
        for name in FORMS:
            ts = ms[(name, D)]
            row[name] = dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))
        row["ratio_backward_over_forward"] = round(row["render_pixels_backward"]["median_ms"] / row["render_pixels"]["median_ms"], 3)
        row["peak_mib"] = round(peak[D], 1)
        res["forms"][f"D{D}"] = row
        print(f"D{D}", json.dumps(row), flush=True)
    if not a.no_errors:
        import test_gpu_raster_grad as cases  # noqa: E402  (the test file's scenes and its two sides)
        for name in cases.CASES:
            rows, _ = cases.run_case(dev, name)
            res["errors"] += _rounded(rows)
        worst = max(res["errors"], key=lambda r: max(r["kernel_fro"] / max(r["floor_fro"], 1e-300),
                                                     r["kernel_max"] / max(r["floor_max"], 1e-300)))
        res["bound_factor"], res["worst"] = cases.FACTOR, worst
        print("worst", json.dumps(worst))
        for kind in ("fro", "max"):  # kernel / floor over every case and tensor
            ratios = [r[f"kernel_{kind}"] / max(r[f"floor_{kind}"], 1e-300) for r in res["errors"]]
            res[f"ratio_{kind}"] = dict(median=round(statistics.median(ratios), 3), largest=round(max(ratios), 3))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)
    if a.project_out:
        proj = project_report(dev, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.project_out)), exist_ok=True)
        with open(a.project_out, "w") as f:
            json.dump(proj, f, indent=1)
        print("wrote", a.project_out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
