#!/usr/bin/env python3
"""The decode-loss call at full size (C2 geometry: 1600 x 1060, D = 512) beside the literal torch statements it replaces, and one
whole fit_decoded_field step split into its stages, all in one run on one device.

  (a) fused      Engine.decode_loss: loss, d/d(rendered) and d/d(decoder) in one call, no [H, W, D] tensor
  (b) literal    F.l1_loss(rendered @ conv, target) forward + backward in torch (rocBLAS GEMMs, [H, W, D] temporaries)

for d = 128 and d = 16, l1 and l2, the forms alternating call by call; ms is the median over --reps calls after --warmup,
peak_extra_mib the torch.cuda.max_memory_allocated delta of one call, its outputs included.  fp32_pipe_floor_ms is the time of the
call's fused multiply-adds (four products of P d D each for the fused form, three for the literal one) at the fp32 matrix rate
(--tflops).  Then a step of the fit at d = 128 on the C2 scene: front (project, sort, blend), render, decode-loss, scatter, Adam.

    timeout -k 10 1100 python tools/time_decode_loss.py --out profiles/decode_loss.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6, help="fit steps to split (after one warm-up step)")
    ap.add_argument("--tflops", type=float, default=157.3, help="peak fp32 matrix rate")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_decode_loss.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    W, H, n, D = cfg.width, cfg.height, cfg.n_gaussians, cfg.feat_dim
    gauss = tuple(t.to(dev).contiguous() for t in syn.activate(syn.make_scene(cfg)))
    vms, K = syn.make_cameras(cfg, n_views=a.steps + 1), syn.intrinsics(cfg)
    eng = get_engine(dev, n, W, H)
    res = dict(tool="tools/time_decode_loss.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"),
               config=a.config, n_gaussians=n, width=W, height=H, D=D, reps=a.reps, warmup=a.warmup, tflops=a.tflops, rows=[])

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

    g = torch.Generator(device=dev).manual_seed(D)
    target = torch.randn(H, W, D, generator=g, device=dev)
    for d in (128, 16):
        rendered = torch.randn(H, W, d, generator=g, device=dev)
        conv = torch.rand(d, D, generator=g, device=dev)
        eng.decode_loss(rendered, conv, target)  # (the workspace of (d, D) exists from here on)
        for loss in ("l1", "l2"):
            f_lit = torch.nn.functional.l1_loss if loss == "l1" else torch.nn.functional.mse_loss
            scale = 1.0 / (H * W * D)

            def fused():
                return eng.decode_loss(rendered, conv, target, loss=loss, scale=scale)[:3]

            def literal():
                r, c = rendered.detach().requires_grad_(True), conv.detach().requires_grad_(True)
                value = f_lit(r @ c, target)
                value.backward()
                return value.detach(), r.grad, c.grad
            forms = dict(fused=fused, literal=literal)
            ms = {k: [] for k in forms}
            peak, last = {}, {}
            for i in range(a.reps + a.warmup):
                for name in (("fused", "literal") if i % 2 == 0 else ("literal", "fused")):
                    t, mem, out = measure(forms[name])
                    if i >= a.warmup:
                        ms[name].append(t)
                        peak[name] = max(peak.get(name, 0.0), mem)
                    last[name] = out
                    del out
            flop = 2.0 * H * W * d * D
            row = dict(d=d, D=D, loss=loss, pixels=H * W, image_mib=round(H * W * D * 4 / 2 ** 20, 1))
            for name, products in (("fused", 4), ("literal", 3)):
                row[name] = dict(median_ms=round(statistics.median(ms[name]), 3), min_ms=round(min(ms[name]), 3),
                                 max_ms=round(max(ms[name]), 3), calls=len(ms[name]), peak_extra_mib=round(peak[name], 1),
                                 fp32_pipe_floor_ms=round(products * flop / (a.tflops * 1e12) * 1e3, 3))
            row["literal_over_fused_ms"] = round(row["literal"]["median_ms"] / row["fused"]["median_ms"], 2)
            for i, what in enumerate(("loss", "grad_rendered", "grad_decoder")):
                x, y = last["fused"][i].double(), last["literal"][i].double()
                row[f"max_diff_over_max_{what}"] = float((x - y).abs().max() / y.abs().max().clamp_min(1e-300))
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
            del last
        del rendered, conv
        torch.cuda.empty_cache()

    # one step of the fit, split (hip events around every stage; the front of a new view every step)
    d = 128
    latents = (0.1 * torch.randn(n, d, generator=g, device=dev)).requires_grad_(True)
    conv = torch.rand(d, D, generator=g, device=dev).requires_grad_(True)
    opt = torch.optim.Adam([latents, conv], lr=2.5e-3)
    stages = ("front", "render", "decode_loss", "scatter", "adam")
    ms = {k: [] for k in stages}
    eng.set_narrow_scatter(True)
    for step in range(a.steps + 1):
        view = eng.view(vms[step], K, W, H)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)]
        ev[0].record()
        eng.project(view, *gauss)
        eng.bin_sort(view)
        eng.blend_weights(view)
        eng.holds_new_view()
        ev[1].record()
        rendered = eng.render(view, latents.detach())
        ev[2].record()
        _, g_r, g_c, _ = eng.decode_loss(rendered, conv.detach(), target, scale=1.0 / (H * W * D), grad_rendered=rendered)
        ev[3].record()
        g_l = torch.zeros(n, d, device=dev)
        eng.scatter(view, g_r, g_l, None)
        ev[4].record()
        latents.grad, conv.grad = g_l, g_c
        opt.step()
        ev[5].record()
        torch.cuda.synchronize()
        if step > 0:
            for i, k in enumerate(stages):
                ms[k].append(ev[i].elapsed_time(ev[i + 1]))
    if eng.stats()["overflow"]:
        raise SystemExit("workspace overflow: the step timings are void")
    res["fit_step"] = dict(d=d, D=D, steps=a.steps, **{k + "_ms": round(statistics.median(v), 3) for k, v in ms.items()},
                           total_ms=round(sum(statistics.median(v) for v in ms.values()), 3))
    print(json.dumps(res["fit_step"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
