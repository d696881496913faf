#!/usr/bin/env python3
"""The photometric loss at full size (1600 x 1060 x 3, C2 geometry) beside the render it belongs to, in one run on one device, the
forms alternating inside every repeat:

  kernel_forward           Engine.image_loss: forward + reduce (gwbp_image_loss without grad)
  kernel_forward_backward  Engine.image_loss(want_grad=True): forward, reduce, backward
  torch_conv2d             the loss in torch float32, SSIM by five 11 x 11 grouped convolutions, forward + autograd backward
  torch_separable          the same with every blur as an 11 x 1 and a 1 x 11 grouped convolution, forward + backward
  render_pixels            gwbp_render_pixels of the D = 3 table on the projected and sorted view
  render_pixels_backward   gwbp_render_pixels_backward (the blend backward) with the loss's gradient image

    timeout -k 10 900 python tools/time_image_loss.py --out profiles/image_loss.json

Each form is timed between one pair of hip events; ms is the median over --repeats.  peak_mib is torch.cuda.max_memory_allocated over
the form, above what was allocated before it.  Merges its section into the file (tools/record_image_loss.py writes the errors there).
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
import torch.nn.functional as F  # noqa: E402
from gsbp_amd import photometric  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402
from gsbp_amd.rasterization import get_engine  # noqa: E402
from record_image_loss import merge  # noqa: E402

FORMS = ("kernel_forward", "kernel_forward_backward", "torch_conv2d", "torch_separable", "render_pixels", "render_pixels_backward")
C1, C2 = 0.01 ** 2, 0.03 ** 2


def torch_loss(x, y, lam, separable):
    """(1 - lam) l1 + lam (1 - mean ssim) over the valid windows, [H, W, 3] float32 inputs, as a CUDA trainer writes it in torch."""
    g = photometric.gaussian_window().to(x.device)
    a, b = x.permute(2, 0, 1)[None], y.permute(2, 0, 1)[None]
    ch = a.shape[1]
    if separable:
        kh, kv = g.view(1, 1, 1, 11).expand(ch, 1, 1, 11), g.view(1, 1, 11, 1).expand(ch, 1, 11, 1)

        def blur(v):
            return F.conv2d(F.conv2d(v, kh, groups=ch), kv, groups=ch)
    else:
        k2 = (g[:, None] * g[None, :]).expand(ch, 1, 11, 11)

        def blur(v):
            return F.conv2d(v, k2, groups=ch)
    mu1, mu2 = blur(a), blur(b)
    s1, s2, s12 = blur(a * a) - mu1 * mu1, blur(b * b) - mu2 * mu2, blur(a * b) - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return (1 - lam) * (x - y).abs().mean() + lam * (1 - ssim.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_image_loss.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    cfg = syn.CONFIGS[a.config]
    W, H, n = cfg.width, cfg.height, cfg.n_gaussians
    gauss = tuple(t.to(dev).contiguous() for t in syn.activate(syn.make_scene(cfg)))
    vms, K = syn.make_cameras(cfg, n_views=2), syn.intrinsics(cfg)
    eng = get_engine(dev, n, W, H)
    table = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(dev)

    def front(v):
        for _ in range(6):
            view = eng.view(vms[v], K, W, H)
            eng.project(view, *gauss)
            eng.bin_sort(view)
            stats = eng.stats()
            if not stats["overflow"]:
                return view
            eng.grow(stats, views=1)
        raise SystemExit("the workspace kept overflowing")

    target = eng.render_pixels(front(1), table)[0].clamp(0, 1).clone()
    view = front(0)
    x = eng.render_pixels(view, table)[0].clamp(0, 1).clone()
    lam = 0.2
    grad = eng.image_loss(x, target, lam, "valid", want_grad=True)[2].clone()
    v_alpha = torch.zeros(H, W, device=dev)

    def torch_form(separable):
        xr = x.clone().requires_grad_(True)
        torch_loss(xr, target, lam, separable).backward()
        return xr.grad

    forms = dict(kernel_forward=lambda: eng.image_loss(x, target, lam, "valid"),
                 kernel_forward_backward=lambda: eng.image_loss(x, target, lam, "valid", want_grad=True),
                 torch_conv2d=lambda: torch_form(False), torch_separable=lambda: torch_form(True),
                 render_pixels=lambda: eng.render_pixels(view, table),
                 render_pixels_backward=lambda: eng.render_pixels_backward(view, table, grad, v_alpha))
    ms, peak = {k: [] for k in FORMS}, {k: 0.0 for k in FORMS}
    for rep in range(a.repeats + a.warmup):
        for name in FORMS:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = forms[name]()
            t1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms[name].append(t0.elapsed_time(t1))
                peak[name] = max(peak[name], (torch.cuda.max_memory_allocated() - base) / 2 ** 20)
            del out
    # the two sides agree (a timing of a wrong result is no timing)
    g_t = torch_form(True)
    agree = float((grad - g_t).norm() / g_t.norm())
    timing = dict(tool="tools/time_image_loss.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), config=a.config,
                  width=W, height=H, D=3, ssim_lambda=lam, padding="valid", repeats=a.repeats, warmup=a.warmup,
                  kernel_vs_torch_gradient_rel=float(f"{agree:.3e}"), forms={})
    for name in FORMS:
        ts = ms[name]
        timing["forms"][name] = dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                                     peak_mib=round(peak[name], 1))
        print(name, json.dumps(timing["forms"][name]), flush=True)
    f = timing["forms"]
    timing["kernel_forward_backward_over_blend_backward"] = round(f["kernel_forward_backward"]["median_ms"]
                                                                  / f["render_pixels_backward"]["median_ms"], 3)
    timing["torch_separable_over_kernel"] = round(f["torch_separable"]["median_ms"] / f["kernel_forward_backward"]["median_ms"], 2)
    print("timing", json.dumps({k: v for k, v in timing.items() if k != "forms"}), flush=True)
    if a.out:
        merge(a.out, dict(timing=timing))
    return 0


if __name__ == "__main__":
    sys.exit(main())
