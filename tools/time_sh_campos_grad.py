#!/usr/bin/env python3
"""The SH colours' backward with the camera centre on the device (csrc/sh.hip) at tools/time_sh_grad.py's size (C2:
1 000 000 Gaussians, SH degree 3, features_dc and features_rest as they are stored), in one run on one device, the forms alternating
inside every repeat:

  bwd_host        Engine.sh_eval_backward: k_sh_eval_bwd, the centre three kernel arguments (the parent commit's kernel)
  bwd_dev         Engine.sh_eval_backward_dev(want_campos=False): k_sh_eval_bwd_dev without the reduction
  bwd_dev_campos  the same with want_campos=True: the reduction, the [n_blocks, 3] partials and k_sh_campos_sum
  fwd_host, fwd_dev   Engine.sh_eval and Engine.sh_eval_dev

    timeout -k 10 900 python tools/time_sh_campos_grad.py --out profiles/sh_campos_grad.json

A form's time is one pair of hip events around --calls calls that end in a synchronise, divided by --calls (the output allocations
are inside: they are what a training step pays); ms is the median over --repeats, with min and max.  The three backward forms must
agree bit for bit in v_head, v_tail and v_means before anything is reported.  "errors": every case of
tests/test_gpu_sh_campos_grad.py's floor rule for v_campos, measured with that file's own functions; FACTOR there is ceil(2 x the
largest ratio).  Nothing is asserted on the timings.
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


def measure_errors(dev):
    import test_gpu_sh_campos_grad as cases  # noqa: E402  (the test file's cases and its two sides)
    rows, top, worst = [], 0.0, None
    for n, d, k, name, k_head, shifted in cases.cases():
        r = cases.measure(dev, n, d, k, k_head, shifted)
        fig = max(r, key=r.get)
        rows.append(dict(n=n, degree=d, K=k, layout=name, figure=fig, ratio=round(r[fig], 4)))
        if r[fig] > top:
            top, worst = r[fig], rows[-1]
    return dict(cases=len(rows), figures=2 * len(rows), largest=round(top, 4), worst=worst, factor=math.ceil(2 * top),
                factor_in_test=cases.FACTOR, consistency_bound=cases.CONSISTENCY, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sh_campos_grad.py measures on a GPU; there is nothing to report without one")
    dev = torch.device("cuda:0")
    errors = measure_errors(dev)
    print("errors", json.dumps({k: v for k, v in errors.items() if k != "rows"}), flush=True)
    cfg = syn.CONFIGS[a.config]
    n, k = cfg.n_gaussians, 16
    gen = torch.Generator().manual_seed(syn.SH_SEED)
    means = syn.make_scene(cfg)["means"].contiguous().to(dev)
    dc = ((torch.rand(n, 1, 3, generator=gen) - 0.5) / 0.28209479177387814).to(dev)
    rest = (0.05 * torch.randn(n, k - 1, 3, generator=gen)).to(dev)
    v_colors = torch.randn(n, 3, generator=gen).to(dev)
    vm = syn.make_cameras(cfg, n_views=1)[0]
    campos_host = (-(vm[:3, :3].T @ vm[:3, 3])).tolist()
    campos_dev = torch.tensor(campos_host, dtype=torch.float32, device=dev)
    eng = gsbp_amd.Engine(n, 32, 32, device=dev)
    forms = dict(bwd_host=lambda: eng.sh_eval_backward(3, means, dc, rest, campos_host, v_colors),
                 bwd_dev=lambda: eng.sh_eval_backward_dev(3, means, dc, rest, campos_dev, v_colors, want_campos=False),
                 bwd_dev_campos=lambda: eng.sh_eval_backward_dev(3, means, dc, rest, campos_dev, v_colors),
                 fwd_host=lambda: eng.sh_eval(3, means, dc, rest, campos_host),
                 fwd_dev=lambda: eng.sh_eval_dev(3, means, dc, rest, campos_dev))
    # the forms computed the same thing, bit for bit: a timing of a different result is no timing
    a0, a1, a2 = forms["bwd_host"](), forms["bwd_dev"](), forms["bwd_dev_campos"]()
    for i in range(3):
        assert torch.equal(a0[i].view(torch.int32), a1[i].view(torch.int32)) and torch.equal(a0[i].view(torch.int32), a2[i].view(torch.int32))
    assert torch.equal(forms["fwd_host"]().view(torch.int32), forms["fwd_dev"]().view(torch.int32))
    gap = (a2[3] + a2[2].double().sum(dim=0)).abs() / a2[2].double().abs().sum(dim=0)
    ms = {name: [] for name in forms}
    for rep in range(a.repeats + a.warmup):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                fn()
            t1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms[name].append(t0.elapsed_time(t1) / a.calls)
    timing = dict(tool="tools/time_sh_campos_grad.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"),
                  config=a.config, n_gaussians=n, sh_degree=3, K=k, repeats=a.repeats, warmup=a.warmup, calls_per_window=a.calls,
                  n_blocks=(n + 255) // 256, forms={})
    for name, ts in ms.items():
        timing["forms"][name] = dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))
        print(name, json.dumps(timing["forms"][name]), flush=True)
    f = timing["forms"]
    timing["bwd_dev_over_bwd_host"] = round(f["bwd_dev"]["median_ms"] / f["bwd_host"]["median_ms"], 4)
    timing["bwd_dev_campos_over_bwd_host"] = round(f["bwd_dev_campos"]["median_ms"] / f["bwd_host"]["median_ms"], 4)
    timing["fwd_dev_over_fwd_host"] = round(f["fwd_dev"]["median_ms"] / f["fwd_host"]["median_ms"], 4)
    timing["v_campos_consistency_at_full_size"] = [float(g) for g in gap.cpu()]
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
