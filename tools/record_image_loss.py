#!/usr/bin/env python3
"""The figures behind the two measured constants of tests/test_gpu_image_loss.py, on one device:

  errors       every case of the test file's floor rule -- shape x padding x D x weights x lambda -- as the four ratios
               |kernel - truth| / max(|float32 restatement - truth|, 2^-24 x the figure of truth) (map and gradient; Frobenius and
               max-abs); the largest of them all decides FACTOR = ceil(2 x largest), ceiling 16
  refine_pose  refine_pose(loss="photometric") on the camera test's case beside the same loop under the torch float32 restatement of
               the loss, --repeats times (rasterization()'s backward sums with float atomics: two runs differ); the largest relative
               difference of the final pose errors decides POSE_MARGIN = 2 x largest, at most 10 %

    timeout -k 10 600 python tools/record_image_loss.py --out profiles/image_loss.json

Merges its two sections into the file (tools/time_image_loss.py writes the timings there).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gsbp_amd  # noqa: E402,F401
import torch  # noqa: E402


def merge(path, sections):
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.update(sections)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_image_loss.py measures on a GPU; there is nothing to report without one")
    import test_gpu_image_loss as cases  # noqa: E402  (the test file's cases and its two sides)
    dev = torch.device("cuda:0")
    names = ("map_fro", "map_max", "grad_fro", "grad_max")
    rows = []
    for H, W, D, padding, weighted, lam in cases.all_cases():
        r = cases.kernel_ratios(dev, H, W, D, padding, weighted, lam)
        rows.append(dict(H=H, W=W, D=D, padding=padding, weighted=weighted, ssim_lambda=lam,
                         **{k: float(f"{x:.3e}") for k, x in zip(names, r)}))
    largest = {k: max(r[k] for r in rows) for k in names}
    worst = max(rows, key=lambda r: max(r[k] for k in names))
    top = max(largest.values())
    errors = dict(cases=len(rows), largest=largest, worst=worst, factor=math.ceil(2 * top), factor_in_test=cases.FACTOR, ceiling=16,
                  rows=rows)
    print("errors", json.dumps({k: v for k, v in errors.items() if k != "rows"}), flush=True)
    diffs, runs = [], []
    for _ in range(a.repeats):
        end_k, end_t, start, res = cases.refine_both(dev)
        diffs.append(cases.relative_difference(end_k, end_t))
        runs.append(dict(kernel=dict(angle_rad=end_k[0], distance=end_k[1]), torch_float32=dict(angle_rad=end_t[0], distance=end_t[1]),
                         loss_first=res["history"][0], loss_last=res["history"][-1], relative_difference=float(f"{diffs[-1]:.3e}")))
    pose = dict(start=dict(angle_rad=start[0], distance=start[1]), runs=runs, largest_relative_difference=float(f"{max(diffs):.3e}"),
                margin=min(2 * max(diffs), 0.10), margin_in_test=cases.POSE_MARGIN)
    print("refine_pose", json.dumps(pose), flush=True)
    if a.out:
        merge(a.out, dict(record=dict(tool="tools/record_image_loss.py", device=torch.cuda.get_device_name(0),
                                      date=time.strftime("%Y-%m-%d")), errors=errors, refine_pose=pose))
    return 0


if __name__ == "__main__":
    sys.exit(main())
