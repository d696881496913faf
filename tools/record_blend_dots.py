#!/usr/bin/env python3
"""The figures behind the factor of tests/test_gpu_blend_dots.py: every case of that file, run once on one device.

    timeout -k 10 600 python tools/record_blend_dots.py --out profiles/blend_dots.json

Per case, quantity (the six columns of v_g2d) and figure (fro, max, row): the float32 reference's error against its float64
run (the floor), the kernel's error against the same truth, and kernel / floor.  The file also holds the largest ratio per figure,
the row it was found in, and the factor that follows from it: ceil(2 x the largest ratio), which the test file's FACTOR must equal
and which is not accepted above 16.  A case whose assertions fail under the test file's current FACTOR is listed under "failed" with
its message; its figures are recorded all the same.
"""
import argparse
import json
import math
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gsbp_amd  # noqa: E402,F401
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_blend_dots.py measures on a GPU; there is nothing to report without one")
    import blend_grad_ref as bg  # noqa: E402
    import test_gpu_blend_dots as t  # noqa: E402  (the test file's cases and its two sides)
    dev = torch.device("cuda:0")
    runs = [(t.test_channel_edges, dict(D=D)) for D in t.CHANNELS]
    runs += [(t.test_antialiased_records, {}), (t.test_row_stride_above_the_channel_count, {}), (t.test_without_v_alpha, {}),
             (t.test_v_alpha_alone, {})]
    runs += [(t.test_list_lengths_around_both_batch_sizes, dict(n=n)) for n in t.LIST_LENGTHS]
    runs += [(t.test_termination_past_the_first_batch, dict(opacity=o)) for o in bg.TERMINATION_OPACITIES]
    runs += [(t.test_tile_counts_on_both_parities_of_the_sort_buffer, dict(name=n)) for n in ("t256", "t272")]
    runs += [(t.test_v_g2d_is_added_into, {}), (t.test_non_finite_colours_of_unpaired_gaussians_reach_nothing, {}),
             (t.test_non_finite_colours_of_valid_pairs_stay_at_their_pixels, {})]
    failed, seconds = [], {}
    for fn, kw in runs:
        label = fn.__name__ + (str(sorted(kw.items())) if kw else "")
        t0 = time.time()
        try:
            fn(dev, **kw)
        except AssertionError as e:
            failed.append(dict(test=label, message=(str(e) or traceback.format_exc())[-2000:]))
            print("FAILED", label, (str(e) or traceback.format_exc())[-500:], flush=True)
        torch.cuda.synchronize()
        seconds[label] = round(time.time() - t0, 2)
        print(f"{label}: {seconds[label]} s", flush=True)
    rows = [dict(r, floor=float(f"{r['floor']:.3e}"), kernel=float(f"{r['kernel']:.3e}"),
                 ratio=None if r["ratio"] is None else round(r["ratio"], 3)) for r in t.ROWS]
    worst = {}
    for fig in ("fro", "max", "row"):
        have = [r for r in rows if r["figure"] == fig and r["ratio"] is not None]
        ratios = sorted(r["ratio"] for r in have)
        worst[fig] = dict(largest=max(have, key=lambda r: r["ratio"]), median=ratios[len(ratios) // 2],
                          floor_range=[min(r["floor"] for r in have), max(r["floor"] for r in have)],
                          kernel_range=[min(r["kernel"] for r in have), max(r["kernel"] for r in have)])
    largest = max(w["largest"]["ratio"] for w in worst.values())
    zero_floor = [r for r in rows if r["ratio"] is None]
    res = dict(tool="tools/record_blend_dots.py", device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"),
               cases=len(set(r["case"] for r in rows)), figures=len(rows), largest_ratio=largest,
               factor_from_measurement=math.ceil(2.0 * largest), factor_in_test=t.FACTOR, ceiling=16,
               zero_floor_rows=len(zero_floor), zero_floor_rows_with_kernel_error=sum(r["kernel"] > 0 for r in zero_floor),
               worst=worst, failed=failed, seconds=seconds, rows=rows)
    print(json.dumps({k: v for k, v in res.items() if k not in ("rows", "seconds")}, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
