#!/usr/bin/env python3
"""Times the calls that read a finished field as a RENDER PAYLOAD, and the two that can write a half field, on fp32, fp16 and bf16
fields, and writes profiles/half_payloads.json.

    python tools/time_half_payloads.py [--config C2] [--dtypes fp16,bf16] [--repeats 7] [--only NAME,...] [--out ...]

One view of the seeded config (C2: N = 1 M Gaussians, 1600 x 1060) is projected, sorted and blended once; the cases run on it:

    render           Engine.render, D = 512 (k_render_rows4)             probe_pixels    Engine.probe_pixels, M = 1024, D = 512
    field_compare    Engine.field_compare, D = 512, fp32 map, no planes  neighbor_mean   spatial.neighbor_mean, D = 512, k = 8
    render_pixels    Engine.render_pixels, D = 16 (k_render_px)          neighbor_blend  sample.neighbor_blend, D = 512, k = 8

The protocol is tools/time_half_fields.py's: FOUR forms run one after the other in every round, so that whatever else the machine does
hits them alike, timed with device events around the Python call (the allocation of its outputs included) after one warm-up round;
the median over the rounds is kept, with the peak of torch.cuda.max_memory_allocated over the call above what was allocated before it.

    a  the fp32 payload                            c  the half payload, read natively
    b  the same call again (a / b is the spread)   d  the earlier form: payload.float(), then the fp32 kernel, the copy inside the timing

For neighbor_mean and neighbor_blend the subject is the half OUTPUT, on a half field: a, b = the fp32 out; c = out_dtype = the half
type; d = the fp32 out followed by .to(dtype).  There is no pass / fail threshold on a time; the requirement is the memory: c allocates
no 4 N D bytes beyond what a allocates (c_peak_minus_a_peak <= 0 for the payload cases, where d_peak_minus_a_peak is the copy).  The
file is rewritten after every case."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gsbp_amd  # noqa: E402
from gsbp_amd import sample, spatial, synthetic as syn  # noqa: E402

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
D_WIDE, D_PX, M_PROBE, K_LIST = 512, 16, 1024, 8


def measure(fn):
    """(milliseconds, peak bytes above the bytes allocated before the call) of one call."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return a.elapsed_time(b), peak


def summarise(times, peaks):
    out = {}
    for form in "abcd":
        out[form] = {"median_ms": round(statistics.median(times[form]), 3), "min_ms": round(min(times[form]), 3),
                     "max_ms": round(max(times[form]), 3), "peak_bytes": int(max(peaks[form]))}
    a, b, c, d = (out[f]["median_ms"] for f in "abcd")
    out["spread_b_over_a"] = round(b / a, 3)
    out["c_over_a"] = round(c / a, 3)
    out["c_over_d"] = round(c / d, 3)
    # (the memory requirement: c allocates what a allocates -- the outputs -- and d one fp32 field more)
    out["c_peak_minus_a_peak"] = out["c"]["peak_bytes"] - out["a"]["peak_bytes"]
    out["d_peak_minus_a_peak"] = out["d"]["peak_bytes"] - out["a"]["peak_bytes"]
    return out


def front(cfg, dev):
    """(engine, view) with view 0 of the config projected, sorted and blended; the workspace grown until nothing overflows."""
    gauss = [t.to(dev) for t in syn.activate(syn.make_scene(cfg))]
    vm, K = syn.make_cameras(cfg, n_views=1)[0].to(dev), syn.intrinsics(cfg).to(dev)
    eng = gsbp_amd.Engine(cfg.n_gaussians, cfg.width, cfg.height, device=dev)
    for _ in range(6):
        view = eng.view(vm, K, cfg.width, cfg.height)
        eng.project(view, *gauss)
        eng.bin_sort(view)
        eng.blend_weights(view)
        stats = eng.stats()
        if not stats["overflow"]:
            return eng, view, stats
        eng.grow(stats)
    raise SystemExit(f"the workspace still overflows: {stats}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", default=None, help="comma-separated case names")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_payloads.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_half_payloads.py needs a GPU")
    dev = torch.device("cuda")
    only = set(args.only.split(",")) if args.only else None
    cfg = syn.CONFIGS[args.config]
    n, W, H = cfg.n_gaussians, cfg.width, cfg.height
    eng, view, stats = front(cfg, dev)
    res = {"tool": "tools/time_half_payloads.py", "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "config": cfg.name, "n": n, "width": W, "height": H, "n_pairs": int(stats["n_pairs"]), "repeats": args.repeats,
           "forms": {"a": "fp32 payload", "b": "fp32 payload again (spread)", "c": "half payload, native",
                     "d": "half payload through .float() + the fp32 kernel",
                     "neighbor_mean, neighbor_blend": "on a half field: a, b = fp32 out, c = half out (out_dtype), d = fp32 out + .to(dtype)"},
           "timing": "device events around the Python call, forms a b c d alternated in every round after one warm-up round, median over "
                     "the rounds; peak_bytes = torch.cuda.max_memory_allocated over the call above the bytes allocated before it",
           "requirement": "the peak of c holds no 4 N D bytes; no threshold on a time", "cases": []}
    gen = torch.Generator().manual_seed(512)
    torch.manual_seed(512)
    fmap = syn.make_feature_map(cfg, 0, device=dev, dim=D_WIDE)
    xy = torch.stack([torch.randint(0, W, (M_PROBE,), generator=gen), torch.randint(0, H, (M_PROBE,), generator=gen)], dim=1)
    xy = xy.to(torch.int32).to(dev)
    idx = (torch.arange(n)[:, None] + torch.randint(-4096, 4097, (n, K_LIST), generator=gen)).clamp_(0, n - 1).to(torch.int32).to(dev)
    w = torch.rand(n, K_LIST, generator=gen).to(dev)
    payload = {"render": (D_WIDE, lambda f: eng.render(view, f)),
               "field_compare": (D_WIDE, lambda f: eng.field_compare(view, f, fmap, want_planes=False)),
               "render_pixels": (D_PX, lambda f: eng.render_pixels(view, f)),
               "probe_pixels": (D_WIDE, lambda f: eng.probe_pixels(view, xy, f))}
    outputs = {"neighbor_mean": lambda f, od: spatial.neighbor_mean(f, idx, out_dtype=od),
               "neighbor_blend": lambda f, od: sample.neighbor_blend(f, idx, w, out_dtype=od)[0]}
    for name, dtype in ((k, DTYPES[k]) for k in args.dtypes.split(",")):
        fields = {}
        for d in (D_WIDE, D_PX):
            f16 = torch.nn.functional.normalize(torch.randn(n, d, device=dev), dim=1).to(dtype)  # (seeded: torch.manual_seed above)
            fields[d] = (f16.float(), f16)
        todo = {}
        for k, (d, c) in payload.items():
            f32, f16 = fields[d]
            todo[k] = (d, {"a": lambda c=c, f=f32: c(f), "b": lambda c=c, f=f32: c(f), "c": lambda c=c, f=f16: c(f),
                           "d": lambda c=c, f=f16: c(f.float())})
        for k, c in outputs.items():
            f16 = fields[D_WIDE][1]
            todo[k] = (D_WIDE, {"a": lambda c=c, f=f16: c(f, None), "b": lambda c=c, f=f16: c(f, None),
                                "c": lambda c=c, f=f16: c(f, dtype), "d": lambda c=c, f=f16: c(f, None).to(dtype)})
        for cname, (d, forms) in todo.items():
            if only is not None and cname not in only:
                continue
            times, peaks = {f: [] for f in "abcd"}, {f: [] for f in "abcd"}
            for r in range(args.repeats + 1):
                for form in "abcd":
                    ms, peak = measure(forms[form])
                    if r > 0:  # (round 0 warms every form)
                        times[form].append(ms)
                        peaks[form].append(peak)
            case = {"case": cname, "dtype": name, "n": n, "D": d, "field_bytes_fp32": 4 * n * d, "field_bytes_half": 2 * n * d}
            case.update(summarise(times, peaks))
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        del fields, todo
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
