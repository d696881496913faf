#!/usr/bin/env python3
"""Times the consumers of a finished field on fp32, fp16 and bf16 fields and writes profiles/half_fields.json.

    python tools/time_half_fields.py [--n 1000000] [--dims 512,1024] [--dtypes fp16,bf16] [--repeats 7] [--only NAME,...] [--out ...]

For every consumer that reads a half field natively (prompt_scores, knn_search, kmeans_assign, cluster_sums, neighbor_similarity,
neighbor_mean, neighbor_blend, column_means + centered_gram as pca._covariance, pca_transform) and for the finalise, FOUR forms are
run one after the other in every round, so that whatever else the machine does hits them alike:

    a  the fp32 field                              c  the half field, read natively
    b  the same call on the fp32 field again       d  the earlier form: field.float(), then the fp32 kernel, the copy inside the timing
       (the a / b difference is the spread)

For the finalise: a, b = fp32 out; c = the typed out; d = the fp32 finalise followed by .to(dtype).  Each form is timed with device
events around the Python call (which includes the allocation of its outputs from the caching allocator) after one warm-up round; the
median over the rounds is kept, with the peak of torch.cuda.max_memory_allocated over the call above what was allocated before it.
The field: N unit rows drawn in fp32 and rounded to the half type, so that a, b and d read the values c reads.  Neighbour lists: k
rows within +-4096 of the row (a spatially sorted scene's locality).  The expectation the figures are reported against: c is not
slower than a beyond the a / b spread, and c is faster than d.  The file is rewritten after every case."""
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
from gsbp_amd import pca, sample, spatial  # noqa: E402

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
P, M_SRC, K_NN, K_MEANS, K_LIST = 4, 1024, 5, 64, 8


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


def consumers(n, d, dev, gen):
    prompts = torch.nn.functional.normalize(torch.randn(P, d, generator=gen), dim=1).to(dev)
    sources = torch.nn.functional.normalize(torch.randn(M_SRC, d, generator=gen), dim=1).to(dev)
    centroids = torch.nn.functional.normalize(torch.randn(K_MEANS, d, generator=gen), dim=1).to(dev)
    labels = torch.randint(0, K_MEANS, (n,), generator=gen).to(dev)
    idx = (torch.arange(n)[:, None] + torch.randint(-4096, 4097, (n, K_LIST), generator=gen)).clamp_(0, n - 1).to(torch.int32).to(dev)
    w = torch.rand(n, K_LIST, generator=gen).to(dev)
    basis = pca.PCABasis(torch.zeros(d, device=dev), torch.linalg.qr(torch.randn(d, 3, generator=gen)).Q.T.contiguous().to(dev),
                         None, None, n)
    return {
        "prompt_scores": lambda f: gsbp_amd.prompt_scores(f, prompts),
        "knn_search": lambda f: gsbp_amd.knn_search(f, sources, K_NN),
        "kmeans_assign": lambda f: gsbp_amd.kmeans_assign(f, centroids, "euclidean"),
        "cluster_sums": lambda f: gsbp_amd.cluster_sums(f, labels, K_MEANS),
        "neighbor_similarity": lambda f: gsbp_amd.neighbor_similarity(f, idx),
        "neighbor_mean": lambda f: spatial.neighbor_mean(f, idx),
        "neighbor_blend": lambda f: sample.neighbor_blend(f, idx, w),
        "pca_covariance": lambda f: pca._covariance(f),
        "pca_transform": lambda f: gsbp_amd.pca_transform(f, basis),
    }


def summarise(times, peaks):
    out = {}
    for form in "abcd":
        out[form] = {"median_ms": round(statistics.median(times[form]), 3), "min_ms": round(min(times[form]), 3),
                     "max_ms": round(max(times[form]), 3), "peak_bytes": int(max(peaks[form]))}
    a, b, c, d = (out[f]["median_ms"] for f in "abcd")
    out["spread_b_over_a"] = round(b / a, 3)
    out["c_over_a"] = round(c / a, 3)
    out["c_over_d"] = round(c / d, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="512,1024")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", default=None, help="comma-separated consumer names (and 'finalize')")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_fields.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_half_fields.py needs a GPU")
    dev = torch.device("cuda")
    only = set(args.only.split(",")) if args.only else None
    res = {"tool": "tools/time_half_fields.py", "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "n": args.n, "repeats": args.repeats,
           "forms": {"a": "fp32 field", "b": "fp32 field again (spread)", "c": "half field, native",
                     "d": "half field through .float() + the fp32 kernel (finalize: fp32 finalise + .to(dtype))"},
           "timing": "device events around the Python call, forms a b c d alternated in every round after one warm-up round, median over "
                     "the rounds; peak_bytes = torch.cuda.max_memory_allocated over the call above the bytes allocated before it",
           "expectation": "c_over_a <= about spread_b_over_a, c_over_d < 1", "cases": []}
    n = args.n
    for d in (int(s) for s in args.dims.split(",")):
        gen = torch.Generator().manual_seed(d)
        calls = consumers(n, d, dev, gen)
        eng = gsbp_amd.Engine(n, 64, 64, device=dev)
        for name, dtype in ((k, DTYPES[k]) for k in args.dtypes.split(",")):
            f16 = torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=1).to(dtype).to(dev)
            f32 = f16.float()
            acc, den = f32 * 3.0, torch.full((n,), 2.0, device=dev)  # accumulators whose finalise is the field
            todo = {k: {"a": lambda c=c: c(f32), "b": lambda c=c: c(f32), "c": lambda c=c: c(f16), "d": lambda c=c: c(f16.float())}
                    for k, c in calls.items()}
            todo["finalize"] = {"a": lambda: eng.finalize(acc, den), "b": lambda: eng.finalize(acc, den),
                                "c": lambda: eng.finalize_typed(acc, den, dtype), "d": lambda: eng.finalize(acc, den).to(dtype)}
            for cname, forms in todo.items():
                if only is not None and cname not in only:
                    continue
                times, peaks = {f: [] for f in "abcd"}, {f: [] for f in "abcd"}
                for r in range(args.repeats + 1):
                    for form in "abcd":
                        ms, peak = measure(forms[form])
                        if r > 0:  # (round 0 warms every form)
                            times[form].append(ms)
                            peaks[form].append(peak)
                case = {"consumer": cname, "dtype": name, "n": n, "D": d, "field_bytes_fp32": 4 * n * d, "field_bytes_half": 2 * n * d}
                case.update(summarise(times, peaks))
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as fh:
                    json.dump(res, fh, indent=1)
            del f16, f32, acc, den, todo
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
