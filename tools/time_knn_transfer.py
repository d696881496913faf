#!/usr/bin/env python3
"""Label transfer by k-NN search at the affordance demo's size: the fused search (and search + vote) against the torch formulation
a user had before it, torch.topk(Q[i:i+c] @ S.T, k) over query chunks of at most 1 GiB of scores + label gather and vote.

    timeout -k 10 1100 python tools/time_knn_transfer.py --out profiles/knn_transfer.json

Per (D, M, k): every form is warmed up once and timed --repeats times with hip events around one whole call (min and median
reported); floor_ms = 2 N M D / 157.3e12 (the fp32 matrix pipe's peak), floor_fraction = floor_ms / min time; peak_mib = the
torch.cuda.max_memory_allocated delta of one call (outputs included).  pass: at D = 1024, k = 5 the fused search + vote is not slower
than the torch form beyond the spread of the repeats (fused min <= torch median).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gsbp_amd  # noqa: E402
import torch  # noqa: E402
from gsbp_amd import transfer  # noqa: E402

PEAK = 157.3e12


def torch_form(Q, S, labels, k, nc):
    """What the feature replaces: chunked GEMM + topk, then labels[I] and a per-row bincount().argmax() (one-hot sum)."""
    n, m = Q.shape[0], S.shape[0]
    chunk = max(1, (1 << 30) // (4 * m))
    idx = torch.empty(n, k, dtype=torch.int64, device=Q.device)
    score = torch.empty(n, k, device=Q.device)
    St = S.t()
    for i in range(0, n, chunk):
        sc, ix = torch.topk(Q[i:i + chunk] @ St, k, dim=1)
        score[i:i + chunk], idx[i:i + chunk] = sc, ix
    counts = torch.zeros(n, nc, dtype=torch.int32, device=Q.device)
    counts.scatter_add_(1, labels[idx], torch.ones(n, k, dtype=torch.int32, device=Q.device))
    return score, idx, counts.argmax(dim=1)


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    ts = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1))
    return dict(min_ms=round(min(ts), 3), median_ms=round(statistics.median(ts), 3), max_ms=round(max(ts), 3),
                peak_mib=round(peak, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="384,512,1024")
    ap.add_argument("--sources", default="4096,16384")
    ap.add_argument("--ks", default="5,20")
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    ok = True
    for D in [int(x) for x in a.dims.split(",")]:
        for M in [int(x) for x in a.sources.split(",")]:
            S = torch.randn(M, D, device=dev, generator=g)
            S = S / S.norm(dim=1, keepdim=True)
            Q = S[torch.randint(0, M, (a.n,), device=dev, generator=g)]
            Q = Q + 0.5 * torch.randn(a.n, D, device=dev, generator=g) / D ** 0.5
            Q = Q / Q.norm(dim=1, keepdim=True)
            labels64 = torch.randint(0, a.classes, (M,), device=dev, generator=g)
            labels = labels64.to(torch.int32)
            for k in [int(x) for x in a.ks.split(",")]:
                floor = 2.0 * a.n * M * D / PEAK * 1e3
                search = timed(lambda: gsbp_amd.knn_search(Q, S, k), a.repeats)
                both = timed(lambda: transfer.vote_labels(gsbp_amd.knn_search(Q, S, k)[1], labels, a.classes), a.repeats)
                ref = timed(lambda: torch_form(Q, S, labels64, k, a.classes), a.repeats)
                lab = transfer.vote_labels(gsbp_amd.knn_search(Q, S, k)[1], labels, a.classes)
                agree = float((lab.long() == torch_form(Q, S, labels64, k, a.classes)[2]).float().mean())
                row = dict(N=a.n, D=D, M=M, k=k, floor_ms=round(floor, 3), fused_search=search, fused_search_vote=both,
                           torch_chunked_topk_vote=ref, fused_floor_fraction=round(floor / search["min_ms"], 3),
                           torch_floor_fraction=round(floor / ref["min_ms"], 3),
                           speedup_min=round(ref["min_ms"] / both["min_ms"], 3), labels_agree=round(agree, 5))
                if D == 1024 and k == 5:
                    row["pass"] = both["min_ms"] <= ref["median_ms"]
                    ok = ok and row["pass"]
                print(json.dumps(row), flush=True)
                rows.append(row)
            del Q, S
            torch.cuda.empty_cache()
    res = dict(tool="tools/time_knn_transfer.py", device=torch.cuda.get_device_name(0), repeats=a.repeats,
               date=time.strftime("%Y-%m-%d"), peak_fp32_matrix_flops=PEAK,
               pass_condition="D = 1024, k = 5: fused search + vote min <= torch form median, same run", passed=ok, rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
