#!/usr/bin/env python3
"""Prompt segmentation at full size: gwbp_prompt_scores beside its two yardsticks taken in the same run -- (a) the torch form of the
reference, F.normalize(F) @ T.T, two max calls and the compare, and (b) gwbp_pca_project at the same N and D with k = min(P, 16),
the closest existing kernel --, probe_pixels for M = 1, 16, 256 after a cached front beside the full "RGB+D" render of the field
(the only way to those numbers before), and one C2-size 2-D mask frame beside the literal 512-channel form.

    timeout -k 10 1100 python tools/time_segment.py --out profiles/segment.json

Every form is warmed up once and timed --repeats times with hip events around one whole call (min and median reported); peak_mib
is the torch.cuda.max_memory_allocated delta of one call (outputs included).  read_floor_ms is one read of the field at the measured
6.29 TB/s copy rate; floor_fraction = floor / min time.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gsbp_amd  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gsbp_amd import pca  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402
from time_pca import HBM, field, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="16,512,1024")
    ap.add_argument("--prompts", default="3,8,32")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-frames", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    res = dict(tool="tools/time_segment.py", device=torch.cuda.get_device_name(0), repeats=a.repeats, date=time.strftime("%Y-%m-%d"),
               hbm_copy_bytes_per_s=HBM, rows=[], probes=[], frames={})
    n = a.n
    for D in [int(x) for x in a.dims.split(",")]:
        X = field(n, D, dev, g)
        read_floor = 4.0 * n * D / HBM * 1e3
        for P in [int(x) for x in a.prompts.split(",")]:
            T = F.normalize(torch.randn(P, D, device=dev, generator=g), dim=1)
            n_pos = max(1, P // 3)

            def torch_form():
                s = F.normalize(X, dim=1) @ T.T
                return s[:, :n_pos].max(dim=1)[0] > s[:, n_pos:].max(dim=1)[0]
            k = min(P, 16, D)
            zero = torch.zeros(D, device=dev)
            row = dict(N=n, D=D, P=P, n_pos=n_pos, read_floor_ms=round(read_floor, 3),
                       prompt_mask=timed(lambda: gsbp_amd.prompt_mask(X, T, n_pos), a.repeats),
                       prompt_scores=timed(lambda: gsbp_amd.prompt_scores(X, T), a.repeats),
                       torch_normalize_matmul_max_compare=timed(torch_form, a.repeats),
                       pca_project_k=k, pca_project=timed(lambda: pca._project(X, zero, T[:k]), a.repeats))
            row["mask_floor_fraction"] = round(read_floor / row["prompt_mask"]["min_ms"], 3)
            row["mask_over_pca_project"] = round(row["prompt_mask"]["min_ms"] / row["pca_project"]["min_ms"], 3)
            row["torch_over_mask"] = round(row["torch_normalize_matmul_max_compare"]["min_ms"] / row["prompt_mask"]["min_ms"], 2)
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
        del X
        torch.cuda.empty_cache()
    if not a.no_frames:
        cfg = syn.CONFIGS["C2"]
        D = cfg.feat_dim
        gauss = tuple(t.to(dev) for t in syn.activate(syn.make_scene(cfg)))
        vms, K = syn.make_cameras(cfg, n_views=1).to(dev), syn.intrinsics(cfg).to(dev)
        W, H = cfg.width, cfg.height
        Fs = field(cfg.n_gaussians, D, dev, g)
        T = F.normalize(torch.randn(8, D, device=dev, generator=g), dim=1)
        with torch.no_grad():
            full = timed(lambda: gsbp_amd.rasterization(*gauss, Fs, vms, K[None], W, H, render_mode="RGB+D", want_meta=False)[0],
                         max(2, a.repeats // 2))
            for M in (1, 16, 256):
                xy = torch.stack([torch.randint(0, W, (M,), generator=torch.Generator().manual_seed(M)),
                                  torch.randint(0, H, (M,), generator=torch.Generator().manual_seed(M + 1))], dim=1).to(dev).int()
                row = dict(M=M, D=D, probe_pixels=timed(lambda: gsbp_amd.probe_pixels(*gauss, Fs, vms[0], K, W, H, xy), a.repeats),
                           full_rgbd_render=full)
                print(json.dumps(row), flush=True)
                res["probes"].append(row)

            def literal():
                out = gsbp_amd.rasterization(*gauss, Fs, vms, K[None], W, H, want_meta=False)[0][0]
                s = F.normalize(out, dim=-1) @ T.T
                return s[..., :3].max(dim=2)[0] > s[..., 3:].max(dim=2)[0]
            table = gsbp_amd.prompt_scores(Fs, T, normalize=False)

            def epilogue():
                s = gsbp_amd.rasterization(*gauss, table, vms, K[None], W, H, want_meta=False)[0][0]
                return s

            res["frames"] = dict(N=cfg.n_gaussians, D=D, P=8, width=W, height=H,
                                 render_prompt_mask=timed(lambda: next(gsbp_amd.render_prompt_mask(*gauss, Fs, vms, K, W, H, T, 3)),
                                                          a.repeats),
                                 of_which_scores_table=timed(lambda: gsbp_amd.prompt_scores(Fs, T, normalize=False), a.repeats),
                                 of_which_render_8_channels=timed(epilogue, a.repeats),
                                 literal_512_channel_form=timed(literal, max(2, a.repeats // 2)))
            print(json.dumps(res["frames"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
