#!/usr/bin/env python3
"""PCA of a finished field at full size: the fit (means, centred Gram, host eigh, each alone), the transform and one C2-size frame
per mode, beside the torch formulation a user had before -- Xc = F - F.mean(0); Xc.T @ Xc and (F - mu) @ V.T -- and, for the
renderings mode, the literal route (a D-channel rasterization() and a matmul).  Also the MEASURED maxima of the covariance error,
the component angles and the transform error on the cases of tests/pca_ref.py, beside their bounds.

    timeout -k 10 1100 python tools/time_pca.py --out profiles/pca.json

Every form is warmed up once and timed --repeats times with hip events around one whole call (min and median reported); peak_mib
is the torch.cuda.max_memory_allocated delta of one call (outputs included).  Floors: the Gram's is the upper-triangle 128 x 128
tiles' FLOP over the fp32 matrix pipe's 157.3 TF peak; the means' and the transform's is one read of the field at the measured
6.29 TB/s copy rate.  floor_fraction = floor / min time.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gsbp_amd  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gsbp_amd import pca  # noqa: E402
from gsbp_amd import synthetic as syn  # noqa: E402
from gsbp_amd._lib import lib, ptr  # noqa: E402
from gsbp_amd._views import run as _run  # noqa: E402

PEAK = 157.3e12
HBM = 6.29e12


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


def field(n, d, dev, g):
    """Row-normalised rows with a large common component, as lifted features have."""
    f = torch.randn(n, d, device=dev, generator=g)
    f += 3.0 * torch.randn(d, device=dev, generator=g)
    f /= f.norm(dim=1, keepdim=True)
    return f


def accuracy(dev):
    import pca_ref
    rows = []
    for case in pca_ref.FIT_CASES:
        X = pca_ref.make_case(*case)
        Xd = torch.from_numpy(X).to(dev)
        E = pca_ref.cov_bound(X)
        err = np.abs(pca._covariance(Xd)[1].cpu().numpy() - pca_ref.cov64(X))
        theta, norm = pca_ref.angle_bounds(X, 3, E)
        basis = gsbp_amd.fit_pca(Xd)
        comps = pca_ref.fit(X)[1]
        got = basis.components.cpu().numpy()
        mu, V = basis.mean.cpu().numpy(), got
        terr = np.abs(gsbp_amd.pca_transform(Xd, basis).cpu().numpy() - pca_ref.transform64(X, mu, V))
        rows.append(dict(N=case[0], D=case[1], max_cov_error=float(err.max()), max_cov_bound=float(E.max()),
                         max_cov_error_over_bound=float((err / E).max()),
                         angles=[pca_ref.angle(comps[j], got[j]) for j in range(3)], angle_bounds=[float(t) for t in theta],
                         max_transform_error=float(terr.max()),
                         max_transform_error_over_bound=float((terr / pca_ref.transform_bound(X, mu, V)).max())))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="512,1024")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-frames", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    res = dict(tool="tools/time_pca.py", device=torch.cuda.get_device_name(0), repeats=a.repeats, date=time.strftime("%Y-%m-%d"),
               peak_fp32_matrix_flops=PEAK, hbm_copy_bytes_per_s=HBM, accuracy=accuracy(dev), rows=[])
    n = a.n
    for D in [int(x) for x in a.dims.split(",")]:
        F = field(n, D, dev, g)
        need = C.c_size_t(0)
        lib().gwbp_pca_workspace_size(n, D, C.byref(need))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        mean = torch.empty(D, device=dev)
        gram = torch.empty(D, D, dtype=torch.float64, device=dev)
        args = (C.c_int64(n), D, ptr(F), C.c_int64(D))
        means_t = timed(lambda: _run("gwbp_column_means", dev, *args, ptr(mean), ptr(ws), ws.numel()), a.repeats)
        gram_t = timed(lambda: _run("gwbp_centered_gram", dev, *args, ptr(mean), ptr(gram), ptr(ws), ws.numel()), a.repeats)
        cov = (gram / (n - 1)).cpu()
        t0 = time.perf_counter()
        pca._eig_basis(cov, 3)
        eigh_ms = (time.perf_counter() - t0) * 1e3
        del ws
        fit_t = timed(lambda: gsbp_amd.fit_pca(F), a.repeats)
        basis = gsbp_amd.fit_pca(F)
        tr_t = timed(lambda: gsbp_amd.pca_transform(F, basis), a.repeats)
        col_t = timed(lambda: gsbp_amd.pca_colors(F, basis), a.repeats)
        t_gram = timed(lambda: (lambda Xc: Xc.T @ Xc)(F - F.mean(0)), a.repeats)
        t_tr = timed(lambda: (F - basis.mean) @ basis.components.T, a.repeats)
        ref = ((F - F.mean(0)).double().T @ (F - F.mean(0)).double() / (n - 1)).cpu() if D <= 512 else None
        n_tb = -(-D // 128)
        gram_floor = 2.0 * n * (n_tb * (n_tb + 1) // 2) * 128 * 128 / PEAK * 1e3
        read_floor = 4.0 * n * D / HBM * 1e3
        row = dict(N=n, D=D, workspace_mib=round(need.value / 2 ** 20, 1), column_means=means_t, centered_gram=gram_t,
                   host_eigh_ms=round(eigh_ms, 1), fit_pca_whole=fit_t, pca_transform=tr_t, pca_colors=col_t,
                   torch_centred_gram=t_gram, torch_transform=t_tr, gram_floor_ms=round(gram_floor, 3),
                   gram_floor_fraction=round(gram_floor / gram_t["min_ms"], 3), read_floor_ms=round(read_floor, 3),
                   means_floor_fraction=round(read_floor / means_t["min_ms"], 3),
                   transform_floor_fraction=round(read_floor / tr_t["min_ms"], 3),
                   torch_gram_floor_fraction=round(2.0 * n * D * D / PEAK * 1e3 / t_gram["min_ms"], 3))
        if ref is not None:
            row["max_cov_difference_to_float64_torch"] = float((cov - ref).abs().max())
        if D == 512 and not a.no_frames:
            cfg = syn.CONFIGS["C2"]
            means, quats, scales, opac = (t.to(dev) for t in syn.activate(syn.make_scene(cfg)))
            vms, K = syn.make_cameras(cfg, n_views=1).to(dev), syn.intrinsics(cfg).to(dev)
            W, H = cfg.width, cfg.height
            Fs = F[:cfg.n_gaussians]
            bs = gsbp_amd.fit_pca(Fs)
            for mode, scale in (("gaussians", 0.2), ("renderings", 1.0)):
                row["frame_" + mode] = timed(lambda: next(gsbp_amd.render_pca(means, quats, scales, opac, Fs, vms, K, W, H, mode=mode,
                                                                               basis=bs, scale=scale)), a.repeats)

            def literal():
                out = gsbp_amd.rasterization(means, quats, scales, opac, Fs, vms, K[None], W, H, want_meta=False)[0][0]
                return (out.reshape(-1, D) - bs.mean) @ bs.components.T
            row["frame_renderings_literal_wide_render"] = timed(literal, max(2, a.repeats // 2))
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        del F
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
