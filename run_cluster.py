#!/usr/bin/env python3
"""Cluster a finished feature field without prompts, clicks or examples: k-means on the HIP path (the assignment on the fp32 matrix
cores, float64 atomic-free sums), written as a codebook -- [k, D] centroids and one int32 code per Gaussian.

    python run_cluster.py --features features.pt --k 64 --out clusters/
    python run_cluster.py --features features.pt --k 256 --metric euclidean --weights d.pt --smooth-k 8 \\
        --checkpoint ckpt.pt --data-dir data/garden --frames --out clusters/
    python run_cluster.py --synthetic C1 --k 8 --iters 5 --smooth-k 4 --frames --out /tmp/clusters

--features: a .pt tensor [N, D] (or a dict with 'features').  --weights: a .pt tensor [N] of row weights (the lift's d).  Writes
codebook.pt ([k, D] float32), codes.pt ([N] int32, -1 for a zero row) and cluster.json: the inertia of every assignment, the
cluster sizes, the number of empty-cluster reseeds and the mean cosine between the rows and their centroid.  --smooth-k K passes the
codes through a majority vote over each Gaussian's K spatial neighbours (needs the scene); --frames renders every view's
render_label_argmax of the codes with a fixed seeded palette into frames/ (frame_0000.png ... when PIL imports, else frames.pt).
With --synthetic and no --features the field is a seeded one with planted clusters on the scene's Gaussians.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gsbp_amd import cli  # noqa: E402

PALETTE_SEED = 70_000
SYNTHETIC_D, SYNTHETIC_NOISE = 64, 0.3


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default=None, help=".pt tensor [N, D]: the field (or a dict with 'features')")
    ap.add_argument("--k", type=int, default=64, help="clusters")
    ap.add_argument("--metric", choices=["cosine", "euclidean"], default="cosine")
    ap.add_argument("--iters", type=int, default=25, help="assignments at most")
    ap.add_argument("--tol", type=float, default=0.0, help="stop when the inertia's relative drop is at most this")
    ap.add_argument("--init", choices=["kmeans++", "sample"], default="kmeans++")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", default=None, help=".pt tensor [N]: row weights")
    ap.add_argument("--smooth-k", type=int, default=0, help="vote the codes over this many spatial neighbours (0: off)")
    cli.add_scene_arguments(ap)
    ap.add_argument("--frames", action="store_true", help="render every view's argmax of the codes")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def palette_of(k: int) -> torch.Tensor:
    """[k, 3] in [0, 1]: seeded, the same for every run."""
    return torch.rand(k, 3, generator=torch.Generator().manual_seed(PALETTE_SEED))


def _load(path, key):
    data = torch.load(path, map_location="cpu")
    if isinstance(data, dict):
        if key not in data:
            raise SystemExit(f"{path}: expected a tensor or a dict with '{key}'")
        data = data[key]
    return data


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.synthetic and not args.features:
        ap.error("give --features (and the scene arguments for --smooth-k / --frames), or --synthetic CFG")
    need_scene = bool(args.synthetic or args.smooth_k or args.frames)
    if need_scene and not args.synthetic and not os.path.exists(args.checkpoint):
        ap.error(f"--smooth-k and --frames need the scene: --checkpoint / --data-dir ({args.checkpoint} does not exist)")
    import gsbp_amd
    cli.require_gpu("run_cluster.py")
    dev = torch.device("cuda")
    scene = cli.load_scene(args, dev).first_views(args.max_views) if need_scene else None
    if args.features:
        feats = _load(args.features, "features").to(dev)
    else:
        feats = gsbp_amd.synthetic_clusters(scene.gauss[0].shape[0], args.k, SYNTHETIC_D, SYNTHETIC_NOISE, args.seed)[0].to(dev)
    if scene is not None and feats.shape[0] != scene.gauss[0].shape[0]:
        raise SystemExit(f"--features: {feats.shape[0]} rows for {scene.gauss[0].shape[0]} Gaussians")
    weights = _load(args.weights, "weights").to(dev) if args.weights else None

    km = gsbp_amd.fit_kmeans(feats, args.k, metric=args.metric, iters=args.iters, tol=args.tol, init=args.init, seed=args.seed,
                             weights=weights)
    codes = km.labels
    report = {"n": int(feats.shape[0]), "d": int(feats.shape[1]), "k": args.k, "metric": args.metric, "init": args.init,
              "seed": args.seed, "n_iter": km.n_iter, "converged": km.converged, "history": km.history, "inertia": km.inertia,
              "reseeds": km.reseeds, "counts": km.counts.cpu().tolist(), "unassigned": int((codes < 0).sum())}
    on = codes >= 0
    x, c = feats[on].float(), km.centroids[codes[on].long()]
    cos = (x * c).sum(dim=1) / (x.norm(dim=1) * c.norm(dim=1)).clamp(min=1e-12)
    report["mean_cosine"] = float(cos.double().mean()) if int(on.sum()) else None
    if args.smooth_k:
        smoothed = gsbp_amd.smooth_labels(scene.gauss[0], codes, args.k, k=args.smooth_k)
        report["smooth_k"], report["smoothed"] = args.smooth_k, int((smoothed != codes).sum())
        codes = smoothed

    os.makedirs(args.out, exist_ok=True)
    torch.save(km.centroids.cpu(), os.path.join(args.out, "codebook.pt"))
    torch.save(codes.cpu(), os.path.join(args.out, "codes.pt"))
    with open(os.path.join(args.out, "cluster.json"), "w") as f:
        json.dump(report, f, indent=1)
    wrote = "codebook.pt, codes.pt, cluster.json"
    if args.frames:
        shade = torch.cat([torch.zeros(1, 3), palette_of(args.k)]).to(dev)  # -1 (nothing there, or an unassigned Gaussian) is black
        raster_kw = dict(camera_model=args.camera_model, rasterize_mode=args.rasterize_mode)
        writer = cli.FrameWriter(os.path.join(args.out, "frames"))
        for v in range(scene.viewmats.shape[0]):
            seg = gsbp_amd.render_label_argmax(*scene.gauss, codes, args.k, scene.viewmats[v], scene.K, scene.width, scene.height,
                                               **raster_kw)
            writer.add(v, (shade[seg.long() + 1] * 255.0).to(torch.uint8))
        writer.close()
        wrote += f", frames/ for {scene.viewmats.shape[0]} views"
    print(f"wrote {args.out}: {wrote}; {km.n_iter} assignments, inertia {km.inertia:.6g}, mean cosine {report['mean_cosine']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
