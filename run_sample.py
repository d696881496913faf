#!/usr/bin/env python3
"""Ask a finished field at arbitrary 3-D points: the vertices of a benchmark's mesh, a sensor's cloud, COLMAP's sparse points, or the
Gaussians of a re-trained scene of the same place.  Every point gets the k Gaussians of largest weight by their own scale, rotation
and opacity (the HIP path: csrc/sample.hip), the field blended over them and the weighted vote of their labels.

    python run_sample.py --checkpoint ckpt.pt --data-dir data/garden --colmap-points --features field.pt --out smp/
    python run_sample.py --checkpoint ckpt.pt --data-dir data/garden --points mesh_vertices.pt --labels labels.pt --num-classes 20 \\
        --gt vertex_labels.pt --out smp/
    python run_sample.py --checkpoint ckpt.pt --data-dir data/garden --scene-points retrained.ply --features field.pt \\
        --fallback nearest --out smp/
    python run_sample.py --synthetic C1 --num-classes 6 --out /tmp/smp

--points: a .pt float tensor [Q, 3] (or a dict with 'points' / 'means' / 'xyz'); --colmap-points: the scene's points3D.bin;
--scene-points: the means of another checkpoint (.pt with 'splats', or a 3DGS .ply).  --features: a .pt float tensor [N, D] (or a
dict with 'features' / 'field'); --labels: a .pt integer tensor [N] (or a dict with 'labels') with --num-classes; --gt: integer [Q]
ground truth for the points (-1: not scored).  --radius r, or --radius-quantile q (default 0.99) of the Gaussians' reach; --mask: a
.pt bool tensor [N], only these Gaussians take part; --fallback nearest: a point where no Gaussian counts takes the field of the
Gaussian with the nearest centre; --out-dtype fp16 | bf16: the sampled features in half.  Writes into --out: sampled_features.pt ({'features' [Q, D], 'valid' [Q], 'wsum' [Q]}),
sampled_labels.pt ({'labels' int32 [Q], 'share' [Q]}), point_gaussians.pt ({'idx', 'weights', 'n_contrib', 'points'}), sample.json
(the radius, the valid / truncated / fallback counts, the quantiles of n_contrib and wsum, the share of Gaussians whose reach
exceeds the radius, the grid's statistics) and with --gt metrics.json (miou_recall of the points' counts).  With --synthetic and no
inputs: seeded points, the seeded planted-region field of run_regions.py, seeded Voronoi labels, and the points' own ground truth.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gsbp_amd import cli  # noqa: E402

QUANTILES = (0.0, 0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    cli.add_scene_arguments(ap, only=("data-dir", "checkpoint", "format", "data-factor", "synthetic"))
    where = ap.add_mutually_exclusive_group()
    where.add_argument("--points", default=None, help=".pt float tensor [Q, 3] (or a dict with 'points' / 'means' / 'xyz')")
    where.add_argument("--colmap-points", action="store_true", help="the scene's COLMAP sparse points (points3D.bin)")
    where.add_argument("--scene-points", default=None, help="the means of another checkpoint (.pt with 'splats') or 3DGS .ply")
    ap.add_argument("--features", default=None, help=".pt float tensor [N, D] (or a dict with 'features' / 'field')")
    ap.add_argument("--labels", default=None, help=".pt integer tensor [N] (or a dict with 'labels'); needs --num-classes")
    ap.add_argument("--num-classes", type=int, default=None)
    ap.add_argument("--gt", default=None, help=".pt integer tensor [Q]: the points' ground truth, -1 = not scored")
    ap.add_argument("--k", type=int, default=8, help="Gaussians kept per point, 1 .. 32")
    reach = ap.add_mutually_exclusive_group()
    reach.add_argument("--radius", type=float, default=None, help="search the centres within this distance of a point")
    reach.add_argument("--radius-quantile", type=float, default=None, help="... or within this quantile of the Gaussians' reach (0.99)")
    ap.add_argument("--alpha-min", type=float, default=None, help="the smallest weight that counts (default 1/255, the blend's)")
    ap.add_argument("--mask", default=None, help=".pt bool tensor [N]: only these Gaussians take part (or a dict with 'mask3d' / 'mask')")
    ap.add_argument("--fallback", choices=["nearest"], default=None, help="fill the points where no Gaussian counts")
    ap.add_argument("--out-dtype", choices=("fp32", "fp16", "bf16"), default="fp32",
                    help="element type of the sampled features: fp16 / bf16 are the fp32 rows rounded once by the kernel's store")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def check_args(ap: argparse.ArgumentParser, args) -> None:
    """The argument checks that need no device."""
    if not args.synthetic and not os.path.exists(args.checkpoint):
        ap.error(f"give --synthetic CFG, or --checkpoint / --data-dir of a scene ({args.checkpoint} does not exist)")
    if not args.synthetic and not (args.points or args.colmap_points or args.scene_points):
        ap.error("give --points, --colmap-points or --scene-points")
    if not args.synthetic and not (args.features or args.labels):
        ap.error("give --features or --labels")
    if not 1 <= args.k <= 32:
        ap.error(f"--k must be in [1, 32], got {args.k}")
    if args.radius is not None and not (0.0 <= args.radius < float("inf")):
        ap.error(f"--radius must be finite and >= 0, got {args.radius}")
    if args.radius_quantile is not None and not (0.0 <= args.radius_quantile <= 1.0):
        ap.error(f"--radius-quantile must be in [0, 1], got {args.radius_quantile}")
    if args.alpha_min is not None and not (1e-30 <= args.alpha_min <= 1.0):
        ap.error(f"--alpha-min must be in [1e-30, 1], got {args.alpha_min}")
    if args.labels and args.num_classes is None:
        ap.error("--labels needs --num-classes")
    if args.num_classes is not None and args.num_classes < 1:
        ap.error(f"--num-classes must be at least 1, got {args.num_classes}")


def _load(path, keys):
    data = torch.load(path, map_location="cpu")
    if isinstance(data, dict):
        for key in keys:
            if key in data:
                return data[key]
        raise SystemExit(f"{path}: expected a tensor or a dict with one of {keys}")
    return data


def _other_means(path):
    from gsbp_amd import scene_io
    if path.endswith(".ply"):
        return scene_io.read_gaussian_ply(path)["means"]
    data = torch.load(path, map_location="cpu", weights_only=False)
    return data["splats"]["means"] if isinstance(data, dict) and "splats" in data else _load(path, ("means",))


def _quantiles(values):
    from gsbp_amd.regions import similarity_quantiles
    return dict(zip((str(q) for q in QUANTILES), similarity_quantiles(values.double(), QUANTILES)))


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    check_args(ap, args)
    import gsbp_amd
    from gsbp_amd import regions, sample, spatial
    cli.require_gpu("run_sample.py")
    dev = torch.device("cuda")
    args.camera_model, args.rasterize_mode, args.max_views = "pinhole", "classic", None
    scene = cli.load_scene(args, dev)
    means, quats, scales, opacities = scene.gauss
    n = means.shape[0]

    gt = None
    if args.points:
        points = _load(args.points, ("points", "means", "xyz")).float()
    elif args.colmap_points:
        proj = scene.splats.get("colmap_project")
        if proj is None or proj.points3D is None:
            raise SystemExit("--colmap-points: the scene has no points3D.bin")
        points = torch.from_numpy(proj.points3D).float()
    elif args.scene_points:
        points = _other_means(args.scene_points).float()
    else:
        points = sample.synthetic_points(means)
    if points.dim() != 2 or points.shape[1] != 3:
        raise SystemExit(f"the points must be [Q, 3], got {tuple(points.shape)}")
    points = points.to(dev)
    nq = points.shape[0]

    feats = labels = None
    num_classes = args.num_classes
    if args.features:
        feats = _load(args.features, ("features", "field"))  # (fp16 / bf16 fields are sampled as stored)
    if args.labels:
        labels = _load(args.labels, ("labels",))
    if args.synthetic and feats is None and labels is None:
        feats = regions.synthetic_regions(means)[0]
        num_classes = num_classes if num_classes is not None else 6
        labels = spatial.synthetic_labels(means, num_classes)[1]
        if not args.gt:  # the points' own ground truth: the class of the Gaussian with the nearest centre
            near = gsbp_amd.spatial_knn(means, 1, queries=points)[1][:, 0].long()
            gt = torch.where(near >= 0, labels[near.clamp(min=0)], torch.full_like(near, -1))
    if feats is not None and (feats.dim() != 2 or feats.shape[0] != n):
        raise SystemExit(f"--features: shape {tuple(feats.shape)} for {n} Gaussians")
    if labels is not None and (labels.dim() != 1 or labels.shape[0] != n or labels.dtype.is_floating_point):
        raise SystemExit(f"--labels: an integer tensor [{n}] is needed, got {tuple(labels.shape)} {labels.dtype}")
    if args.gt:
        gt = _load(args.gt, ("labels", "gt"))
        if gt.dim() != 1 or gt.shape[0] != nq or gt.dtype.is_floating_point:
            raise SystemExit(f"--gt: an integer tensor [{nq}] is needed, got {tuple(gt.shape)} {gt.dtype}")
    mask = None
    if args.mask:
        mask = _load(args.mask, ("mask3d", "mask")).bool()
        if mask.dim() != 1 or mask.shape[0] != n:
            raise SystemExit(f"--mask: shape {tuple(mask.shape)} for {n} Gaussians")
        mask = mask.to(dev)

    alpha_min = args.alpha_min if args.alpha_min is not None else sample.ALPHA_MIN
    pg = gsbp_amd.point_gaussians(points, means, quats, scales, opacities, args.k, args.radius, alpha_min, mask,
                                  quantile=args.radius_quantile if args.radius_quantile is not None else 0.99, return_visited=True)
    os.makedirs(args.out, exist_ok=True)
    torch.save({"idx": pg.idx.cpu(), "weights": pg.weights.cpu(), "n_contrib": pg.n_contrib.cpu(), "points": points.cpu()},
               os.path.join(args.out, "point_gaussians.pt"))
    wrote = "point_gaussians.pt, sample.json"
    wsum = pg.weights.sum(dim=1)
    valid = pg.n_contrib > 0
    finite = torch.isfinite(points).all(dim=1)
    report = {"n": n, "points": nq, "finite_points": int(finite.sum()), "k": args.k, "radius": pg.radius, "alpha_min": alpha_min,
              "valid": int(valid.sum()), "truncated": int((pg.n_contrib > args.k).sum()), "fallback": 0,
              "n_contrib_quantiles": _quantiles(pg.n_contrib), "visited_mean": float(pg.visited.double().mean()) if nq else 0.0,
              "beyond_radius": pg.beyond_radius, "grid": pg.grid_stats}
    if feats is not None:
        out, ok, wsum = gsbp_amd.sample_field(feats.to(dev), pg, args.fallback or "none", return_wsum=True,
                                              out_dtype=cli.FIELD_DTYPES[args.out_dtype])
        if args.fallback:
            report["fallback"] = sample.fallback_rows(pg, ok)
        torch.save({"features": out.cpu(), "valid": ok.cpu(), "wsum": wsum.cpu()}, os.path.join(args.out, "sampled_features.pt"))
        wrote += ", sampled_features.pt"
    report["wsum_quantiles"] = _quantiles(wsum[valid]) if bool(valid.any()) else {}
    if labels is not None:
        lab, share = gsbp_amd.sample_labels(labels.to(dev), num_classes, pg)
        torch.save({"labels": lab.cpu(), "share": share.cpu()}, os.path.join(args.out, "sampled_labels.pt"))
        report["labelled"] = int((lab >= 0).sum())
        wrote += ", sampled_labels.pt"
        if gt is not None:
            counts = gsbp_amd.score_point_labels(lab, gt.to(dev), num_classes)
            metrics = gsbp_amd.miou_recall(counts, classes=list(range(num_classes)))
            metrics["counts"] = counts.cpu().tolist()
            metrics = {k: ({str(c): v for c, v in val.items()} if isinstance(val, dict) else val) for k, val in metrics.items()}
            metrics = {k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in metrics.items()}
            with open(os.path.join(args.out, "metrics.json"), "w") as f:
                json.dump(metrics, f, indent=1)
            wrote += ", metrics.json"
    with open(os.path.join(args.out, "sample.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(f"wrote {args.out}: {wrote}; {nq} points, radius {pg.radius:.4g}, valid {report['valid']}, truncated {report['truncated']}, "
          f"fallback {report['fallback']}, beyond radius {pg.beyond_radius:.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
