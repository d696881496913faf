#!/usr/bin/env python3
"""Clean what was decided per Gaussian with the Gaussians' spatial neighbours: per-Gaussian labels and 3-D masks by a majority vote
over the k nearest means, a field by their average, and floaters by statistical outlier removal -- on the HIP path (exact k-NN on a
uniform grid; the reference's only neighbour search is sklearn on the host, f3dgs/utils_simple_trainer.py:141-145).

    python run_clean.py --checkpoint ckpt.pt --data-dir data/garden --labels labels.pt --num-classes 12 --k 8 --out cleaned/
    python run_clean.py --checkpoint ckpt.pt --data-dir data/garden --mask mask3d.pt --remove-outliers --out cleaned/
    python run_clean.py --synthetic C1 --k 8 --remove-outliers --out /tmp/cleaned

--labels: a .pt tensor [N] (or a dict with 'labels', what run_transfer.py writes).  --mask: a .pt bool tensor [N] (or a dict with
'mask3d' / 'mask').  --features: a .pt tensor [N, D] (float32, float16 or bfloat16; --field-dtype: the smoothed one's).  Writes into --out whichever of labels.pt, mask3d.pt, features.pt were given,
cleaned; neighbors.pt ({'idx': [N, k] int32, 'dist': [N, k] float32}); and clean.json with the counts changed and removed and the
grid's statistics.  With --synthetic and no inputs: seeded labels (a Voronoi partition of space with 5 % flipped) and a seeded mask
with floaters on the scene's means.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gsbp_amd import cli  # noqa: E402

SYNTHETIC_CLASSES = 6


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    cli.add_scene_arguments(ap, only=("data-dir", "checkpoint", "format", "data-factor", "synthetic"))
    ap.add_argument("--labels", default=None, help=".pt tensor [N] of per-Gaussian labels (or a dict with 'labels')")
    ap.add_argument("--num-classes", type=int, default=None, help="labels outside [0, K) are ignored (default: max label + 1)")
    ap.add_argument("--mask", default=None, help=".pt bool tensor [N]: a 3-D mask (or a dict with 'mask3d' / 'mask')")
    ap.add_argument("--features", default=None, help=".pt tensor [N, D]: a field to average over the neighbours")
    ap.add_argument("--field-dtype", choices=("fp32", "fp16", "bf16"), default="fp32",
                    help="element type of the smoothed field in features.pt: fp16 / bf16 are the fp32 averages rounded once by the "
                         "kernel's store (no fp32 field is made); the input field is read as it is stored")
    ap.add_argument("--k", type=int, default=8, help="spatial neighbours per Gaussian, itself included (1..32)")
    ap.add_argument("--iterations", type=int, default=1, help="rounds of the vote")
    ap.add_argument("--min-fraction", type=float, default=0.5, help="a Gaussian stays in the mask with this share of neighbours in it")
    ap.add_argument("--remove-outliers", action="store_true", help="drop the mask's (or the scene's) statistical outliers")
    ap.add_argument("--std-ratio", type=float, default=2.0, help="outliers lie this many standard deviations above the mean")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def _load(path, keys):
    data = torch.load(path, map_location="cpu")
    if isinstance(data, dict):
        for key in keys:
            if key in data:
                return data[key]
        raise SystemExit(f"{path}: expected a tensor or a dict with one of {keys}")
    return data


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.synthetic and not os.path.exists(args.checkpoint):
        ap.error(f"give --synthetic CFG, or --checkpoint / --data-dir of a scene ({args.checkpoint} does not exist)")
    import gsbp_amd
    from gsbp_amd import spatial
    cli.require_gpu("run_clean.py")
    dev = torch.device("cuda")
    if args.synthetic:
        from gsbp_amd import synthetic as syn
        means = syn.make_scene(syn.CONFIGS[args.synthetic])["means"].float().to(dev)
    else:
        from gsbp_amd import scene_io
        means = scene_io.load_checkpoint(args.checkpoint, args.data_dir, format=args.format,
                                         data_factor=args.data_factor)["means"].float().to(dev)
    n = means.shape[0]
    labels = _load(args.labels, ("labels",)) if args.labels else None
    mask = _load(args.mask, ("mask3d", "mask")) if args.mask else None
    feats = _load(args.features, ("features",)) if args.features else None
    num_classes = args.num_classes
    if args.synthetic and labels is None and mask is None and feats is None:
        labels, num_classes = spatial.synthetic_labels(means, SYNTHETIC_CLASSES)[0], SYNTHETIC_CLASSES
        mask = spatial.synthetic_mask(means)[0]
    for name, t in (("labels", labels), ("mask", mask), ("features", feats)):
        if t is not None and t.shape[0] != n:
            raise SystemExit(f"--{name}: {t.shape[0]} rows for {n} Gaussians")

    dist, idx, stats = gsbp_amd.spatial_knn(means, args.k, return_stats=True)
    os.makedirs(args.out, exist_ok=True)
    torch.save({"idx": idx.cpu(), "dist": dist.cpu()}, os.path.join(args.out, "neighbors.pt"))
    report = {"n": n, "k": args.k, "iterations": args.iterations, "grid": stats}
    if labels is not None:
        from gsbp_amd.transfer import narrow_source_labels
        before, nc = narrow_source_labels(labels, num_classes)
        after = gsbp_amd.smooth_labels(means, before, nc, iterations=args.iterations, neighbors=idx)
        torch.save(after.cpu(), os.path.join(args.out, "labels.pt"))
        report["labels"] = {"num_classes": nc, "changed": int((after.cpu() != before.cpu()).sum())}
    if mask is not None:
        before = mask.to(dev).bool()
        after = gsbp_amd.smooth_mask(means, before, min_fraction=args.min_fraction, iterations=args.iterations, neighbors=idx)
        report["mask"] = {"before": int(before.sum()), "changed": int((after != before).sum()), "smoothed": int(after.sum())}
        if args.remove_outliers:
            kept = gsbp_amd.remove_outliers(means, after, k=min(args.k, 31), std_ratio=args.std_ratio)
            report["mask"]["outliers_removed"] = int(after.sum()) - int(kept.sum())
            after = kept
        report["mask"]["after"] = int(after.sum())
        torch.save(after.cpu(), os.path.join(args.out, "mask3d.pt"))
    elif args.remove_outliers:
        kept = gsbp_amd.remove_outliers(means, None, k=min(args.k, 31), std_ratio=args.std_ratio)
        report["mask"] = {"before": n, "outliers_removed": n - int(kept.sum()), "after": int(kept.sum())}
        torch.save(kept.cpu(), os.path.join(args.out, "mask3d.pt"))
    if feats is not None:
        out = gsbp_amd.smooth_features(means, feats.to(dev), neighbors=idx, out_dtype=cli.FIELD_DTYPES[args.field_dtype])
        torch.save(out.cpu(), os.path.join(args.out, "features.pt"))
        report["features"] = {"D": int(out.shape[1]), "dtype": args.field_dtype}
    with open(os.path.join(args.out, "clean.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(f"wrote {args.out}: {json.dumps({key: report[key] for key in report if key != 'grid'})}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
