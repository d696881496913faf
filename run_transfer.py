#!/usr/bin/env python3
"""Command-line counterpart of the reference's transfer_affordance (affordance_transfer/demo_affordance_transfer.py:1377-1396):
labels for every Gaussian of a finished feature field from a small set of labelled example features, by exact inner-product
k-NN search and a majority vote, on the HIP path.

    python run_transfer.py --features results/features_dino.pt --examples results/features_and_labels.pkl --k 5 --out labels.pt
    python run_transfer.py --synthetic --out /tmp/labels.pt --counts

--features: a .pt tensor [N, D] (what run_backproject.py writes).  --examples: a .pt or .npz with `features` [M, D] and `labels`
[M] or [M, 1], or the reference's features_and_labels.pkl.  Writes {'labels': [N] int32, 'k', 'num_classes'} and, with --counts,
'counts': [N, num_classes] int32.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gsbp_amd import cli  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default=None, help=".pt tensor [N, D]: the finished feature field")
    ap.add_argument("--examples", default=None, help=".pt / .npz / .pkl with 'features' [M, D] and 'labels' [M] or [M, 1]")
    ap.add_argument("--k", type=int, default=5, help="neighbours per Gaussian (the reference uses 5; 1..32)")
    ap.add_argument("--num-classes", type=int, default=None, help="labels outside [0, K) are ignored (default: max label + 1)")
    ap.add_argument("--out", default="labels.pt")
    ap.add_argument("--counts", action="store_true", help="also write the per-class neighbour counts [N, K]")
    ap.add_argument("--synthetic", action="store_true",
                    help="a seeded field and example set (transfer.synthetic_transfer) instead of files")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.synthetic and not (args.features and args.examples):
        ap.error("give --features and --examples, or --synthetic")
    import gsbp_amd
    from gsbp_amd import transfer
    cli.require_gpu("run_transfer.py")
    dev = torch.device("cuda")
    if args.synthetic:
        feats, src, labels = transfer.synthetic_transfer()
    else:
        feats = torch.load(args.features, map_location="cpu")
        src, labels = transfer.load_examples(args.examples)
    lab, nc = transfer.narrow_source_labels(labels, args.num_classes)
    res = gsbp_amd.transfer_labels(feats.to(dev), src.to(dev), lab, k=args.k, num_classes=nc, return_counts=args.counts)
    out = {"k": args.k, "num_classes": nc}
    if args.counts:
        out["labels"], out["counts"] = res[0].cpu(), res[1].cpu()
    else:
        out["labels"] = res.cpu()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    torch.save(out, args.out)
    print(f"wrote {args.out}: {out['labels'].shape[0]} labels, k = {args.k}, {nc} classes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
