#!/usr/bin/env python3
"""Split a scene into regions by geometry AND features: the connected components of the Gaussians' spatial k-NN graph with the edges
cut where the cosine of the two feature rows falls below a threshold (region growing on the HIP path: csrc/regions.hip; the
reference has nothing of the kind, its users would run a host-side graph library on a copy of the [N, D] field).

    python run_regions.py --checkpoint ckpt.pt --data-dir data/garden --features field.pt --sim-min 0.9 --min-size 200 --out reg/
    python run_regions.py --checkpoint ckpt.pt --data-dir data/garden --features field.pt --levels 0.8,0.9,0.95 --radius-factor 2 \\
        --prompts prompts.pt --frames --out reg/
    python run_regions.py --synthetic C1 --sim-min 0.9 --out /tmp/reg

--features: a .pt float tensor [N, D <= 2048] (or a dict with 'features' / 'field').  --sim-min t (default 0.9, a guess, not a tuned
value), or --levels t1,t2,...: one similarity pass and one partition per threshold; ascending thresholds refine each other, and the
LAST level is what labels, --prompts and --frames use.  --radius r or --radius-factor f (f x the median distance to the 8th
neighbour): also cut the edges longer than that.  --mask: a .pt bool tensor [N], only these Gaussians take part.  Writes into --out:
regions.pt ({'labels': int32 [N], -1 for dead rows, Gaussians outside the mask and regions below --min-size; 'sizes'; with --levels
also 'levels': int32 [L, N]}), regions.json (the thresholds, the counts, the ten largest sizes, the dead rows, the quantiles of the
valid similarities, the grid's statistics), with --prompts (a .pt dict with 'prompts' [P, D] and 'n_pos', or a tensor: all positive)
mask3d.pt (bool [N], constant per region), with --frames every view's render_label_argmax of the region ids, with
--save-similarity neighbors.pt ({'dist', 'idx'}) and similarity.pt.  With --synthetic and no --features: seeded planted regions.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gsbp_amd import cli  # noqa: E402

PALETTE_SEED = 80_000
DEFAULT_SIM_MIN = 0.9
QUANTILES = (0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99)


def _levels(text: str):
    try:
        ts = [float(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--levels wants comma-separated numbers, got {text!r}")
    if not ts or any(t != t for t in ts):
        raise argparse.ArgumentTypeError(f"--levels wants at least one threshold and no NaN, got {text!r}")
    return ts


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    cli.add_scene_arguments(ap)
    ap.add_argument("--features", default=None, help=".pt float tensor [N, D] (or a dict with 'features' / 'field')")
    ap.add_argument("--k", type=int, default=8, help="spatial neighbours per Gaussian (itself not counted), 1 .. 31")
    cut = ap.add_mutually_exclusive_group()
    cut.add_argument("--sim-min", type=float, default=None, help=f"edges need at least this cosine (default {DEFAULT_SIM_MIN}: a guess)")
    cut.add_argument("--levels", type=_levels, default=None, help="t1,t2,...: one partition per threshold from one similarity pass")
    reach = ap.add_mutually_exclusive_group()
    reach.add_argument("--radius", type=float, default=None, help="also cut the edges longer than this")
    reach.add_argument("--radius-factor", type=float, default=None,
                       help="the radius as a multiple of the median distance to the 8th neighbour")
    ap.add_argument("--mask", default=None, help=".pt bool tensor [N]: only these Gaussians take part (or a dict with 'mask3d' / 'mask')")
    ap.add_argument("--min-size", type=int, default=1, help="regions with fewer members are dropped")
    ap.add_argument("--prompts", default=None, help=".pt dict with 'prompts' [P, D] and 'n_pos' (or a tensor: all positive)")
    ap.add_argument("--frames", action="store_true", help="render every view's argmax of the region ids")
    ap.add_argument("--save-similarity", action="store_true", help="also write neighbors.pt and similarity.pt")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def check_args(ap: argparse.ArgumentParser, args) -> None:
    """The argument checks that need no device."""
    if not args.synthetic and not os.path.exists(args.checkpoint):
        ap.error(f"give --synthetic CFG, or --checkpoint / --data-dir of a scene ({args.checkpoint} does not exist)")
    if not args.synthetic and not args.features:
        ap.error("give --features")
    if not 1 <= args.k <= 31:
        ap.error(f"--k must be in [1, 31], got {args.k}")
    if args.sim_min is not None and args.sim_min != args.sim_min:
        ap.error("--sim-min must not be NaN")
    if args.min_size < 1:
        ap.error(f"--min-size must be at least 1, got {args.min_size}")
    for name in ("radius", "radius_factor"):
        v = getattr(args, name)
        if v is not None and not (0.0 <= v < float("inf")):
            ap.error(f"--{name.replace('_', '-')} must be finite and >= 0, got {v}")


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
    check_args(ap, args)
    import gsbp_amd
    from gsbp_amd import regions
    cli.require_gpu("run_regions.py")
    dev = torch.device("cuda")
    scene = cli.load_scene(args, dev).first_views(args.max_views)
    means = scene.gauss[0]
    n = means.shape[0]
    feats = _load(args.features, ("features", "field")) if args.features else regions.synthetic_regions(means)[0]
    if feats.dim() != 2 or feats.shape[0] != n:
        raise SystemExit(f"--features: shape {tuple(feats.shape)} for {n} Gaussians")
    feats = feats.to(dev)
    mask = None
    if args.mask:
        mask = _load(args.mask, ("mask3d", "mask")).bool()
        if mask.dim() != 1 or mask.shape[0] != n:
            raise SystemExit(f"--mask: shape {tuple(mask.shape)} for {n} Gaussians")
        mask = mask.to(dev)

    dist, idx, grid = gsbp_amd.spatial_knn(means, min(args.k + 1, n), return_stats=True)
    radius = args.radius
    if radius is None and args.radius_factor is not None:
        radius = gsbp_amd.suggest_radius(means, factor=args.radius_factor, mask=mask)
    thresholds = args.levels if args.levels else [args.sim_min if args.sim_min is not None else DEFAULT_SIM_MIN]
    sim, live = gsbp_amd.neighbor_similarity(feats, idx)  # the one pass over the [N, D] field; every level below is integer work
    levels = gsbp_amd.similarity_levels(means, feats, thresholds, radius=radius, mask=mask, neighbors=(dist, idx), similarity=(sim, live),
                                        min_size=args.min_size)
    labels = levels[-1]
    sizes = torch.bincount(labels[labels >= 0].long())
    core = live if mask is None else live & mask

    os.makedirs(args.out, exist_ok=True)
    saved = {"labels": labels.cpu(), "sizes": sizes.cpu()}
    if args.levels:
        saved["levels"] = levels.cpu()
    torch.save(saved, os.path.join(args.out, "regions.pt"))
    n_reg = int(sizes.shape[0])
    quant = regions.similarity_quantiles(sim, QUANTILES)
    report = {"n": n, "k": int(idx.shape[1]) - 1, "thresholds": thresholds, "radius": radius, "min_size": args.min_size,
              "regions": n_reg, "in_regions": int((labels >= 0).sum()), "live": int(core.sum()), "dead_rows": n - int(live.sum()),
              "largest": sizes.sort(descending=True).values[:10].cpu().tolist(),
              "similarity_quantiles": dict(zip((str(q) for q in QUANTILES), quant)),
              "valid_similarities": int((~torch.isnan(sim)).sum()), "grid": grid}
    if args.levels:
        report["regions_per_level"] = [int(row.max()) + 1 for row in levels]
    wrote = "regions.pt, regions.json"
    if args.prompts:
        data = torch.load(args.prompts, map_location="cpu")
        prompts, n_pos = (data["prompts"], int(data.get("n_pos", data["prompts"].shape[0]))) if isinstance(data, dict) else \
            (data, int(data.shape[0]))
        keep = gsbp_amd.region_prompt_mask(feats, labels, prompts.float().to(dev), n_pos)
        torch.save(keep.cpu(), os.path.join(args.out, "mask3d.pt"))
        report["selected"] = int(keep.sum())
        wrote += ", mask3d.pt"
    if args.save_similarity:
        torch.save({"dist": dist.cpu(), "idx": idx.cpu()}, os.path.join(args.out, "neighbors.pt"))
        torch.save(sim.cpu(), os.path.join(args.out, "similarity.pt"))
        wrote += ", neighbors.pt, similarity.pt"
    with open(os.path.join(args.out, "regions.json"), "w") as f:
        json.dump(report, f, indent=1)
    if args.frames:
        c = max(n_reg, 1)
        palette = torch.rand(c, 3, generator=torch.Generator().manual_seed(PALETTE_SEED))
        shade = torch.cat([torch.zeros(1, 3), palette]).to(dev)  # -1 (nothing there, or a Gaussian in no region) is black
        raster_kw = dict(camera_model=args.camera_model, rasterize_mode=args.rasterize_mode)
        writer = cli.FrameWriter(os.path.join(args.out, "frames"))
        for v in range(scene.viewmats.shape[0]):
            seg = gsbp_amd.render_label_argmax(*scene.gauss, labels, c, scene.viewmats[v], scene.K, scene.width, scene.height,
                                               **raster_kw)
            writer.add(v, (shade[seg.long() + 1] * 255.0).to(torch.uint8))
        writer.close()
        wrote += f", frames/ for {scene.viewmats.shape[0]} views"
    print(f"wrote {args.out}: {wrote}; thresholds {thresholds}, {n_reg} regions, largest {report['largest'][:3]}, "
          f"dead rows {report['dead_rows']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
