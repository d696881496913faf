#!/usr/bin/env python3
"""Split a 3-D mask or a per-Gaussian label field into instances: the connected components of the Gaussians' means under "within a
radius of each other, and of the same class" (DBSCAN with a deterministic border rule, on the HIP path: csrc/components.hip; the
reference would run sklearn on a host copy, as for its only neighbour search, f3dgs/utils_simple_trainer.py:141-145).

    python run_instances.py --checkpoint ckpt.pt --data-dir data/garden --mask mask3d.pt --radius-factor 2 --min-size 200 --out inst/
    python run_instances.py --checkpoint ckpt.pt --data-dir data/garden --labels labels.pt --num-classes 12 --radius 0.05 \\
        --min-points 4 --keep-largest 3 --frames --out inst/
    python run_instances.py --synthetic C1 --radius-factor 2 --min-size 50 --seed-index 17 --out /tmp/inst

--mask: a .pt bool tensor [N] (or a dict with 'mask3d' / 'mask').  --labels: a .pt integer tensor [N] (or a dict with 'labels');
labels outside [0, --num-classes) are dropped and two classes never merge.  --radius r, or --radius-factor f (default 2): f x the
median distance to the 8th neighbour within the mask / the labelled Gaussians.  Writes into --out: instances.pt ({'instances': int32
[N], ids by descending size, -1 for noise and for components below --min-size; 'sizes'; 'classes'; 'core'}), instances.json (the
radius used, the counts, the ten largest sizes, the noise count, the grid's statistics), with --keep-largest / --seed-index also
mask3d.pt (bool [N]: the union of the n biggest instances and of the instances that hold the seed Gaussians), and with --frames
every view's render_label_argmax of the instance ids.  With --synthetic and no input: a seeded mask of three balls and floaters.
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
DEFAULT_FACTOR = 2.0


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    cli.add_scene_arguments(ap)
    what = ap.add_mutually_exclusive_group()
    what.add_argument("--mask", default=None, help=".pt bool tensor [N]: a 3-D mask (or a dict with 'mask3d' / 'mask')")
    what.add_argument("--labels", default=None, help=".pt integer tensor [N] of per-Gaussian labels (or a dict with 'labels')")
    ap.add_argument("--num-classes", type=int, default=None, help="labels outside [0, K) are dropped (default: max label + 1)")
    reach = ap.add_mutually_exclusive_group()
    reach.add_argument("--radius", type=float, default=None, help="Gaussians this close are neighbours")
    reach.add_argument("--radius-factor", type=float, default=None,
                       help=f"the radius as a multiple of the median distance to the 8th neighbour (default {DEFAULT_FACTOR})")
    ap.add_argument("--min-points", type=int, default=1, help="neighbours (itself included) that make a Gaussian a core point")
    ap.add_argument("--min-size", type=int, default=1, help="components with fewer members are dropped")
    ap.add_argument("--keep-largest", type=int, default=None, help="select the n biggest instances into mask3d.pt")
    ap.add_argument("--seed-index", type=int, action="append", default=None, help="select the instance of this Gaussian (repeatable)")
    ap.add_argument("--frames", action="store_true", help="render every view's argmax of the instance ids")
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
    if not args.synthetic and not (args.mask or args.labels):
        ap.error("give --mask or --labels")
    import gsbp_amd
    from gsbp_amd import components
    cli.require_gpu("run_instances.py")
    dev = torch.device("cuda")
    scene = cli.load_scene(args, dev).first_views(args.max_views)
    means = scene.gauss[0]
    n = means.shape[0]
    if args.mask:
        what = _load(args.mask, ("mask3d", "mask")).bool()
    elif args.labels:
        what = _load(args.labels, ("labels",)).long()
    else:
        what = components.synthetic_instances(means)[0]
    if what.dim() != 1 or what.shape[0] != n:
        raise SystemExit(f"--mask / --labels: shape {tuple(what.shape)} for {n} Gaussians")
    what = what.to(dev)

    if what.dtype == torch.bool:
        live = what
    else:
        live = (what >= 0) & (what < (args.num_classes if args.num_classes is not None else int(what.max()) + 1))
    radius = args.radius
    if radius is None:
        radius = gsbp_amd.suggest_radius(means, factor=args.radius_factor if args.radius_factor is not None else DEFAULT_FACTOR, mask=live)
    inst = gsbp_amd.split_instances(means, what, radius, args.min_points, args.min_size, args.num_classes)

    os.makedirs(args.out, exist_ok=True)
    torch.save({"instances": inst.instances.cpu(), "sizes": inst.sizes.cpu(), "classes": inst.classes.cpu(), "core": inst.core.cpu()},
               os.path.join(args.out, "instances.pt"))
    n_inst = int(inst.sizes.shape[0])
    live_n = int(live.sum())
    report = {"n": n, "live": live_n, "radius": inst.radius, "min_points": args.min_points, "min_size": args.min_size,
              "instances": n_inst, "in_instances": int((inst.instances >= 0).sum()), "core": int(inst.core.sum()),
              "largest": inst.sizes[:10].cpu().tolist(), "noise": live_n - int((inst.instances >= 0).sum()), "grid": inst.grid_stats}
    wrote = "instances.pt, instances.json"
    if args.keep_largest is not None or args.seed_index:
        keep = gsbp_amd.select_components(inst, seeds=args.seed_index, largest=args.keep_largest)
        torch.save(keep.cpu(), os.path.join(args.out, "mask3d.pt"))
        report["selected"] = int(keep.sum())
        wrote += ", mask3d.pt"
    with open(os.path.join(args.out, "instances.json"), "w") as f:
        json.dump(report, f, indent=1)
    if args.frames:
        k = max(n_inst, 1)
        palette = torch.rand(k, 3, generator=torch.Generator().manual_seed(PALETTE_SEED))
        shade = torch.cat([torch.zeros(1, 3), palette]).to(dev)  # -1 (nothing there, or a Gaussian in no instance) is black
        raster_kw = dict(camera_model=args.camera_model, rasterize_mode=args.rasterize_mode)
        writer = cli.FrameWriter(os.path.join(args.out, "frames"))
        for v in range(scene.viewmats.shape[0]):
            seg = gsbp_amd.render_label_argmax(*scene.gauss, inst.instances, k, scene.viewmats[v], scene.K, scene.width, scene.height,
                                               **raster_kw)
            writer.add(v, (shade[seg.long() + 1] * 255.0).to(torch.uint8))
        writer.close()
        wrote += f", frames/ for {scene.viewmats.shape[0]} views"
    print(f"wrote {args.out}: {wrote}; radius {inst.radius:.6g}, {n_inst} instances, largest {report['largest'][:3]}, "
          f"noise {report['noise']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
