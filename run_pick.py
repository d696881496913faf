#!/usr/bin/env python3
"""From clicks to Gaussians: the Gaussians each clicked pixel is made of (csrc/pixels.hip), optionally the object around them, and
every view's id map and median depth.

    python run_pick.py --checkpoint ckpt.pt --data-dir data/garden --click 0:812,440 --click 3:640,512 --k 4 --out pick/
    python run_pick.py --checkpoint ckpt.pt --data-dir data/garden --click 0:812,440 --components --radius-factor 2 --out pick/
    python run_pick.py --synthetic C1 --click 0:200,150 --k 4 --id-maps --median-depth --out /tmp/pick

--click VIEW:X,Y (repeatable): pixel (x, y) of view VIEW.  Writes into --out: picked.pt ({'ids': int64 [U], the distinct Gaussians of
the clicks' top-k lists, heaviest first; 'clicks': int32 [C, 3] (view, x, y); 'lists': {'ids' int32 [C, k], 'weights' [C, k],
'n_contrib' [C], 'alpha' [C], 'median_id' [C], 'median_depth' [C]}}) and pick.json (the clicks, k, the picked count and the ten
heaviest ids).  With --components also mask3d.pt (bool [N]: the radius components -- --radius r, or --radius-factor f, default 2 --
that hold a picked Gaussian, through select_components).  With --id-maps / --median-depth every view's id_map_0000.pt (int32 [H, W],
-1: nothing there) / median_depth_0000.pt (float32 [H, W]).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gsbp_amd import cli  # noqa: E402

DEFAULT_FACTOR = 2.0


def parse_click(text: str):
    """'VIEW:X,Y' -> (view, x, y)."""
    try:
        view, at = text.split(":")
        x, y = at.split(",")
        return int(view), int(x), int(y)
    except ValueError:
        raise argparse.ArgumentTypeError(f"a click is VIEW:X,Y (three integers), got {text!r}")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    cli.add_scene_arguments(ap)
    ap.add_argument("--click", type=parse_click, action="append", default=None, metavar="VIEW:X,Y",
                    help="pixel (x, y) of view VIEW (repeatable)")
    ap.add_argument("--k", type=int, default=4, help="Gaussians listed per click (1..16)")
    ap.add_argument("--min-weight", type=float, default=0.0, help="list entries at or below this weight are not picked")
    ap.add_argument("--components", action="store_true", help="select the radius components of the picked Gaussians into mask3d.pt")
    reach = ap.add_mutually_exclusive_group()
    reach.add_argument("--radius", type=float, default=None, help="Gaussians this close are neighbours (--components)")
    reach.add_argument("--radius-factor", type=float, default=None,
                       help=f"the radius as a multiple of the median distance to the 8th neighbour (default {DEFAULT_FACTOR})")
    ap.add_argument("--id-maps", action="store_true", help="write every view's dominant-Gaussian id map")
    ap.add_argument("--median-depth", action="store_true", help="write every view's median depth")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.synthetic and not os.path.exists(args.checkpoint):
        ap.error(f"give --synthetic CFG, or --checkpoint / --data-dir of a scene ({args.checkpoint} does not exist)")
    if not args.click and not (args.id_maps or args.median_depth):
        ap.error("give --click VIEW:X,Y, --id-maps or --median-depth")
    import gsbp_amd
    from gsbp_amd import pixels
    cli.require_gpu("run_pick.py")
    dev = torch.device("cuda")
    scene = cli.load_scene(args, dev).first_views(args.max_views)
    n_views = scene.viewmats.shape[0]
    raster_kw = dict(camera_model=args.camera_model, rasterize_mode=args.rasterize_mode)
    os.makedirs(args.out, exist_ok=True)
    report = {"n": scene.gauss[0].shape[0], "k": args.k, "clicks": [list(c) for c in args.click or []]}
    wrote = []

    if args.click:
        for view, _, _ in args.click:
            if not 0 <= view < n_views:
                ap.error(f"--click names view {view}, the scene has views 0..{n_views - 1}")
        lists = []
        for view in sorted({c[0] for c in args.click}):  # one call per clicked view, the rows back in the clicks' order
            rows = [i for i, c in enumerate(args.click) if c[0] == view]
            xy = [[args.click[i][1], args.click[i][2]] for i in rows]
            pg = gsbp_amd.pixel_gaussians(*scene.gauss, scene.viewmats[view], scene.K, scene.width, scene.height, args.k, xy, **raster_kw)
            lists.append((torch.tensor(rows, device=dev), pg))
        back = torch.argsort(torch.cat([rows for rows, _ in lists]))
        merged = {f: torch.cat([getattr(pg, f) for _, pg in lists])[back] for f in pixels.PixelGaussians._fields}
        picked = pixels.ranked_ids(merged["ids"], merged["weights"], args.min_weight)
        torch.save({"ids": picked.cpu(), "clicks": torch.tensor(args.click, dtype=torch.int32),
                    "lists": {f: t.cpu() for f, t in merged.items()}}, os.path.join(args.out, "picked.pt"))
        report["picked"] = int(picked.shape[0])
        report["heaviest"] = picked[:10].cpu().tolist()
        wrote.append("picked.pt")
        if args.components:
            means = scene.gauss[0]
            radius = args.radius
            if radius is None:
                radius = gsbp_amd.suggest_radius(means, factor=args.radius_factor if args.radius_factor is not None else DEFAULT_FACTOR)
            comps = gsbp_amd.radius_components(means, radius)
            keep = gsbp_amd.select_components(comps, seeds=picked)
            torch.save(keep.cpu(), os.path.join(args.out, "mask3d.pt"))
            report["radius"], report["selected"] = float(radius), int(keep.sum())
            wrote.append("mask3d.pt")
    elif args.components:
        ap.error("--components needs --click")

    if args.id_maps or args.median_depth:
        for v in range(n_views):
            pg = gsbp_amd.pixel_gaussians(*scene.gauss, scene.viewmats[v], scene.K, scene.width, scene.height, 1, **raster_kw)
            if args.id_maps:
                torch.save(pg.ids[..., 0].cpu(), os.path.join(args.out, f"id_map_{v:04d}.pt"))
            if args.median_depth:
                torch.save(pg.median_depth.cpu(), os.path.join(args.out, f"median_depth_{v:04d}.pt"))
        wrote.append(f"{'id_map' if args.id_maps else ''}{' / ' if args.id_maps and args.median_depth else ''}"
                     f"{'median_depth' if args.median_depth else ''} of {n_views} views")
    with open(os.path.join(args.out, "pick.json"), "w") as f:
        json.dump(report, f, indent=1)
    wrote.append("pick.json")
    print(f"wrote {args.out}: {', '.join(wrote)}" + (f"; picked {report['picked']} Gaussians, heaviest {report['heaviest'][:3]}"
                                                      if args.click else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
