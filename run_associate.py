#!/usr/bin/env python3
"""Associate per-view instance masks whose ids are unrelated between the views (an "everything" segmenter run on each image by
itself: automatic masks, superpixels) into consistent 3-D groups, training-free, on the HIP path (csrc/associate.hip: an integer
overlap table and integer votes per view straight from the blend's weight store; gsbp_amd.associate_masks).  The reference gets
consistent ids only by tracking one box prompt through the frames with a video predictor
(affordance_transfer/demo_affordance_transfer.py:302-328).

    python run_associate.py --checkpoint ckpt.pt --data-dir data/garden --masks masks/ --max-masks 256 --out assoc/
    python run_associate.py --checkpoint ckpt.pt --data-dir data/garden --masks masks/ --pixel-weights conf/ --frames --out assoc/
    python run_backproject.py --checkpoint ckpt.pt --data-dir data/garden --label-maps assoc/maps --num-classes <n_groups> ...
    python run_associate.py --synthetic C1 --out /tmp/assoc

--masks DIR: <image name>.pt integer tensors [H, W] (another shape is a low-resolution map, read with mode='nearest'), ids in
[0, --max-masks), anything else ignored.  --pixel-weights DIR: <image name>.pt [H, W] weight maps (bool, uint8, float) that weight
every pixel's evidence.  Writes into --out: association.pt ({'maps': int32 [V, max_masks] mask id -> group id or -1, 'groups':
int32 [N], 'n_groups'}), maps/<image name>.pt (every view's map renamed to group ids, int32, the layout run_backproject.py
--label-maps reads), associate.json (the parameters, the per-view table of matched / opened / dropped / dead masks and the share of
weight on Gaussians without a group, the group sizes), with --save-votes votes.pt (int64 [N, max_groups] fixed-point evidence,
8 * N * max_groups bytes) and with --frames every view's render_label_argmax of the groups.  With --synthetic and no --masks: seeded
instance maps with ids permuted per view (synthetic.make_instance_views).  The defaults --iou-min 0.2 and --min-mass 1.0 come from
one synthetic scene and are not tuned on real segmenter output.

--votes sparse [--slots S] [--on-overflow raise]: the evidence in S slots per Gaussian instead of the dense table.  association.pt
then also carries 'keys' int32 [N, S], 'vals' int64 [N, S], 'spill' int64 [N] and 'certain' bool [N]; associate.json gains
'sparse_votes': the overflowed rows, the spilled share, the histogram of slots in use.
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
SYNTHETIC_INSTANCES = 6


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    cli.add_scene_arguments(ap, max_views_help="associate only the first views")
    ap.add_argument("--masks", default=None, help="directory with <image name>.pt INTEGER tensors [H,W]: every view's instance ids")
    ap.add_argument("--max-masks", type=int, default=None, help="ids lie in [0, K); anything else is ignored (default 256; with "
                                                                  f"--synthetic and no --masks {SYNTHETIC_INSTANCES})")
    ap.add_argument("--max-groups", type=int, default=256, help="3-D groups at most; masks that would open more are dropped")
    ap.add_argument("--iou-min", type=float, default=0.2, help="a mask continues a group from this IoU in weight space on")
    ap.add_argument("--min-mass", type=float, default=1.0, help="masks with less blend weight than this are ignored")
    ap.add_argument("--pixel-weights", default=None, help="directory with <image name>.pt [H,W] per-pixel weight maps")
    ap.add_argument("--frames", action="store_true", help="render every view's argmax of the groups")
    ap.add_argument("--save-votes", action="store_true", help="also write votes.pt, int64 [N, max_groups]")
    ap.add_argument("--votes", choices=["dense", "sparse"], default="dense",
                    help="sparse: the evidence in --slots (group, sum) slots per Gaussian instead of a dense [N, max_groups] table: "
                         "N * (12 * slots + 8) bytes whatever --max-groups, which may then be 65536")
    ap.add_argument("--slots", type=int, default=8, help="slots per Gaussian of --votes sparse (1 .. 32)")
    ap.add_argument("--on-overflow", choices=["warn", "raise"], default="warn",
                    help="--votes sparse: a Gaussian that has received more than --slots distinct groups spills; warn once and go "
                         "on (the later decisions may then differ from run to run), or stop at the first such view")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def _load_map(directory: str, name: str, integer: bool) -> torch.Tensor:
    t = torch.load(os.path.join(directory, name + ".pt"), map_location="cpu")
    if not torch.is_tensor(t) or t.dim() != 2 or (integer and (t.is_floating_point() or t.is_complex())):
        raise SystemExit(f"{name}.pt in {directory}: a 2-D {'integer ' if integer else ''}tensor is required")
    return t


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.synthetic and not os.path.exists(args.checkpoint):
        ap.error(f"give --synthetic CFG, or --checkpoint / --data-dir of a scene ({args.checkpoint} does not exist)")
    if not args.synthetic and not args.masks:
        ap.error("give --masks DIR")
    import gsbp_amd
    from gsbp_amd import synthetic as syn
    cli.require_gpu("run_associate.py")
    dev = torch.device("cuda")
    scene = cli.load_scene(args, dev).first_views(args.max_views)
    n, n_views, W, H = scene.gauss[0].shape[0], scene.viewmats.shape[0], scene.width, scene.height
    upsample = None
    if args.masks:
        max_masks = args.max_masks if args.max_masks is not None else 256
        if tuple(_load_map(args.masks, scene.names[0], True).shape) != (H, W):
            upsample = "nearest"

        def mask_fn(v):
            return _load_map(args.masks, scene.names[v], True).to(dev)
    else:
        max_masks = args.max_masks if args.max_masks is not None else SYNTHETIC_INSTANCES
        _, synthetic_maps, _ = syn.make_instance_views(scene.cfg, scene.viewmats, min(SYNTHETIC_INSTANCES, max_masks), n_ids=max_masks,
                                                       device=dev)

        def mask_fn(v):
            return synthetic_maps[v]
    weight_fn = None
    if args.pixel_weights:
        def weight_fn(v):
            c = _load_map(args.pixel_weights, scene.names[v], False).to(dev)
            return c if c.dtype in (torch.bool, torch.uint8, torch.float16, torch.bfloat16, torch.float32) else c.float()
    raster_kw = dict(camera_model=args.camera_model, rasterize_mode=args.rasterize_mode)
    assoc = gsbp_amd.associate_masks(*scene.gauss, scene.viewmats, scene.K, W, H, mask_fn, max_masks, max_groups=args.max_groups,
                                     iou_min=args.iou_min, min_mass=args.min_mass, pixel_weight_fn=weight_fn, upsample=upsample,
                                     votes=args.votes, slots=args.slots, on_overflow=args.on_overflow, **raster_kw)
    sparse = args.votes == "sparse"

    os.makedirs(os.path.join(args.out, "maps"), exist_ok=True)
    saved = {"maps": torch.stack(assoc.maps).cpu(), "groups": assoc.groups.cpu(), "n_groups": assoc.n_groups}
    if sparse:  # the lists are small: they always go along (canonical order; keys -1 = empty)
        saved.update(keys=assoc.votes.keys.cpu(), vals=assoc.votes.vals.cpu(), spill=assoc.votes.spill.cpu())
        saved["certain"] = gsbp_amd.sparse_votes_groups(assoc.votes)[1].cpu()
    torch.save(saved, os.path.join(args.out, "association.pt"))
    for v in range(n_views):
        torch.save(gsbp_amd.remap_masks(mask_fn(v), assoc.maps[v]).cpu(), os.path.join(args.out, "maps", scene.names[v] + ".pt"))
    sizes = torch.bincount(assoc.groups[assoc.groups >= 0].long(), minlength=max(assoc.n_groups, 1))[:max(assoc.n_groups, 0)]
    report = {"n": n, "views": n_views, "max_masks": max_masks, "max_groups": args.max_groups, "iou_min": args.iou_min,
              "min_mass": args.min_mass, "upsample": upsample, "pixel_weights": bool(args.pixel_weights), "n_groups": assoc.n_groups,
              "grouped": int((assoc.groups >= 0).sum()), "group_sizes": sizes.cpu().tolist(), "per_view": assoc.views,
              "votes": args.votes}
    if sparse:
        report["sparse_votes"] = gsbp_amd.sparse_votes_stats(assoc.votes)
    with open(os.path.join(args.out, "associate.json"), "w") as f:
        json.dump(report, f, indent=1)
    wrote = "association.pt, maps/, associate.json"
    if args.save_votes:
        if sparse and assoc.n_groups > 4096:
            raise SystemExit(f"--save-votes would densify {assoc.n_groups} groups: the lists are in association.pt")
        dense = gsbp_amd.sparse_votes_dense(assoc.votes, max(assoc.n_groups, 1)) if sparse else assoc.votes
        torch.save(dense.cpu(), os.path.join(args.out, "votes.pt"))
        wrote += ", votes.pt"
    if args.frames:
        k = max(assoc.n_groups, 1)
        palette = torch.rand(k, 3, generator=torch.Generator().manual_seed(PALETTE_SEED))
        shade = torch.cat([torch.zeros(1, 3), palette]).to(dev)  # -1 (nothing there, or a Gaussian without a group) is black
        writer = cli.FrameWriter(os.path.join(args.out, "frames"))
        for v in range(n_views):
            seg = gsbp_amd.render_label_argmax(*scene.gauss, assoc.groups, k, scene.viewmats[v], scene.K, W, H, **raster_kw)
            writer.add(v, (shade[seg.long() + 1] * 255.0).to(torch.uint8))
        writer.close()
        wrote += f", frames/ for {n_views} views"
    print(f"wrote {args.out}: {wrote}; {assoc.n_groups} groups over {n_views} views, {report['grouped']} of {n} Gaussians grouped, "
          f"largest {sorted(report['group_sizes'], reverse=True)[:3]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
