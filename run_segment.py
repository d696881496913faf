#!/usr/bin/env python3
"""Command-line counterpart of the reference's segment.py / segment_compressed.py / click_and_segment.py: score a finished feature
field against prompt embeddings (and clicked pixels), write the 3-D mask, the per-view 2-D masks and the renders of the extracted
and the deleted scene, all on the HIP path (one pass over the field, P-channel renders, no [H, W, D] image).

    python run_segment.py --features F.pt --prompts P.pt --data-dir data/garden --checkpoint ckpt.pt --out seg/
    python run_segment.py --features F16.pt --prompts P.pt --encoder E.pt ...      # the compressed field: prompts @ encoder, renormalised
    python run_segment.py --features F.pt --prompts P.pt --click 3:410,222 --neg-click 3:90,40 ...
    python run_segment.py --synthetic C1 --out /tmp/seg                            # a seeded scene; its field is lifted first

--features: a .pt tensor [N, D], one row per Gaussian.  --prompts: a .pt dict {"prompts": [P, D], "n_pos": int}: embedding vectors
(no text encoder is part of this project), the first n_pos of them positive.  --click / --neg-click VIEW:X,Y (repeatable) add the
field rendered at that pixel of that view as one more positive / negative prompt.  Writes into --out: mask3d.pt (bool [N]),
mask2d/, extracted/ and deleted/ with one frame_0000.png ... per view when PIL imports, else frames.pt (uint8 [C, H, W, 3]) in each;
with --synthetic also features.pt and prompts.pt; with --export also extracted.pt and deleted.pt (gsplat checkpoint layout).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gsbp_amd import cli  # noqa: E402


def parse_click(text: str):
    try:
        view, xy = text.split(":")
        x, y = xy.split(",")
        return int(view), int(x), int(y)
    except ValueError:
        raise argparse.ArgumentTypeError(f"a click is VIEW:X,Y (three integers), got {text!r}")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default=None, help=".pt tensor [N, D]: the finished feature field")
    ap.add_argument("--prompts", default=None, help=".pt dict {'prompts': [P, D], 'n_pos': int}")
    ap.add_argument("--threshold", type=float, default=None, help="also require score[:, 0] > threshold (3-D mask)")
    ap.add_argument("--no-normalize", action="store_true", help="bare dot products instead of F.normalize(features) @ prompts.T")
    ap.add_argument("--click", type=parse_click, action="append", default=[], metavar="VIEW:X,Y", help="a positive click")
    ap.add_argument("--neg-click", type=parse_click, action="append", default=[], metavar="VIEW:X,Y", help="a negative click")
    ap.add_argument("--encoder", default=None, help=".pt tensor [D_in, D]: prompts @ encoder, renormalised (compressed field)")
    cli.add_scene_arguments(ap, max_views_help="render only the first views")
    ap.add_argument("--export", action="store_true", help="also write extracted.pt / deleted.pt")
    ap.add_argument("--out", default="./results/segment")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.synthetic and not (args.features and args.prompts):
        ap.error("give --features and --prompts (and the scene arguments), or --synthetic")
    import gsbp_amd
    from gsbp_amd import segment as seg, synthetic as syn
    cli.require_gpu("run_segment.py")
    dev = torch.device("cuda")
    os.makedirs(args.out, exist_ok=True)
    scene = cli.load_scene(args, dev)
    splats, gauss, K, W, H, cfg = scene.splats, scene.gauss, scene.K, scene.width, scene.height, scene.cfg
    sh_degree = None
    if args.synthetic:
        colors = torch.rand(cfg.n_gaussians, 3, generator=torch.Generator().manual_seed(syn.SH_SEED)).to(dev)
        if args.features:
            feats = torch.load(args.features, map_location=dev)
        else:
            feats = gsbp_amd.create_feature_field(*gauss, scene.viewmats, K, W, H,
                                                  lambda v: syn.make_feature_map(cfg, v, device=dev), cfg.feat_dim)
            torch.save(feats.cpu(), os.path.join(args.out, "features.pt"))
        if args.prompts:
            prompts, n_pos = seg.load_prompts(args.prompts)
        else:
            prompts, n_pos = syn.make_prompts(feats)
            seg.save_prompts(os.path.join(args.out, "prompts.pt"), prompts, n_pos)
    else:
        colors, sh_degree = torch.cat([splats["features_dc"], splats["features_rest"]], dim=1).float(), 3
        feats = torch.load(args.features, map_location=dev)
        prompts, n_pos = seg.load_prompts(args.prompts)
    n = splats["means"].shape[0]
    if feats.shape[0] != n:
        raise SystemExit(f"{feats.shape[0]} feature rows for {n} Gaussians (prune the scene as run_backproject.py did)")
    viewmats = scene.first_views(args.max_views).viewmats
    if args.encoder:
        prompts = seg.encode_prompts(prompts, torch.load(args.encoder, map_location="cpu"))
    raster_kw = dict(camera_model=args.camera_model, rasterize_mode=args.rasterize_mode)

    def activated(s):
        return s["means"].float(), s["rotation"].float(), torch.exp(s["scaling"]).float(), torch.sigmoid(s["opacity"]).float()

    pos, neg = list(prompts[:n_pos].to(dev)), list(prompts[n_pos:].to(dev))
    for clicks, side in ((args.click, pos), (args.neg_click, neg)):
        for view, x, y in clicks:
            if not 0 <= view < viewmats.shape[0]:
                raise SystemExit(f"click view {view} outside the {viewmats.shape[0]} views")
            vec, _, alpha = gsbp_amd.probe_pixels(*gauss, feats, viewmats[view], K, W, H, [[x, y]], **raster_kw)
            print(f"click view {view} ({x}, {y}): alpha {float(alpha[0]):.3f}")
            side.append(vec[0])
    prompts, n_pos = torch.stack(pos + neg), len(pos)

    normalize = not args.no_normalize
    mask3d = gsbp_amd.prompt_mask(feats, prompts, n_pos, threshold=args.threshold, normalize=normalize)
    torch.save(mask3d.cpu(), os.path.join(args.out, "mask3d.pt"))
    print(f"mask3d: {int(mask3d.sum())} of {n} Gaussians")
    extracted, deleted = gsbp_amd.apply_mask3d(splats, mask3d)
    if args.export:
        torch.save(seg.checkpoint_layout(extracted), os.path.join(args.out, "extracted.pt"))
        torch.save(seg.checkpoint_layout(deleted), os.path.join(args.out, "deleted.pt"))

    writers = {k: cli.FrameWriter(os.path.join(args.out, k)) for k in ("mask2d", "extracted", "deleted")}
    if n_pos < prompts.shape[0]:
        frames = gsbp_amd.render_prompt_mask(*gauss, feats, viewmats, K, W, H, prompts, n_pos, colors=colors, sh_degree=sh_degree,
                                             **raster_kw)
        for v, (mask2d, frame) in enumerate(frames):
            writers["mask2d"].add(v, frame)
    for name, part, keep in (("extracted", extracted, mask3d), ("deleted", deleted, ~mask3d)):
        if part["means"].shape[0] == 0:
            continue
        g, c = activated(part), colors[keep]
        for v in range(viewmats.shape[0]):
            rgb = gsbp_amd.rasterization(*g, c, viewmats[v:v + 1], K[None], W, H, sh_degree=sh_degree, want_meta=False,
                                         **raster_kw)[0][0]
            writers[name].add(v, (rgb * 255.0).clamp_(0.0, 255.0).to(torch.uint8))
    for w in writers.values():
        w.close()
    print(f"wrote {args.out}: mask3d.pt, mask2d/, extracted/, deleted/ for {viewmats.shape[0]} views")
    return 0


if __name__ == "__main__":
    sys.exit(main())
