#!/usr/bin/env python3
"""Command-line counterpart of the reference's visualize_pca.py: fit a 3-component PCA on a finished feature field, colour the
Gaussians by it and render the frames, all on the HIP path (no host copy of the field, no sklearn, no [H, W, D] render).

    python run_pca.py --features results/garden/features_lseg.pt --data-dir data/garden --checkpoint ckpt.pt --out pca/
    python run_pca.py --features F.pt --mode renderings --out pca/          # "PCA on renderings" (scale 1.0)
    python run_pca.py --synthetic C1 --out /tmp/pca                         # a seeded scene; its field is lifted first

--features: a .pt tensor [N, D] (what run_backproject.py writes), one row per Gaussian of the scene.  Writes into --out:
pca_basis.pt (PCABasis.state_dict()), pca_colors.pt ({'colors': [N, 3], 'lo', 'hi'}), with --synthetic also features.pt, and one
frame per view: frame_0000.png ... (R, G, B = components 1, 2, 3) when PIL imports, else frames.pt (uint8 [C, H, W, 3]).
--mode gaussians renders the colours with scales x --scale (default 0.2, as the reference); --mode renderings the PCA of the
rendered features (default scale 1.0).
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
    cli.add_scene_arguments(ap, only=("data-dir", "checkpoint", "format", "data-factor", "synthetic"))
    ap.add_argument("--mode", choices=["gaussians", "renderings"], default="gaussians")
    ap.add_argument("--scale", type=float, default=None, help="factor on the Gaussians' scales (default 0.2 / 1.0 by --mode)")
    cli.add_scene_arguments(ap, only=("camera-model", "rasterize-mode", "max-views"), max_views_help="render only the first views")
    ap.add_argument("--out", default="./results/pca")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.synthetic and not args.features:
        ap.error("give --features (and the scene arguments), or --synthetic")
    import gsbp_amd
    from gsbp_amd import synthetic as syn
    cli.require_gpu("run_pca.py")
    dev = torch.device("cuda")
    os.makedirs(args.out, exist_ok=True)
    scene = cli.load_scene(args, dev, activate_on_host=True)
    (means, quats, scales, opac), K, viewmats, W, H, cfg = scene.gauss, scene.K, scene.viewmats, scene.width, scene.height, scene.cfg
    if args.features:
        feats = torch.load(args.features, map_location=dev)
    else:
        feats = gsbp_amd.create_feature_field(means, quats, scales, opac, viewmats, K, W, H,
                                              lambda v: syn.make_feature_map(cfg, v, device=dev), cfg.feat_dim)
        torch.save(feats.cpu(), os.path.join(args.out, "features.pt"))
    if feats.shape[0] != means.shape[0]:
        raise SystemExit(f"{feats.shape[0]} feature rows for {means.shape[0]} Gaussians (prune the scene as run_backproject.py did)")
    viewmats = scene.first_views(args.max_views).viewmats

    basis = gsbp_amd.fit_pca(feats, 3)
    colors, lo, hi = gsbp_amd.pca_colors(feats, basis)
    torch.save(basis.state_dict(), os.path.join(args.out, "pca_basis.pt"))
    torch.save({"colors": colors.cpu(), "lo": float(lo), "hi": float(hi)}, os.path.join(args.out, "pca_colors.pt"))
    print("explained variance ratio:", [round(float(r), 4) for r in basis.explained_variance_ratio])

    scale = args.scale if args.scale is not None else (0.2 if args.mode == "gaussians" else 1.0)
    frames = gsbp_amd.render_pca(means, quats, scales, opac, feats, viewmats, K, W, H, mode=args.mode, basis=basis, scale=scale,
                                 camera_model=args.camera_model, rasterize_mode=args.rasterize_mode)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    kept = []
    for v, frame in enumerate(frames):
        if Image is not None:
            Image.fromarray(frame.cpu().numpy(), "RGB").save(os.path.join(args.out, f"frame_{v:04d}.png"))
        else:
            kept.append(frame.cpu())
    if Image is None:
        torch.save(torch.stack(kept), os.path.join(args.out, "frames.pt"))
    print(f"wrote {args.out}: pca_basis.pt, pca_colors.pt, {viewmats.shape[0]} {args.mode} frames "
          f"({'png' if Image is not None else 'frames.pt'})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
