#!/usr/bin/env python3
"""Score a finished feature field against the 2-D maps it was lifted from, on the HIP path: the field is rendered and compared with
each view's map inside one kernel (gwbp_field_compare), so no [H, W, D] image is made.

    python run_fidelity.py --features features.pt --maps maps/ --data-dir data/scene --checkpoint ckpt.pt --out fidelity/
    python run_fidelity.py --features features.pt --maps tokens/ --upsample nearest --weights-out weights/ --cosine-min 0.5 ...
    python run_fidelity.py --synthetic C1 --out /tmp/fidelity          # a seeded scene, its seeded maps and the field lifted from them

--features: a .pt float tensor [N, D], one row per Gaussian of the scene (a field of run_backproject.py --no-prune).  --maps DIR:
per view <image name>.pt, the [H, W, D] map the field was built from (float32, float16 or bfloat16, read as stored); a view without
a file is skipped.  --upsample nearest: the maps are the network's low-resolution [h, w, D] maps, read through nearest upsampling
and never expanded (bilinear maps: store the upsampled map).  Writes into --out: table.pt (float64 [V, 8] per view: sum cosine, sum
l1, sum l2, sum mm, n_valid, n_bad, n_pixels, D) and fidelity.json (mean cosine, mean absolute error, MSE and relative error, per
view and overall).  --weights-out DIR with --cosine-min T (or --quantile Q): one bool [H, W] weight map <image name>.pt per scored
view, True where the field agrees with the view's map -- the directory run_backproject.py --pixel-weights reads for a second,
robust lift.
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


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default=None, help=".pt float tensor [N, D]: the finished field")
    ap.add_argument("--maps", default=None, help="directory of <image name>.pt feature maps [H, W, D] ([h, w, D] with --upsample)")
    ap.add_argument("--upsample", choices=["nearest"], default=None, help="the maps are low-resolution, nearest-upsampled")
    ap.add_argument("--weights-out", default=None, metavar="DIR", help="write one agreement weight map per view here")
    ap.add_argument("--cosine-min", type=float, default=None, help="weight 1 where the per-pixel cosine is at least this")
    ap.add_argument("--quantile", type=float, default=None, help="weight 0 for this share of each view's lowest cosines")
    cli.add_scene_arguments(ap)
    ap.add_argument("--out", default="./results/fidelity")
    return ap


def _json_number(x: float):
    return None if math.isnan(x) else x


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.synthetic and not (args.features and args.maps):
        ap.error("give --features and --maps (and the scene arguments), or --synthetic")
    if args.weights_out and (args.cosine_min is None) == (args.quantile is None):
        ap.error("--weights-out needs exactly one of --cosine-min and --quantile")
    import gsbp_amd
    from gsbp_amd import synthetic as syn
    cli.require_gpu("run_fidelity.py")
    dev = torch.device("cuda")
    os.makedirs(args.out, exist_ok=True)
    raster_kw = dict(camera_model=args.camera_model, rasterize_mode=args.rasterize_mode)
    scene = cli.load_scene(args, dev, activate_on_host=True)
    gauss, K, viewmats, W, H, names, cfg = scene.gauss, scene.K, scene.viewmats, scene.width, scene.height, scene.names, scene.cfg
    if args.synthetic:
        upsample = cfg.upsample if cfg.lowres else None
        if upsample == "bilinear":
            raise SystemExit(f"{args.synthetic} has bilinear low-resolution maps: the comparison takes the upsampled map")

        def map_of(v):
            return syn.make_feature_map(cfg, v, device=dev)
        if args.features:
            features = torch.load(args.features, map_location="cpu")
        else:
            features = gsbp_amd.create_feature_field(*gauss, viewmats, K, W, H, map_of, cfg.feat_dim, reduction=cfg.reduction,
                                                     upsample=upsample, **raster_kw)
    else:
        features = torch.load(args.features, map_location="cpu")
        upsample = args.upsample

        def map_of(v):
            path = os.path.join(args.maps, names[v] + ".pt")
            return torch.load(path).to(dev) if os.path.exists(path) else None
    features = torch.as_tensor(features).to(dev)
    n = gauss[0].shape[0]
    if features.dim() != 2 or features.shape[0] != n:
        raise SystemExit(f"the field has shape {tuple(features.shape)}, the scene {n} Gaussians (a field built on the pruned scene "
                         "does not fit the checkpoint: build it with run_backproject.py --no-prune)")
    scene = scene.first_views(args.max_views)
    viewmats, names = scene.viewmats, scene.names

    table = gsbp_amd.score_field_views(*gauss, features, viewmats, K, W, H, map_of, upsample=upsample, **raster_kw)
    torch.save(table.cpu(), os.path.join(args.out, "table.pt"))
    rep = gsbp_amd.field_fidelity(table)
    with open(os.path.join(args.out, "fidelity.json"), "w") as f:
        json.dump(dict(overall={k: _json_number(x) for k, x in rep["overall"].items()},
                       per_view={k: [_json_number(x) for x in t.tolist()] for k, t in rep["per_view"].items()},
                       n_valid=rep["n_valid"].tolist(), n_bad=rep["n_bad"].tolist(), views=names,
                       views_scored=rep["views_scored"], D=int(features.shape[1]), width=W, height=H), f, indent=1)
    o = rep["overall"]
    print(f"mean cosine {o['cosine']:.4f}  MAE {o['mae']:.3e}  MSE {o['mse']:.3e}  relative error {o['relative']:.4f}  "
          f"({rep['views_scored']} of {len(names)} views scored)")

    if args.weights_out:
        os.makedirs(args.weights_out, exist_ok=True)
        kept = total = 0
        for v in range(viewmats.shape[0]):
            fmap = map_of(v)
            if fmap is None:
                continue
            planes = gsbp_amd.render_field_agreement(*gauss, features, fmap, viewmats[v], K, W, H, upsample=upsample, **raster_kw)
            w = gsbp_amd.agreement_weights(planes, cosine_min=args.cosine_min, quantile=args.quantile)
            torch.save(w.cpu(), os.path.join(args.weights_out, names[v] + ".pt"))
            kept, total = kept + int(w.sum()), total + w.numel()
        print(f"wrote {args.weights_out}: weight maps with {kept} of {total} pixels kept")
    print(f"wrote {args.out}: table.pt, fidelity.json for {viewmats.shape[0]} views")
    return 0


if __name__ == "__main__":
    sys.exit(main())
