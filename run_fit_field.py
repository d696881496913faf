#!/usr/bin/env python3
"""Fit a latent feature field and its decoder to 2-D feature maps on frozen Gaussians, on the HIP path (the reference's
Feature-3DGS baseline, f3dgs/simple_trainer_feature_3dgs.py, with the scene fixed): per step one view is rendered, decoded,
compared and differentiated without any [H, W, D] image (gwbp_decode_loss), and Adam updates the latents and the decoder.

    python run_fit_field.py --maps maps/ --data-dir data/scene --checkpoint ckpt.pt --steps 3000 --out fit/
    python run_fit_field.py --synthetic C1 --steps 200 --score --out /tmp/fit   # a seeded scene and its seeded maps

--maps DIR: per view <image name>.pt, the [H, W, D] map (float32, float16 or bfloat16, read as stored); views without a file take
no part.  --pixel-weights DIR: per view <image name>.pt, an [H, W] weight map (as run_backproject.py --pixel-weights reads them).
Writes into --out: decoded_field.pt ({"features": [N, d], "conv": [d, D]}: the keys of a Feature-3DGS checkpoint) and history.json
(the steps' losses).  --score also writes fidelity.json: the field_fidelity summary of the decoded field beside that of the field
create_feature_field lifts from the same maps, so that the two methods can be read side by side.
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
    ap.add_argument("--maps", default=None, help="directory of <image name>.pt feature maps [H, W, D]")
    cli.add_scene_arguments(ap, only=("synthetic",))
    ap.add_argument("--pixel-weights", default=None, metavar="DIR", help="directory of <image name>.pt weight maps [H, W]")
    ap.add_argument("--latent-dim", type=int, default=128, help="channels of the latent table: a multiple of 16 in [16, 128]")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--loss", choices=["l1", "l2"], default="l1")
    ap.add_argument("--lr", type=float, default=2.5e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--score", action="store_true", help="also score the decoded and the lifted field against the maps")
    cli.add_scene_arguments(ap, only=("data-dir", "checkpoint", "format", "data-factor"))
    ap.add_argument("--out", default="./results/fit_field")
    return ap


def _summary(rep):
    return dict(overall={k: None if math.isnan(x) else x for k, x in rep["overall"].items()}, views_scored=rep["views_scored"])


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if bool(args.synthetic) == bool(args.maps):
        ap.error("give exactly one of --maps (with the scene arguments) and --synthetic")
    import gsbp_amd
    from gsbp_amd import synthetic as syn
    cli.require_gpu("run_fit_field.py")
    dev = torch.device("cuda")
    os.makedirs(args.out, exist_ok=True)
    if args.synthetic and syn.CONFIGS[args.synthetic].lowres:
        raise SystemExit(f"{args.synthetic} has low-resolution maps: the fit takes full-resolution [H, W, D] maps")
    scene = cli.load_scene(args, dev, activate_on_host=True)
    gauss, K, viewmats, W, H, names, cfg = scene.gauss, scene.K, scene.viewmats, scene.width, scene.height, scene.names, scene.cfg
    if args.synthetic:
        dim = cfg.feat_dim
        maps = [syn.make_feature_map(cfg, v, device=dev) for v in range(viewmats.shape[0])]

        def map_of(v):
            return maps[v]
    else:
        have = [v for v, name in enumerate(names) if os.path.exists(os.path.join(args.maps, name + ".pt"))]
        if not have:
            raise SystemExit(f"no <image name>.pt map of this scene in {args.maps}")
        viewmats, names = viewmats[have], [names[v] for v in have]

        def map_of(v):
            return torch.load(os.path.join(args.maps, names[v] + ".pt")).to(dev)
        dim = int(map_of(0).shape[2])

    weight_of = None
    if args.pixel_weights:
        def weight_of(v):
            path = os.path.join(args.pixel_weights, names[v] + ".pt")
            return torch.load(path).to(dev) if os.path.exists(path) else None

    latents, decoder, history = gsbp_amd.fit_decoded_field(*gauss, viewmats, K, W, H, map_of, dim, latent_dim=args.latent_dim,
                                                           steps=args.steps, lr=args.lr, loss=args.loss, pixel_weight_fn=weight_of,
                                                           seed=args.seed)
    torch.save({"features": latents.cpu(), "conv": decoder.cpu()}, os.path.join(args.out, "decoded_field.pt"))
    with open(os.path.join(args.out, "history.json"), "w") as f:
        json.dump(dict(loss=args.loss, lr=args.lr, latent_dim=args.latent_dim, D=dim, steps=args.steps, seed=args.seed,
                       views=names, history=history), f, indent=1)
    if history:
        print(f"{args.loss} loss {history[0]:.6e} -> {history[-1]:.6e} over {len(history)} steps")
    if args.score:
        fields = dict(decoded=gsbp_amd.decode_field(latents, decoder),
                      lifted=gsbp_amd.create_feature_field(*gauss, viewmats, K, W, H, map_of, dim))
        rep = {k: _summary(gsbp_amd.field_fidelity(gsbp_amd.score_field_views(*gauss, f, viewmats, K, W, H, map_of)))
               for k, f in fields.items()}
        with open(os.path.join(args.out, "fidelity.json"), "w") as f:
            json.dump(rep, f, indent=1)
        for k, r in rep.items():
            print(f"{k:8s} " + "  ".join(f"{m} {x:.4e}" if x is not None else f"{m} nan" for m, x in r["overall"].items()))
    print(f"wrote {args.out}: decoded_field.pt, history.json" + (", fidelity.json" if args.score else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
