#!/usr/bin/env python3
"""Polish a scene against its images on the HIP path: Adam on chosen parameters of a fixed set of Gaussians under the reference
trainer's loss, (1 - lambda) L1 + lambda (1 - SSIM) (gsbp_amd.polish_scene; the loss is the fused kernel pair of csrc/ssim.hip).

    python run_polish.py --data-dir data/garden --checkpoint ckpt.pt --images data/garden/images_4 --params opacities sh0 \\
        --steps 500 --out polished/
    python run_polish.py --synthetic T0 --steps 60 --out /tmp/polish    # a seeded scene against its own renders

--images DIR: per view the image <image name> itself (read with PIL when it imports), or <image name>.pt / .npy, [H, W, 3] in [0, 1]
(uint8 images are divided by 255); views without a file take no part.  --synthetic CFG: the targets are renders of the unperturbed
seeded scene, and the start is a seeded perturbation of the named parameters.
Writes into --out: polished.pt (the splat dict's tensors, pre-activation, under the reference's key names), history.json (the steps'
losses) and metrics.json ({"before", "after"}: per-view and mean PSNR / SSIM / L1 / MSE, gsbp_amd.score_image_views).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gsbp_amd import cli  # noqa: E402

PARAMS = ("means", "scales", "quats", "opacities", "sh0", "shN")
PERTURB_SEED = 4242
PERTURB = {"means": 0.002, "scales": 0.1, "quats": 0.05, "opacities": 0.5, "sh0": 0.3, "shN": 0.05}  # std of the synthetic start


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    cli.add_scene_arguments(ap, only=[o for o in cli.SCENE_OPTIONS if o != "max-views"])
    ap.add_argument("--images", default=None, metavar="DIR", help="the views' images (not with --synthetic)")
    ap.add_argument("--params", nargs="+", choices=PARAMS, default=["opacities", "sh0"])
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--ssim-lambda", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    # (default=SUPPRESS: an option that is not given leaves the parsed namespace as it was before the option existed)
    ap.add_argument("--sh-degree-interval", type=int, default=argparse.SUPPRESS, metavar="INTERVAL",
                    help="render step s at SH degree min(s // INTERVAL, the tables' degree), as the reference trainer does with "
                         "its interval of 1000 (default: off, every step at the full degree)")
    ap.add_argument("--adam", choices=("torch", "fused", "visible"), default=argparse.SUPPRESS,
                    help="the optimiser step: torch.optim.Adam (the default), the fused HIP kernel, or that kernel on the Gaussians "
                         "each step's view saw (the others keep their parameters and Adam moments)")
    ap.add_argument("--means-lr-final", type=float, default=argparse.SUPPRESS, metavar="FACTOR",
                    help="decay the means' learning rate exponentially to FACTOR of its start over the run, as the reference trainer "
                         "does with 0.01 (default: off)")
    ap.add_argument("--out", default="./results/polish")
    return ap


def load_image(directory: str, name: str, dev):
    """The view's image as float32 [H, W, 3] in [0, 1] on the device, or None when the directory has none."""
    for path in (os.path.join(directory, name + ".pt"), os.path.join(directory, name + ".npy"), os.path.join(directory, name)):
        if not os.path.isfile(path):
            continue
        if path.endswith(".pt"):
            t = torch.load(path)
        elif path.endswith(".npy"):
            import numpy as np
            t = torch.from_numpy(np.load(path))
        else:
            import numpy as np
            from PIL import Image
            t = torch.from_numpy(np.asarray(Image.open(path).convert("RGB")))
        t = t.to(dev)
        return (t.float() / 255.0 if t.dtype == torch.uint8 else t.float())[..., :3].contiguous()
    return None


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if bool(args.synthetic) == bool(args.images):
        ap.error("give exactly one of --images (with the scene arguments) and --synthetic")
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    import gsbp_amd
    from gsbp_amd import synthetic as syn
    from gsbp_amd.polish import PARAM_KEYS, render_splats
    cli.require_gpu("run_polish.py")
    dev = torch.device("cuda")
    os.makedirs(args.out, exist_ok=True)
    scene = cli.load_scene(args, dev)
    splats = {k: t for k, t in scene.splats.items() if torch.is_tensor(t) and t.dim() >= 1 and t.shape[0] == scene.gauss[0].shape[0]}
    viewmats, names, K, W, H = scene.viewmats, scene.names, scene.K, scene.width, scene.height
    kw = dict(camera_model=args.camera_model, rasterize_mode=args.rasterize_mode)
    if args.synthetic:
        n = splats["means"].shape[0]
        gen = torch.Generator().manual_seed(syn.SH_SEED)
        splats["features_dc"] = ((torch.rand(n, 1, 3, generator=gen) - 0.5) / 0.28209479177387814).to(dev)
        splats["features_rest"] = torch.zeros(n, 0, 3, device=dev)
        with torch.no_grad():
            images = [render_splats(splats, viewmats[v], K, W, H, **kw).clamp(0.0, 1.0) for v in range(viewmats.shape[0])]
        gen = torch.Generator().manual_seed(PERTURB_SEED)
        for name in args.params:
            key = PARAM_KEYS[name]
            splats[key] = splats[key] + PERTURB[name] * torch.randn(splats[key].shape, generator=gen).to(dev)

        def image_of(v):
            return images[v]
    else:
        have = [v for v, name in enumerate(names) if load_image(args.images, name, "cpu") is not None]
        if not have:
            raise SystemExit(f"no image of this scene's views in {args.images}")
        viewmats, names = viewmats[have], [names[v] for v in have]

        def image_of(v):
            return load_image(args.images, names[v], dev)

    before = gsbp_amd.score_image_views(splats, viewmats, K, W, H, image_of, **kw)
    polished, history = gsbp_amd.polish_scene(splats, viewmats, K, W, H, image_of, params=args.params, steps=args.steps,
                                              ssim_lambda=args.ssim_lambda, seed=args.seed,
                                              sh_degree_interval=getattr(args, "sh_degree_interval", None),
                                              **{k: getattr(args, k) for k in ("adam", "means_lr_final") if hasattr(args, k)}, **kw)
    after = gsbp_amd.score_image_views(polished, viewmats, K, W, H, image_of, **kw)
    torch.save({k: t.cpu() for k, t in polished.items()}, os.path.join(args.out, "polished.pt"))
    with open(os.path.join(args.out, "history.json"), "w") as f:
        json.dump(dict(params=list(args.params), steps=args.steps, ssim_lambda=args.ssim_lambda, seed=args.seed,
                       views=names, history=history), f, indent=1)
    with open(os.path.join(args.out, "metrics.json"), "w") as f:
        json.dump(dict(before=before, after=after), f, indent=1)
    print(f"loss {history[0]:.6e} -> {history[-1]:.6e} over {len(history)} steps; mean PSNR {before['mean']['psnr']:.3f} -> "
          f"{after['mean']['psnr']:.3f} dB, SSIM {before['mean']['ssim']:.4f} -> {after['mean']['ssim']:.4f}")
    print(f"wrote {args.out}: polished.pt, history.json, metrics.json")
    return 0


if __name__ == "__main__":
    sys.exit(main())
