#!/usr/bin/env python3
"""Train a scene against its images on the HIP path with densification: Adam under the reference trainer's loss while the set of
Gaussians grows and shrinks by gsplat's default rule (gsbp_amd.train_scene; the rounds are the kernels of csrc/densify.hip), or,
with --strategy mcmc, by its MCMCStrategy: dead Gaussians relocated onto alive ones, growth by 5 % a round up to --cap-max, noise on
the means every step (csrc/mcmc.hip), and the reference's opacity and scale regularisers.

    python run_train.py --colmap data/garden/sparse/0 --images data/garden/images_4 --data-factor 4 --steps 7000 --out trained/
    python run_train.py --synthetic T0 --steps 60 --refine-start 10 --refine-every 10 --out /tmp/train
    python run_train.py --synthetic T0 --steps 60 --strategy mcmc --cap-max 300 --refine-start 10 --refine-every 10 --out /tmp/train
    python run_train.py --synthetic T0 --steps 60 --feature-dim 32 --latent-dim 16 --out /tmp/train
    python run_train.py --synthetic T0 --steps 60 --pose-opt --pose-opt-lr 2e-3 --pose-noise 0.02 --out /tmp/train

--colmap DIR: cameras.bin, images.bin and points3D.bin of a COLMAP sparse model; the start is its point cloud (gsbp_amd.
init_splats_from_points).  --images DIR: per view the image <image name> itself (read with PIL when it imports), or <image name>.pt /
.npy, [H, W, 3] in [0, 1] (uint8 images are divided by 255); views without a file take no part.  --synthetic CFG: the targets are
renders of the seeded scene with seeded colours, and the start is every --start-stride'th Gaussian of it.
Writes into --out: trained.pt (the splat dict's tensors, pre-activation, under the reference's key names), history.json (the steps'
losses and sizes, the rounds' counts, the resets) and metrics.json ({"before", "after"}: per-view and mean PSNR / SSIM / L1 / MSE,
gsbp_amd.score_image_views).
--feature-dim D adds the reference trainer's feature term (gsbp_amd.train_scene(feature_fn=...)): a second render per step, of a
[N, --latent-dim] latent table that a [--latent-dim, D] decoder turns into the view's feature map, under --feature-weight x L1.  With
--synthetic the maps are a hidden seeded latent field and decoder rendered on the true scene; with --colmap they are --feature-maps
DIR/<image stem>.npy or .pt, [h, w, D], upsampled bilinearly to the view when smaller (as the reference upsamples its network's
output); views without a map take no part.  Then --out also holds features.pt (the latents, and the decoder under "decoder"), and
history.json the steps' feature losses.
--depth-loss adds the reference trainer's depth term (gsbp_amd.train_scene(depth_fn=...)): --depth-lambda x scene scale x the mean
|1 / depth - 1 / true depth| of the render's expected depth sampled at the view's points.  With --colmap the points are the view's
triangulated COLMAP points (gsbp_amd.scene_io.view_depth_points); with --synthetic 256 seeded positions per view with the true scene's
depth there.  history.json then holds the steps' depth losses under "depth_loss".
--pose-opt trains a correction per view with the Gaussians (gsbp_amd.train_scene(pose_opt=True): the reference trainer's pose_opt, for
captures whose COLMAP poses are slightly off) at --pose-opt-lr (decayed to a hundredth over the run) with --pose-opt-reg weight decay;
--pose-noise STD perturbs every view once, seeded, before anything else (the reference's pose_noise: a test of the former, and it may
stand alone).  Then --out also holds poses.pt (pose_adjust [V, 9] under --pose-opt, viewmats [V, 4, 4]: the views as they ended, and
the views' names), metrics.json's "after" is scored with those view matrices, and history.json holds the option values and, under
--pose-noise, pose_err: per step the mean absolute difference between the true and the used camera-to-world matrices.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gsbp_amd import cli  # noqa: E402
from run_polish import load_image  # noqa: E402

PARAMS = ("means", "scales", "quats", "opacities", "sh0", "shN")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--colmap", default=None, metavar="DIR", help="a COLMAP sparse model: cameras.bin, images.bin, points3D.bin")
    ap.add_argument("--images", default=None, metavar="DIR", help="the views' images (with --colmap)")
    ap.add_argument("--data-factor", type=int, default=1, help="the images are this many times smaller than the model's cameras")
    cli.add_scene_arguments(ap, only=["synthetic", "camera-model", "rasterize-mode"])
    ap.add_argument("--start-stride", type=int, default=2, help="--synthetic: start from every n-th Gaussian of the scene")
    ap.add_argument("--params", nargs="+", choices=PARAMS, default=list(PARAMS))
    ap.add_argument("--steps", type=int, default=7000)
    ap.add_argument("--sh-degree", type=int, default=3, help="--colmap: the SH degree of the start")
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
    ap.add_argument("--depth-loss", action="store_true", default=argparse.SUPPRESS,
                    help="add the reference trainer's depth term: the render's expected depth against the view's triangulated COLMAP "
                         "points (--colmap), or against 256 seeded samples of the true scene's depth per view (--synthetic)")
    ap.add_argument("--depth-lambda", type=float, default=argparse.SUPPRESS, help="weight of the depth term (default 0.01)")
    ap.add_argument("--depth-kind", choices=("disparity", "depth"), default=argparse.SUPPRESS,
                    help="what a depth MAP is compared in (train_scene(depth_kind=...)).  Both sources this script has hand over POINTS, "
                         "which are always compared in disparity: the switch is passed on and changes nothing until a map source exists")
    ap.add_argument("--pose-opt", action="store_true", default=argparse.SUPPRESS,
                    help="train a pose correction per view with the Gaussians, as the reference trainer's pose_opt does")
    ap.add_argument("--pose-opt-lr", type=float, default=argparse.SUPPRESS, help="its learning rate (default 1e-5)")
    ap.add_argument("--pose-opt-reg", type=float, default=argparse.SUPPRESS, help="its weight decay (default 1e-6)")
    ap.add_argument("--pose-noise", type=float, default=argparse.SUPPRESS, metavar="STD",
                    help="perturb every view once by a seeded pose error of this standard deviation (default 0: off)")
    ap.add_argument("--feature-dim", type=int, default=argparse.SUPPRESS, metavar="D",
                    help="train a latent feature field beside the colours against feature maps of D channels")
    ap.add_argument("--latent-dim", type=int, default=argparse.SUPPRESS, help="channels of the latent table (default 128)")
    ap.add_argument("--feature-weight", type=float, default=argparse.SUPPRESS, help="weight of the feature term (default 1)")
    ap.add_argument("--feature-maps", default=argparse.SUPPRESS, metavar="DIR", help="--colmap: <image stem>.npy / .pt per view")
    # the schedule (gsbp_amd.DensifyConfig; gsplat's defaults)
    ap.add_argument("--prune-opa", type=float, default=0.005)
    ap.add_argument("--grow-grad2d", type=float, default=2e-4)
    ap.add_argument("--grow-scale3d", type=float, default=0.01)
    ap.add_argument("--prune-scale3d", type=float, default=0.1)
    ap.add_argument("--refine-start", type=int, default=500)
    ap.add_argument("--refine-stop", type=int, default=15000, help="--strategy mcmc: 25000 unless the option is given")
    ap.add_argument("--refine-every", type=int, default=100)
    ap.add_argument("--reset-every", type=int, default=3000)
    ap.add_argument("--pause-refine-after-reset", type=int, default=0)
    ap.add_argument("--scene-scale", type=float, default=None,
                    help="default: 1.1 x the largest distance of a camera from the cameras' centre (--colmap), 1 (--synthetic)")
    ap.add_argument("--max-gaussians", type=int, default=None)
    # --strategy mcmc (gsbp_amd.MCMCConfig; gsplat's defaults).  It shares --refine-start and --refine-every; its --refine-stop
    # defaults to 25000
    ap.add_argument("--strategy", choices=("default", "mcmc"), default="default")
    ap.add_argument("--cap-max", type=int, default=1_000_000)
    ap.add_argument("--noise-lr", type=float, default=5e5)
    ap.add_argument("--min-opacity", type=float, default=0.005)
    ap.add_argument("--opacity-reg", type=float, default=None, help="default: 0 (--strategy default), 0.01 (--strategy mcmc)")
    ap.add_argument("--scale-reg", type=float, default=None, help="default: 0 (--strategy default), 0.01 (--strategy mcmc)")
    ap.add_argument("--out", default="./results/train")
    return ap


FEATURE_SEED = 1234  # --synthetic: the hidden latent field and decoder of the feature maps
DEPTH_SEED, DEPTH_POINTS = 4321, 256  # --synthetic --depth-loss: the seeded positions per view


def synthetic_depth_points(full, viewmats, K, W, H, dev, **kw):
    """--synthetic --depth-loss: per view, DEPTH_POINTS seeded uniform positions with the depths the TARGET scene's expected-depth
    render has there under the depth loss's own bilinear rule; positions whose sample is 0 (nothing rendered there) are dropped."""
    import gsbp_amd
    from gsbp_amd.polish import render_splats
    gen = torch.Generator().manual_seed(DEPTH_SEED)
    out = []
    for v in range(viewmats.shape[0]):
        xy = (torch.rand(DEPTH_POINTS, 2, generator=gen) * torch.tensor([W - 1.0, H - 1.0])).to(dev)
        with torch.no_grad():
            render, alpha = render_splats(full, viewmats[v], K, W, H, render_mode="RGB+D", return_alpha=True, **kw)
            d = gsbp_amd.sample_expected_depth(render, alpha, xy)
        keep = d > 0
        out.append((xy[keep].contiguous(), d[keep].contiguous()))
    return out


def feature_map_path(directory: str, name: str):
    """The file of the view's feature map, <image stem>.pt or .npy, or None when the directory has neither."""
    stem = os.path.splitext(name)[0]
    for path in (os.path.join(directory, stem + ".pt"), os.path.join(directory, stem + ".npy")):
        if os.path.isfile(path):
            return path
    return None


def load_feature_map(directory: str, name: str, dev, width: int, height: int, dim: int):
    """The view's feature map as float32 [H, W, dim] on the device, or None when the directory has none.  A map of another size is
    resampled to the view on the device with F.interpolate(mode="bilinear"), as the reference resamples its feature network's output."""
    path = feature_map_path(directory, name)
    if path is None:
        return None
    if path.endswith(".pt"):
        t = torch.load(path)
    else:
        import numpy as np
        t = torch.from_numpy(np.load(path))
    t = t.to(dev).float()
    if t.dim() != 3 or t.shape[2] != dim:
        raise SystemExit(f"{path}: expected [h, w, {dim}], got {tuple(t.shape)}")
    if tuple(t.shape[:2]) != (height, width):
        t = torch.nn.functional.interpolate(t.permute(2, 0, 1)[None], (height, width), mode="bilinear")[0].permute(1, 2, 0)
    return t.contiguous()


def camera_extent(viewmats: torch.Tensor) -> float:
    """The largest distance of a camera centre from the centres' mean (what gsplat's trainer multiplies by 1.1 for its scene scale)."""
    vm = viewmats.detach().double().cpu()
    centres = -(vm[:, :3, :3].transpose(1, 2) @ vm[:, :3, 3:]).squeeze(-1)
    return float((centres - centres.mean(dim=0)).norm(dim=1).max())


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    stop_given = any(a.split("=")[0] == "--refine-stop" for a in (sys.argv[1:] if argv is None else argv))
    if bool(args.synthetic) == bool(args.colmap):
        ap.error("give exactly one of --colmap (with --images) and --synthetic")
    if args.colmap and not args.images:
        ap.error("--colmap needs --images")
    if args.steps < 1 or args.start_stride < 1:
        ap.error("--steps and --start-stride must be at least 1")
    feature_dim = getattr(args, "feature_dim", None)
    latent_dim = getattr(args, "latent_dim", 128)
    if feature_dim is None and any(hasattr(args, k) for k in ("latent_dim", "feature_weight", "feature_maps")):
        ap.error("--latent-dim, --feature-weight and --feature-maps need --feature-dim")
    depth_loss = getattr(args, "depth_loss", False)
    if not depth_loss and any(hasattr(args, k) for k in ("depth_lambda", "depth_kind")):
        ap.error("--depth-lambda and --depth-kind need --depth-loss")
    pose_kw = {k: getattr(args, k) for k in ("pose_opt", "pose_opt_lr", "pose_opt_reg", "pose_noise") if hasattr(args, k)}
    if "pose_opt" not in pose_kw and any(k in pose_kw for k in ("pose_opt_lr", "pose_opt_reg")):
        ap.error("--pose-opt-lr and --pose-opt-reg need --pose-opt")
    if feature_dim is not None and bool(args.colmap) != hasattr(args, "feature_maps"):
        ap.error("--feature-dim takes its maps from --feature-maps with --colmap, and renders them itself with --synthetic")
    import gsbp_amd
    from gsbp_amd import scene_io, synthetic as syn
    from gsbp_amd.polish import render_splats
    cli.require_gpu("run_train.py")
    dev = torch.device("cuda")
    os.makedirs(args.out, exist_ok=True)
    kw = dict(camera_model=args.camera_model, rasterize_mode=args.rasterize_mode)
    if args.synthetic:
        cfg = syn.CONFIGS[args.synthetic]
        full = {k: t.to(dev) for k, t in syn.make_scene(cfg).items()}
        n = full["means"].shape[0]
        gen = torch.Generator().manual_seed(syn.SH_SEED)
        full["features_dc"] = ((torch.rand(n, 1, 3, generator=gen) - 0.5) / 0.28209479177387814).to(dev)
        full["features_rest"] = torch.zeros(n, 0, 3, device=dev)
        K, viewmats, W, H = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg).to(dev), cfg.width, cfg.height
        names = [f"view_{v:04d}" for v in range(viewmats.shape[0])]
        with torch.no_grad():
            images = [render_splats(full, viewmats[v], K, W, H, **kw).clamp(0.0, 1.0) for v in range(viewmats.shape[0])]
        feature_maps = None
        if feature_dim is not None:  # a hidden latent field and decoder, rendered on the true scene
            gen = torch.Generator().manual_seed(FEATURE_SEED)
            true_latents = torch.rand(n, latent_dim, generator=gen).to(dev)
            true_decoder = (torch.rand(latent_dim, feature_dim, generator=gen) / latent_dim).to(dev)
            geometry = (full["means"], full["rotation"], torch.exp(full["scaling"]), torch.sigmoid(full["opacity"]))
            with torch.no_grad():
                feature_maps = [gsbp_amd.render_latents(*geometry, true_latents, viewmats[v], K, W, H, **kw)[0] @ true_decoder
                                for v in range(viewmats.shape[0])]
        depth_points = synthetic_depth_points(full, viewmats, K, W, H, dev, **kw) if depth_loss else None
        splats = {k: t[::args.start_stride].contiguous() for k, t in full.items()}
        scene_scale = 1.0 if args.scene_scale is None else args.scene_scale

        def image_of(v):
            return images[v]
    else:
        proj = scene_io.read_colmap_model(args.colmap)
        if proj.points3D is None or len(proj.points3D) == 0:
            raise SystemExit(f"{args.colmap} has no points3D.bin: there is nothing to start from")
        K = scene_io.camera_matrix(next(iter(proj.cameras.values())), args.data_factor).float().to(dev)
        W, H = int(K[0, 2] * 2), int(K[1, 2] * 2)
        viewmats = scene_io.sorted_viewmats(proj).to(dev)
        names = sorted(im.name for im in proj.images.values())
        have = [v for v, name in enumerate(names) if load_image(args.images, name, "cpu") is not None]
        if not have:
            raise SystemExit(f"no image of this model's views in {args.images}")
        feature_maps = None
        if feature_dim is not None:
            have = [v for v in have if feature_map_path(args.feature_maps, names[v]) is not None]
            if not have:
                raise SystemExit(f"no feature map of this model's views in {args.feature_maps}")
        viewmats, names = viewmats[have], [names[v] for v in have]
        depth_points = None
        if depth_loss:  # the views' triangulated points, as the reference's loader hands them to its trainer
            by_name = {im.name: im for im in proj.images.values()}
            depth_points = [tuple(t.to(dev) for t in scene_io.view_depth_points(proj, by_name[name], K, W, H)) for name in names]
        splats = gsbp_amd.init_splats_from_points(torch.from_numpy(proj.points3D).float().to(dev),
                                                  torch.from_numpy(proj.point3D_colors).to(dev), sh_degree=args.sh_degree)
        scene_scale = 1.1 * camera_extent(viewmats) if args.scene_scale is None else args.scene_scale

        def image_of(v):
            return load_image(args.images, names[v], dev)

    mcmc = args.strategy == "mcmc"
    reg = dict(opacity_reg=(0.01 if mcmc else 0.0) if args.opacity_reg is None else args.opacity_reg,
               scale_reg=(0.01 if mcmc else 0.0) if args.scale_reg is None else args.scale_reg)
    if mcmc:
        cfg = gsbp_amd.MCMCConfig(cap_max=args.cap_max, noise_lr=args.noise_lr, refine_start_iter=args.refine_start,
                                  refine_stop_iter=args.refine_stop if stop_given else 25000,
                                  refine_every=args.refine_every, min_opacity=args.min_opacity)
    else:
        cfg = gsbp_amd.DensifyConfig(prune_opa=args.prune_opa, grow_grad2d=args.grow_grad2d, grow_scale3d=args.grow_scale3d,
                                     prune_scale3d=args.prune_scale3d, refine_start_iter=args.refine_start,
                                     refine_stop_iter=args.refine_stop,
                                     refine_every=args.refine_every, reset_every=args.reset_every,
                                     pause_refine_after_reset=args.pause_refine_after_reset, scene_scale=scene_scale,
                                     max_gaussians=args.max_gaussians)
    feature_kw = {}
    if feature_dim is not None:
        loaded = {}  # --colmap: a view's map is read and resampled once, at the first step that takes the view, and kept

        def feature_of(v):
            if feature_maps is not None:
                return feature_maps[v]
            if v not in loaded:
                loaded[v] = load_feature_map(args.feature_maps, names[v], dev, W, H, feature_dim)
            return loaded[v]
        feature_kw = dict(feature_fn=feature_of, feature_dim=feature_dim, latent_dim=latent_dim,
                          feature_weight=getattr(args, "feature_weight", 1.0))
    depth_kw = {}
    if depth_loss:  # (depth_scale: the reference multiplies its depth term by the scene's scale)
        depth_kw = dict(depth_fn=lambda v: depth_points[v], depth_scale=scene_scale,
                        **{k: getattr(args, k) for k in ("depth_lambda", "depth_kind") if hasattr(args, k)})
    before = gsbp_amd.score_image_views(splats, viewmats, K, W, H, image_of, **kw)
    n_start = splats["means"].shape[0]
    trained, history = gsbp_amd.train_scene(splats, viewmats, K, W, H, image_of, args.steps, strategy=cfg, params=args.params,
                                            ssim_lambda=args.ssim_lambda, seed=args.seed,
                                            sh_degree_interval=getattr(args, "sh_degree_interval", None), **reg, **feature_kw,
                                            **{k: getattr(args, k) for k in ("adam", "means_lr_final") if hasattr(args, k)}, **depth_kw,
                                            **pose_kw, **kw)
    after = gsbp_amd.score_image_views(trained, history.get("viewmats", viewmats), K, W, H, image_of, **kw)
    torch.save({k: t.cpu() for k, t in trained.items() if torch.is_tensor(t)}, os.path.join(args.out, "trained.pt"))
    extra = {}
    if feature_dim is not None:
        torch.save(dict(features=trained["features"].cpu(), decoder=history["decoder"].cpu()), os.path.join(args.out, "features.pt"))
        extra = dict(feature_loss=history["feature_loss"], feature_dim=feature_dim, latent_dim=latent_dim,
                     feature_weight=feature_kw["feature_weight"])
    if pose_kw:
        torch.save(dict(viewmats=history["viewmats"].cpu(), views=names,
                        **({"pose_adjust": history["pose_adjust"].cpu()} if "pose_adjust" in history else {})),
                   os.path.join(args.out, "poses.pt"))
        extra.update(pose_kw, **({"pose_err": history["pose_err"]} if "pose_err" in history else {}))
    with open(os.path.join(args.out, "history.json"), "w") as f:
        json.dump(dict(**extra, params=list(args.params), steps=args.steps, ssim_lambda=args.ssim_lambda, seed=args.seed, views=names,
                       strategy=args.strategy, **reg, config={k: getattr(cfg, k) for k in cfg.__dataclass_fields__}, loss=history["loss"], n=history["n"],
                       rounds=history["rounds"], resets=history["resets"], sh_degree=history["sh_degree"],
                       **({"adam": args.adam} if hasattr(args, "adam") else {}),
                       **({"means_lr": history["means_lr"]} if "means_lr" in history else {}),
                       **({"depth_loss": history["depth_loss"], "depth_lambda": getattr(args, "depth_lambda", 1e-2),
                           "depth_scale": scene_scale} if depth_loss else {})), f, indent=1)
    with open(os.path.join(args.out, "metrics.json"), "w") as f:
        json.dump(dict(before=before, after=after), f, indent=1)
    print(f"{n_start} -> {trained['means'].shape[0]} Gaussians in {len(history['rounds'])} rounds; loss {history['loss'][0]:.6e} -> "
          f"{history['loss'][-1]:.6e} over {len(history['loss'])} steps; mean PSNR {before['mean']['psnr']:.3f} -> "
          f"{after['mean']['psnr']:.3f} dB, SSIM {before['mean']['ssim']:.4f} -> {after['mean']['ssim']:.4f}")
    if feature_dim is not None:
        print(f"feature loss {history['feature_loss'][0]:.6e} -> {history['feature_loss'][-1]:.6e}; wrote features.pt")
    if "pose_err" in history:
        print(f"pose error {history['pose_err'][0]:.6e} -> {history['pose_err'][-1]:.6e}")
    print(f"wrote {args.out}: trained.pt, history.json, metrics.json" + (", poses.pt" if pose_kw else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
