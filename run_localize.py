#!/usr/bin/env python3
"""Where was this image, or this feature map, taken from?  Refines a camera pose against a target by gradient descent through the
rasteriser (gsbp_amd.refine_pose: rasterization(camera_grad=True), the HIP blend and projection backward kernels).

    python run_localize.py --checkpoint ckpt.pt --data-dir data/garden --target photo.npy --init-view 12 --out pose.json
    python run_localize.py --checkpoint ckpt.pt --data-dir data/garden --field pca16.pt --target map16.pt --loss cosine \\
        --init-pose guess.json --steps 200 --out pose.json
    python run_localize.py --synthetic T0 --target target.pt --init-view 0 --perturb 0.03,-0.02,0.02,0.05,-0.04,0.03 --out pose.json

The table rendered against the target is the scene's RGB (the SH DC colours; a seeded random table for a synthetic scene), or --field:
a .pt / .npy tensor [N, D] with D <= 32 -- a PCA or compressed field qualifies, a 512-channel one does not.  --target: .npy / .pt
[H, W, D] at the scene's resolution; --weights: [H, W], optional.  The initial pose is --init-pose (a 4 x 4 world-to-camera matrix in a
.json list, .npy or .pt) or the scene's view --init-view, either one moved by --perturb (a twist: rotation vector, then translation).
--out: JSON with the refined "viewmat" (4 x 4), the "twist" found, the loss "history" (one value per step) and the initial pose.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gsbp_amd import cli  # noqa: E402

MAX_DIM = 32
C0 = 0.28209479177387814
RGB_SEED = 4242


def load_array(path: str) -> torch.Tensor:
    """A tensor from .pt, .npy or .json."""
    if path.endswith(".npy"):
        import numpy as np
        return torch.from_numpy(np.load(path))
    if path.endswith(".json"):
        with open(path) as f:
            data = json.load(f)
        return torch.tensor(data["viewmat"] if isinstance(data, dict) else data)
    return torch.as_tensor(torch.load(path, map_location="cpu"))


def parse_twist(text: str):
    try:
        vals = [float(x) for x in text.split(",")]
    except ValueError:
        vals = []
    if len(vals) != 6:
        raise argparse.ArgumentTypeError(f"a twist is six comma-separated numbers (rotation vector, translation), got {text!r}")
    return vals


def scene_rgb(scene, dev) -> torch.Tensor:
    """[N, 3]: the SH DC colours of a checkpoint (+ 0.5, clamped at 0); a seeded random table for a synthetic scene, which has none."""
    if "features_dc" in scene.splats:
        return (scene.splats["features_dc"].float().reshape(-1, 3) * C0 + 0.5).clamp_min(0.0).contiguous()
    n = scene.gauss[0].shape[0]
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(RGB_SEED)).to(dev)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    cli.add_scene_arguments(ap, only=[o for o in cli.SCENE_OPTIONS if o != "max-views"])
    ap.add_argument("--field", default=None, help=f".pt / .npy [N, D], D <= {MAX_DIM}: the table to render (default: the scene's RGB)")
    ap.add_argument("--target", required=True, help=".npy / .pt [H, W, D]: the image or feature map to localise")
    ap.add_argument("--weights", default=None, help=".npy / .pt [H, W]: per-pixel weights of the loss")
    start = ap.add_mutually_exclusive_group(required=True)
    start.add_argument("--init-pose", default=None, help="a 4 x 4 world-to-camera matrix (.json, .npy, .pt)")
    start.add_argument("--init-view", type=int, default=None, help="start from this view of the scene")
    ap.add_argument("--perturb", type=parse_twist, default=None, metavar="W0,W1,W2,V0,V1,V2", help="a twist applied to the initial pose")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--loss", choices=["l2", "cosine", "photometric"], default="l2",
                    help="photometric: the trainer's (1 - lambda) L1 + lambda (1 - SSIM), from the fused kernels")
    ap.add_argument("--ssim-lambda", type=float, default=0.2, help="lambda of --loss photometric")
    ap.add_argument("--out", required=True, help="the JSON file to write")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.synthetic and not os.path.exists(args.checkpoint):
        ap.error(f"give --synthetic CFG, or --checkpoint / --data-dir of a scene ({args.checkpoint} does not exist)")
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    import gsbp_amd
    cli.require_gpu("run_localize.py")
    dev = torch.device("cuda")
    scene = cli.load_scene(args, dev)
    n = scene.gauss[0].shape[0]
    table = scene_rgb(scene, dev) if args.field is None else load_array(args.field).to(dev).float().contiguous()
    if table.dim() != 2 or table.shape[0] != n or table.shape[1] > MAX_DIM:
        ap.error(f"the table must be [{n}, D] with D <= {MAX_DIM}, got {tuple(table.shape)}: project a wider field first "
                 "(run_pca.py, or the compressed lift)")
    target = load_array(args.target).to(dev).float()
    if target.dim() == 2:
        target = target[..., None]
    if tuple(target.shape) != (scene.height, scene.width, table.shape[1]):
        ap.error(f"the target must be [{scene.height}, {scene.width}, {table.shape[1]}], got {tuple(target.shape)}")
    weights = None if args.weights is None else load_array(args.weights).to(dev).float()
    if args.init_pose is not None:
        vm0 = load_array(args.init_pose).double().reshape(4, 4)
    else:
        if not 0 <= args.init_view < scene.viewmats.shape[0]:
            ap.error(f"--init-view {args.init_view}: the scene has views 0..{scene.viewmats.shape[0] - 1}")
        vm0 = scene.viewmats[args.init_view].double().cpu()
    if args.perturb is not None:
        vm0 = gsbp_amd.se3_exp(torch.tensor(args.perturb, dtype=torch.float64)) @ vm0
    res = gsbp_amd.refine_pose(*scene.gauss, table, target, vm0, scene.K, scene.width, scene.height, steps=args.steps, lr=args.lr,
                               weights=weights, loss=args.loss, camera_model=args.camera_model, rasterize_mode=args.rasterize_mode,
                               ssim_lambda=args.ssim_lambda)
    angle, dist = gsbp_amd.pose_error(res["viewmat"], vm0)
    report = {"viewmat": res["viewmat"].double().cpu().tolist(), "twist": res["twist"].cpu().tolist(), "history": res["history"],
              "initial_viewmat": vm0.tolist(), "moved": {"angle_rad": angle, "distance": dist}, "loss": args.loss, "steps": args.steps,
              "lr": args.lr, "channels": int(table.shape[1])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print(f"wrote {args.out}: loss {res['history'][0]:.4g} -> {res['history'][-1]:.4g} in {args.steps} steps; the pose moved "
          f"{angle:.4f} rad and {dist:.4f} from the initial one")
    return 0


if __name__ == "__main__":
    sys.exit(main())
