"""What the run_*.py command lines share: the scene options, the "needs a GPU" exit, the scene itself -- a checkpoint with its
COLMAP cameras, or a seeded synthetic config -- and the frame writer.  Importing this module does no work and needs no GPU.

    ap = argparse.ArgumentParser(); cli.add_scene_arguments(ap); args = ap.parse_args()
    cli.require_gpu("run_x.py")
    scene = cli.load_scene(args, torch.device("cuda"))      # splats, gauss, K, viewmats, width, height, names, cfg
    scene = scene.first_views(args.max_views)               # where the command line truncates
"""
from __future__ import annotations

import os
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import scene_io, synthetic as syn

# the names the command lines give a field's element type (--field-dtype, --out-dtype)
FIELD_DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
SCENE_OPTIONS = ("data-dir", "checkpoint", "format", "data-factor", "synthetic", "camera-model", "rasterize-mode", "max-views")


def add_scene_arguments(ap, *, only: Optional[Sequence[str]] = None, max_views_help: str = "score only the first views",
                        camera_model_default: Optional[str] = "pinhole") -> None:
    """Declare the scene options on ap, in the order of SCENE_OPTIONS.  only: the names (without dashes) to declare with this
    call, for a command line that takes a subset or has options of its own between them."""
    options = {
        "data-dir": dict(default="./data/garden"),
        "checkpoint": dict(default="./data/garden/ckpts/ckpt_29999_rank0.pt"),
        "format": dict(choices=["inria", "gsplat", "ply"], default="gsplat"),
        "data-factor": dict(type=int, default=4),
        "synthetic": dict(default=None, help="a seeded synthetic config (C1, ...) instead of files"),
        "camera-model": dict(choices=["pinhole", "ortho", "fisheye"], default=camera_model_default),
        "rasterize-mode": dict(choices=["classic", "antialiased"], default="classic"),
        "max-views": dict(type=int, default=None, help=max_views_help),
    }
    unknown = set(only or ()) - set(options)
    if unknown:
        raise ValueError(f"no scene options {sorted(unknown)}")
    for name in SCENE_OPTIONS:
        if only is None or name in only:
            ap.add_argument("--" + name, **options[name])


def require_gpu(prog: str) -> None:
    if not torch.cuda.is_available():
        raise SystemExit(f"{prog} needs a GPU (there is no CPU path)")


class Scene(NamedTuple):
    splats: Dict            # the pre-activation parameters under the reference's key names, tensors on the device
    gauss: Tuple            # (means, quats, scales, opacities): activated, float32, on the device
    K: torch.Tensor         # [3, 3]
    viewmats: torch.Tensor  # [V, 4, 4]: a checkpoint's images sorted by name
    width: int
    height: int
    names: List[str]        # per view: the image's name, view_0000 ... of a synthetic scene
    cfg: Optional[syn.Config]  # the synthetic config, None for a checkpoint

    def first_views(self, n: Optional[int]) -> "Scene":
        """The scene with its first n views (--max-views); all of them with n None."""
        return self if n is None else self._replace(viewmats=self.viewmats[:n], names=self.names[:n])


def load_scene(args, dev, activate_on_host: bool = False) -> Scene:
    """The scene of the parsed scene options: --synthetic CFG (synthetic.make_scene and its cameras), else --checkpoint / --data-dir /
    --format / --data-factor (scene_io.load_checkpoint; width and height are twice the principal point, backproject.py:85-86).
    activate_on_host: exp and sigmoid run before the parameters move to the device instead of after; the two differ in the last
    bit, and each command line keeps the order it has always had."""
    if args.synthetic:
        cfg = syn.CONFIGS[args.synthetic]
        splats = syn.make_scene(cfg)
        K, viewmats, width, height = syn.intrinsics(cfg).to(dev), syn.make_cameras(cfg).to(dev), cfg.width, cfg.height
        names = [f"view_{v:04d}" for v in range(viewmats.shape[0])]
    else:
        cfg = None
        splats = scene_io.load_checkpoint(args.checkpoint, args.data_dir, format=args.format, data_factor=args.data_factor,
                                          rasterizer=getattr(args, "rasterizer", None))
        K = splats["camera_matrix"].float().to(dev)
        width, height = int(K[0, 2] * 2), int(K[1, 2] * 2)
        viewmats = scene_io.sorted_viewmats(splats["colmap_project"]).to(dev)
        names = sorted(im.name for im in splats["colmap_project"].images.values())
    on_dev = {k: (t.to(dev) if torch.is_tensor(t) else t) for k, t in splats.items()}
    gauss = tuple(t.to(dev).float() for t in syn.activate(splats if activate_on_host else on_dev))
    return Scene(on_dev, gauss, K, viewmats, width, height, names, cfg)


class FrameWriter:
    """frame_0000.png ... in a directory when PIL imports, else one frames.pt (uint8 [C, H, W, 3]) there."""

    def __init__(self, directory: str):
        os.makedirs(directory, exist_ok=True)
        self.dir, self.kept = directory, []
        try:
            from PIL import Image
            self.image = Image
        except ImportError:
            self.image = None

    def add(self, v: int, frame: torch.Tensor) -> None:
        if self.image is not None:
            self.image.fromarray(frame.cpu().numpy(), "RGB").save(os.path.join(self.dir, f"frame_{v:04d}.png"))
        else:
            self.kept.append(frame.cpu())

    def close(self) -> None:
        if self.image is None and self.kept:
            torch.save(torch.stack(self.kept), os.path.join(self.dir, "frames.pt"))
