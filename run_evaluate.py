#!/usr/bin/env python3
"""Command-line counterpart of the reference's evaluate_results / render_affordance (affordance_transfer/demo_affordance_transfer.py:
1445-1611, 1399-1439): render per-Gaussian labels to 2-D class maps, score them against ground-truth label maps (mIoU, recall) and
write the segmentation and the tinted frames, all on the HIP path (one blend pass per view, the counts made in the kernel).

    python run_evaluate.py --labels labels.pt --gt gt/ --data-dir data/scene --checkpoint ckpt.pt --out eval/
    python run_evaluate.py --synthetic C1 --num-classes 8 --out /tmp/eval          # a seeded scene, seeded labels and label maps

--labels: a .pt integer tensor [N] (or [N, 1]), one class id per Gaussian (transfer_labels' output).  --gt DIR: per view
<image name without extension>.pt or .npy, an integer [H, W] label map; a view without a file is skipped, as the reference skips its
automatically labelled views.  --num-classes: by default the largest label + 1.  --cut: a pixel is predicted for a class when
uint8(clamp(opacity, 0, 1) * 255) > cut (the reference's 64).  Writes into --out: counts.pt (int64 [V, K, 3]: intersection,
predicted, ground truth), metrics.json (per-class IoU and recall, mIoU, recall), argmax/ and tinted/ with one frame_0000.png ... per
view when PIL imports, else frames.pt (uint8 [V, H, W, 3]) in each; with --synthetic also labels.pt.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gsbp_amd import cli  # noqa: E402

# render_affordance's palette (class 0, the background, grey)
PALETTE = [[125, 125, 125], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255], [128, 0, 0]]
LABEL_SEED = 60_000


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", default=None, help=".pt integer tensor [N]: one class id per Gaussian")
    ap.add_argument("--gt", default=None, help="directory of <image name>.pt / .npy integer [H, W] label maps")
    ap.add_argument("--cut", type=int, default=64, help="predicted where uint8(clamp(opacity, 0, 1) * 255) > cut")
    ap.add_argument("--num-classes", type=int, default=None)
    ap.add_argument("--min-opacity", type=float, default=0.0, help="argmax frames: -1 (black) below this opacity")
    cli.add_scene_arguments(ap)
    ap.add_argument("--out", default="./results/evaluate")
    return ap


def palette_of(k: int) -> torch.Tensor:
    """[k, 3] in [0, 1]: the reference's eight colours, then seeded random ones."""
    extra = torch.rand(max(0, k - len(PALETTE)), 3, generator=torch.Generator().manual_seed(LABEL_SEED))
    return torch.cat([torch.tensor(PALETTE, dtype=torch.float32) / 255.0, extra])[:max(k, 1)]


def load_gt(directory: str, name: str):
    stem = os.path.splitext(name)[0]
    for ext in (".pt", ".npy"):
        path = os.path.join(directory, stem + ext)
        if os.path.exists(path):
            if ext == ".pt":
                return torch.as_tensor(torch.load(path, map_location="cpu"))
            import numpy as np
            return torch.from_numpy(np.load(path))
    return None


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.synthetic and not (args.labels and args.gt):
        ap.error("give --labels and --gt (and the scene arguments), or --synthetic")
    import gsbp_amd
    from gsbp_amd import synthetic as syn
    cli.require_gpu("run_evaluate.py")
    dev = torch.device("cuda")
    os.makedirs(args.out, exist_ok=True)
    if args.synthetic and args.num_classes is None:
        ap.error("--synthetic needs --num-classes")
    scene = cli.load_scene(args, dev)
    splats, gauss, K, W, H, cfg = scene.splats, scene.gauss, scene.K, scene.width, scene.height, scene.cfg
    if args.synthetic:
        splats["features_dc"] = (torch.rand(cfg.n_gaussians, 1, 3, generator=torch.Generator().manual_seed(syn.SH_SEED)).to(dev)
                                 - 0.5) / gsbp_amd.label_render.C0
        splats["features_rest"] = torch.zeros(cfg.n_gaussians, 0, 3, device=dev)
        if args.labels:
            labels = torch.load(args.labels, map_location="cpu")
        else:
            labels = torch.randint(0, args.num_classes, (cfg.n_gaussians,), generator=torch.Generator().manual_seed(LABEL_SEED))
            torch.save(labels, os.path.join(args.out, "labels.pt"))

        def gt_of(v):
            return syn.make_label_map(cfg, v, args.num_classes, device=dev)
    else:
        labels = torch.load(args.labels, map_location="cpu")

        def gt_of(v):
            return load_gt(args.gt, scene.names[v])
    labels = torch.as_tensor(labels).reshape(-1).long().to(dev)
    n = splats["means"].shape[0]
    if labels.shape[0] != n:
        raise SystemExit(f"{labels.shape[0]} labels for {n} Gaussians")
    k = args.num_classes if args.num_classes is not None else int(labels.max()) + 1
    scene = scene.first_views(args.max_views)
    viewmats, names = scene.viewmats, scene.names
    raster_kw = dict(camera_model=args.camera_model, rasterize_mode=args.rasterize_mode)

    counts = gsbp_amd.score_label_views(*gauss, labels, k, viewmats, K, W, H, gt_of, cut=args.cut, **raster_kw)
    torch.save(counts.cpu(), os.path.join(args.out, "counts.pt"))
    metrics = gsbp_amd.miou_recall(counts)
    scored = [v for v in range(viewmats.shape[0]) if bool(counts[v].any())]
    with open(os.path.join(args.out, "metrics.json"), "w") as f:
        json.dump(dict(metrics, iou={str(i): x for i, x in metrics["iou"].items()},
                       recall={str(i): x for i, x in metrics["recall"].items()}, num_classes=k, cut=args.cut,
                       views=len(names), scored_views=len(scored)), f, indent=1)
    print(f"mIoU {metrics['miou']:.4f}  recall {metrics['mean_recall']:.4f}  ({len(scored)} of {len(names)} views scored, "
          f"{metrics['n_present']} classes present)")

    palette = palette_of(k).to(dev)
    shade = torch.cat([torch.zeros(1, 3, device=dev), palette])  # -1 (nothing, or below --min-opacity) is black
    tinted = gsbp_amd.recolor_by_labels(splats, labels, palette)
    sh = torch.cat([tinted["features_dc"], tinted["features_rest"]], dim=1).float()
    sh_degree = {1: 0, 4: 1, 9: 2, 16: 3}[sh.shape[1]]
    writers = {name: cli.FrameWriter(os.path.join(args.out, name)) for name in ("argmax", "tinted")}
    for v in range(viewmats.shape[0]):
        seg = gsbp_amd.render_label_argmax(*gauss, labels, k, viewmats[v], K, W, H, min_opacity=args.min_opacity, **raster_kw)
        writers["argmax"].add(v, (shade[seg.long() + 1] * 255.0).to(torch.uint8))
        rgb = gsbp_amd.rasterization(*gauss, sh, viewmats[v:v + 1], K[None], W, H, sh_degree=sh_degree, want_meta=False,
                                     backgrounds=torch.ones(1, 3, device=dev), **raster_kw)[0][0]
        writers["tinted"].add(v, (rgb * 255.0).clamp_(0.0, 255.0).to(torch.uint8))
    for w in writers.values():
        w.close()
    print(f"wrote {args.out}: counts.pt, metrics.json, argmax/, tinted/ for {viewmats.shape[0]} views")
    return 0


if __name__ == "__main__":
    sys.exit(main())
