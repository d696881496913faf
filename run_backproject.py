#!/usr/bin/env python3
"""Command-line counterpart of `python backproject.py` (reference main(): backproject.py:301-336), on the fused
HIP path.  Flag names follow the reference's tyro flags; the 2-D feature network (LSeg / DINOv2 weights are not
available offline) is replaced by per-view feature maps read from --feature-maps, or by --synthetic inputs.

    python run_backproject.py --synthetic C1 --results-dir /tmp/out
    python run_backproject.py --data-dir data/garden --checkpoint ckpt.pt --format gsplat --data-factor 4 \
        --feature-maps feats/ --feature lseg --results-dir results/garden
    torchrun --nproc-per-node 8 run_backproject.py ...      # views shard over ranks, one RCCL all-reduce
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--data-dir", default="./data/garden")
    ap.add_argument("--checkpoint", default="./data/garden/ckpts/ckpt_29999_rank0.pt")
    ap.add_argument("--results-dir", default="./results/garden")
    ap.add_argument("--format", choices=["inria", "gsplat", "ply"], default="gsplat")
    ap.add_argument("--rasterizer", choices=["inria", "gsplat"], default=None, help="deprecated alias of --format")
    ap.add_argument("--data-factor", type=int, default=4)
    ap.add_argument("--feature", choices=["lseg", "dino"], default="lseg")
    # The reference's main() also takes these two (backproject.py:309-310).  There feature_field_batch_count is handed to
    # create_feature_field_lseg and never read (backproject.py:25-27,77-82), and run_feature_field_on_cpu only moves the LSeg
    # NETWORK to the CPU (backproject.py:30-41) -- the rasterisation stays on the GPU either way.  Here the 2-D network is
    # replaced by supplied feature maps, so both are accepted for command-line compatibility and change nothing.
    ap.add_argument("--feature-field-batch-count", type=int, default=1,
                    help="accepted for compatibility with the reference's main() (unused there as well)")
    ap.add_argument("--run-feature-field-on-cpu", action=argparse.BooleanOptionalAction, default=False,
                    help="accepted for compatibility: the reference moves only its LSeg network to the CPU with it; the "
                         "feature maps are supplied here, the back-projection always runs on the GPU")
    maps = ap.add_mutually_exclusive_group()
    maps.add_argument("--feature-maps", default=None, help="directory with <image name>.pt tensors [H,W,D]")
    maps.add_argument("--label-maps", default=None,
                      help="directory with <image name>.pt INTEGER tensors [H,W] (a segmenter's class / instance ids, a mask; "
                           "another shape is a low-resolution map, upsampled with mode='nearest'): writes label_field.pt, the "
                           "[N, --num-classes] fraction of every Gaussian's blend weight per class, instead of a feature field")
    maps.add_argument("--mask-features", default=None, metavar="DIR",
                      help="directory with <image name>.pt files holding {'labels': [H,W] integer mask / instance ids (another "
                           "shape is a low-resolution map, upsampled with mode='nearest'), 'table': [M,D] one embedding per mask "
                           "(float32 / float16 / bfloat16)}: the feature map is table[labels] (a zero row outside [0, M)), "
                           "back-projected without materialising it; writes the same features_<feature>.pt as --feature-maps.  "
                           "With --synthetic: 'synthetic' for seeded Voronoi mask maps and tables (synthetic.make_mask_features)")
    ap.add_argument("--num-masks", type=int, default=200,
                    help="masks per view of --synthetic --mask-features synthetic (default 200)")
    ap.add_argument("--num-classes", type=int, default=None,
                    help="number of classes K of --label-maps (ids outside [0, K) are ignored); with --synthetic: use seeded "
                         "piecewise-constant (Voronoi) label maps with K classes instead of feature maps")
    ap.add_argument("--votes", choices=["binary", "projection", "gradient"], default=None,
                    help="with --label-maps (or --synthetic) and --num-classes: per-view votes of the label maps instead of the "
                         "label field (get_mask3d's voting_method; create_vote_field) on the loaded scene, not pruned: writes "
                         "votes.pt = {'counts': [N, K] votes, 'views': [N] views that voted, 'method'} and, for K = 2, "
                         "'mask3d' / 'mask3d_inverted' (votes for class 1 minus votes for class 0, > 0 / < 0)")
    ap.add_argument("--pixel-weights", default=None, metavar="DIR",
                    help="directory with <image name>.pt per-pixel weight maps [H,W] at the view's resolution (bool, uint8 with "
                         "non-zero = 1, float16, bfloat16 or float32): which pixels count and how much, for feature and label "
                         "maps alike.  With --synthetic: 'mask' or 'confidence' for the seeded maps of synthetic.make_pixel_weights")
    ap.add_argument("--encoder", default=None, help="[512,16] encoder tensor (.pt): backproject_compressed.py")
    ap.add_argument("--synthetic", default=None, help="run a seeded synthetic config (C1, C2, ...) instead of files")
    ap.add_argument("--no-prune", action="store_true",
                    help="skip the pruning step and build the field on ALL Gaussians (the default, like the reference's main(), "
                         "is prune_by_gradients -> test_proper_pruning -> build on the pruned scene, backproject.py:320-325)")
    ap.add_argument("--prune-by-product", action="store_true",
                    help="ONE sweep instead of two: build the field on all Gaussians and take the mask from the same "
                         "denominators (keep = d > 0), then drop the pruned rows.  Not the reference's arithmetic to the last "
                         "digit: a pruned Gaussian has no weight anywhere but may be the one that TERMINATES pixels "
                         "(T' <= 1e-4), so building with it present moves some kept rows (C2 size, two views: median 7e-9, "
                         "99 %% of the rows within 1.2e-7, 0.4 %% beyond 1e-3 of the prune-first result; tests/test_gpu_pruning.py)")
    ap.add_argument("--dist-backend", default="nccl", help="process-group backend under torchrun (nccl = RCCL over xGMI)")
    ap.add_argument("--one-device", action="store_true",
                    help="every rank uses cuda:0 (with --dist-backend gloo: the N > 1 bookkeeping on a one-GPU box)")
    # gsplat.rasterization's projection options (not flags of the reference's main(), which always rasterises pinhole / classic)
    ap.add_argument("--camera-model", choices=["pinhole", "ortho", "fisheye"], default=None,
                    help="camera model of the projection (default pinhole; gsplat's fisheye is the ideal equidistant model, "
                         "no distortion coefficients)")
    ap.add_argument("--rasterize-mode", choices=["classic", "antialiased"], default="classic",
                    help="antialiased: opacity x compensation, for scenes trained with gsplat's antialiased switch")
    ap.add_argument("--map-dtype", choices=["float32", "keep"], default="float32",
                    help="keep: hand fp16 / bf16 feature maps to the library as stored (read natively by the 128- and "
                         "256-channel kernels and token space, no fp32 copy); float32: convert every map first")
    return ap


def add_later_options(ap: argparse.ArgumentParser) -> argparse.ArgumentParser:
    """The options that came after the set tests/golden/cli_options.json records for build_parser(); main() declares both."""
    ap.add_argument("--sparse-slots", type=int, default=None, metavar="S",
                    help="with --label-maps (or --synthetic) and --num-classes: keep S (1 .. 32) (class, share) slots per Gaussian "
                         "instead of the dense [N, K] field (create_sparse_label_field: N * (12 S + 16) bytes whatever K): writes "
                         "sparse_label_field.pt = {'ids': int32 [N, S] (-1 empty), 'fractions': float32 [N, S], 'spill_fraction': "
                         "[N], 'total': int64 [N], 'num_classes', 'slots', 'stats'}, largest share first.  One process")
    ap.add_argument("--field-dtype", choices=["fp32", "fp16", "bf16"], default="fp32",
                    help="element type of the feature field that is written (features_<feature>.pt; not label fields): fp16 / bf16 "
                         "halve the file and the memory of everything that loads it.  The accumulators stay fp32 and the finalise "
                         "rounds once; run_segment.py, run_pca.py, run_cluster.py, run_transfer.py, run_regions.py, run_clean.py and "
                         "run_sample.py read such a field as it is stored")
    return ap


FIELD_DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def camera_warnings(cam, camera_model_arg):
    """One-line warnings about a COLMAP camera the projection does not model exactly: a fisheye model without --camera-model
    (it is projected as a pinhole), and fisheye distortion coefficients (gsplat's fisheye model ignores them too)."""
    out = []
    if cam.gsplat_camera_model == "fisheye":
        if camera_model_arg is None:
            out.append(f"warning: the COLMAP camera is {cam.model}, a fisheye model, and --camera-model was not given: "
                       "projecting as pinhole (pass --camera-model fisheye)")
        if cam.distortion.size and bool((cam.distortion != 0).any()):
            out.append(f"warning: the {cam.model} camera has non-zero distortion coefficients "
                       f"{[float(k) for k in cam.distortion]}; they are ignored (gsplat's fisheye model has none)")
    return out


def load_label_map(label_dir: str, image_name: str) -> torch.Tensor:
    """<label_dir>/<image name>.pt: an integer label map (uint8, bool, int16, int32 or int64), as stored."""
    lab = torch.load(os.path.join(label_dir, image_name + ".pt"))
    if not torch.is_tensor(lab) or lab.is_floating_point() or lab.is_complex() or lab.dim() != 2:
        raise SystemExit(f"{image_name}.pt in {label_dir}: a 2-D integer label tensor is required, got "
                         f"{lab.dtype if torch.is_tensor(lab) else type(lab).__name__}"
                         f"{' ' + str(tuple(lab.shape)) if torch.is_tensor(lab) else ''}")
    return lab


def load_mask_features(mask_dir: str, image_name: str):
    """<mask_dir>/<image name>.pt: {"labels": [h, w] integer map, "table": [M, D] float32 / float16 / bfloat16}, as stored."""
    m = torch.load(os.path.join(mask_dir, image_name + ".pt"))
    lab, tab = (m.get("labels"), m.get("table")) if isinstance(m, dict) else (None, None)
    if (not torch.is_tensor(lab) or lab.is_floating_point() or lab.is_complex() or lab.dim() != 2 or not torch.is_tensor(tab)
            or tab.dtype not in (torch.float32, torch.float16, torch.bfloat16) or tab.dim() != 2):
        raise SystemExit(f"{image_name}.pt in {mask_dir}: a dict with a 2-D integer 'labels' tensor and a 2-D float32 / float16 / "
                         "bfloat16 'table' tensor is required")
    return lab, tab


def load_pixel_weights(weight_dir: str, image_name: str, H: int, W: int) -> torch.Tensor:
    """<weight_dir>/<image name>.pt: an [H, W] weight map of a type the weighted blend reads."""
    c = torch.load(os.path.join(weight_dir, image_name + ".pt"))
    ok = (torch.float32, torch.float16, torch.bfloat16, torch.uint8, torch.bool)
    if not torch.is_tensor(c) or c.dtype not in ok or tuple(c.shape) != (H, W):
        raise SystemExit(f"{image_name}.pt in {weight_dir}: an [{H},{W}] bool / uint8 / float16 / bfloat16 / float32 weight map is "
                         f"required, got {c.dtype if torch.is_tensor(c) else type(c).__name__}"
                         f"{' ' + str(tuple(c.shape)) if torch.is_tensor(c) else ''}")
    return c


def main(argv=None):
    ap = add_later_options(build_parser())
    args = ap.parse_args(argv)
    labels_mode = bool(args.label_maps) or (bool(args.synthetic) and args.num_classes is not None)
    if labels_mode and (args.num_classes is None or args.num_classes < 1):
        ap.error("--label-maps needs --num-classes K >= 1")
    if labels_mode and args.encoder:
        ap.error("--encoder applies to feature maps, not to --label-maps / --num-classes")
    if args.votes and not labels_mode:
        ap.error("--votes needs label maps: --label-maps DIR --num-classes K, or --synthetic CFG --num-classes K")
    if args.sparse_slots is not None and (not labels_mode or args.votes or not 1 <= args.sparse_slots <= 32):
        ap.error("--sparse-slots S (1 .. 32) goes with --label-maps DIR --num-classes K (or --synthetic CFG --num-classes K), "
                 "without --votes")
    if args.sparse_slots is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--sparse-slots runs in one process (the slot lists of two ranks are not merged)")
    masks_mode = bool(args.mask_features)
    if masks_mode and (args.encoder or args.num_classes is not None):
        ap.error("--mask-features takes neither --encoder nor --num-classes")
    if masks_mode and args.synthetic and args.mask_features != "synthetic":
        ap.error("with --synthetic, --mask-features takes 'synthetic' (seeded mask maps)")
    if masks_mode and args.num_masks < 1:
        ap.error("--num-masks must be positive")
    camera_model = args.camera_model or "pinhole"
    cam_kw = dict(camera_model=camera_model, rasterize_mode=args.rasterize_mode)

    import gsbp_amd  # BEFORE the first HIP call: the package asks the runtime for the hardware queues its view pipeline needs
    if not torch.cuda.is_available():
        raise RuntimeError("a HIP device is required (the reference likewise requires CUDA, backproject.py:314)")
    import torch.distributed as dist
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        torch.cuda.set_device(0 if args.one_device else int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group(args.dist_backend)
    dev = torch.device("cuda", torch.cuda.current_device())
    rank = dist.get_rank() if dist.is_initialized() else 0

    from gsbp_amd import cli, scene_io, synthetic as syn

    # (a synthetic scene is activated on the device, a checkpoint on the host, backproject.py:55-57 -- as ever: the last bit differs)
    scene = cli.load_scene(args, dev, activate_on_host=not args.synthetic)
    splats, (means, quats, scales, opac), K, viewmats, W, H = scene[:6]  # splats: pre-activation, the reference's key names
    names, cfg = scene.names, scene.cfg  # the views in the reference's order: images sorted by name (backproject.py:74)
    if args.synthetic:
        dim = cfg.feat_dim
        encoder = syn.make_encoder(cfg).to(dev) if cfg.encoder_dim else None

        # (DINO64 / LSEG480: the network's own low-resolution map, upsampled inside the kernels like the reference's F.interpolate)
        upsample = cfg.upsample
        reduction = cfg.reduction if cfg.lowres else ("mean" if args.feature == "dino" else "sum")

        def feature_fn(v):
            return syn.make_feature_map(cfg, v, device=dev)

        def label_fn(v):
            return syn.make_label_map(cfg, v, args.num_classes, device=dev)
        label_upsample = None

        def mask_fn(v):
            return syn.make_mask_features(cfg, v, args.num_masks, dim, device=dev)
        pixel_weight_fn = None
        if args.pixel_weights:
            if args.pixel_weights not in ("mask", "confidence"):
                raise SystemExit("--pixel-weights with --synthetic takes 'mask' or 'confidence'")

            def pixel_weight_fn(v):
                return syn.make_pixel_weights(cfg, v, device=dev, kind=args.pixel_weights)
    else:
        splats = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in splats.items()}
        if rank == 0:
            for line in camera_warnings(next(iter(splats["colmap_project"].cameras.values())), args.camera_model):
                print(line, file=sys.stderr)
        if labels_mode:
            # a map at another resolution than the view's is read with F.interpolate(mode="nearest")'s index maps in the kernel
            first_labels = load_label_map(args.label_maps, names[0])
            label_upsample = "nearest" if tuple(first_labels.shape) != (H, W) else None

            def label_fn(v):
                return load_label_map(args.label_maps, names[v]).to(dev)
        elif masks_mode:
            first_labels, first_table = load_mask_features(args.mask_features, names[0])
            label_upsample = "nearest" if tuple(first_labels.shape) != (H, W) else None
            dim = int(first_table.shape[1])

            def mask_fn(v):
                lab, tab = load_mask_features(args.mask_features, names[v])
                return lab.to(dev), tab.to(dev)
        elif not args.feature_maps:
            raise SystemExit("--feature-maps is required (no LSeg/DINO weights offline)")
        encoder = torch.load(args.encoder).to(dev).float() if args.encoder else None
        first = (torch.load(os.path.join(args.feature_maps, names[0] + ".pt"))
                 if not (labels_mode or masks_mode) else None)
        if not masks_mode:
            dim = first.shape[-1] if first is not None else None
        # A map at the network's resolution is upsampled the way the reference does it -- bilinear for lseg (backproject.py:110-112),
        # nearest for dino's patch tokens (:244-248) -- INSIDE the kernels (dino maps whose tokens cover a tile: token space); with an
        # encoder the map is materialised first (the encoder-fused kernels read full-resolution pixels)
        pixel_weight_fn = None
        if args.pixel_weights:
            def pixel_weight_fn(v):
                return load_pixel_weights(args.pixel_weights, names[v], H, W).to(dev)
        mode = "nearest" if args.feature == "dino" else "bilinear"
        upsample = mode if (first is not None and tuple(first.shape[:2]) != (H, W) and encoder is None) else None
        reduction = "mean" if args.feature == "dino" else "sum"  # backproject.py:263,283 vs :127,145

        def feature_fn(v):
            f = torch.load(os.path.join(args.feature_maps, names[v] + ".pt")).to(dev)
            if args.map_dtype == "float32" or f.dtype not in (torch.float16, torch.bfloat16):
                f = f.float()
            if upsample is not None or tuple(f.shape[:2]) == (H, W):
                return f
            f = f.float()  # (a map the CLI upsamples itself: interpolated in fp32, as before)
            kw = {"align_corners": False} if mode == "bilinear" else {}
            return torch.nn.functional.interpolate(f.permute(2, 0, 1)[None], size=(H, W), mode=mode, **kw)[0].permute(1, 2, 0)

    # backproject.py:323-325: splats_optimized = prune_by_gradients(splats); test_proper_pruning(splats, splats_optimized);
    # the field is then built on the PRUNED scene.  The mask costs one blend per view (no scatter).  Under a process group
    # the sweep AND the render check are sharded over the ranks by view like the field build itself (round 4 had rank 0 do
    # both alone while the others waited: ~0.3 s at C2 against a 0.09 s field build per rank at 8 GPUs); the weight sums are
    # all-reduced, so every rank holds the SAME mask and the shapes of the collectives that follow agree by construction.
    n_all = means.shape[0]
    keep = None

    def report_and_check(keep):
        if rank == 0:
            print("Total splats", keep.numel())  # utils.py:258-260
            print("Pruned", int((~keep).sum()), "splats")
            print("Remaining", int(keep.sum()), "splats")
        if "features_dc" in splats:  # utils.test_proper_pruning renders with the SH colours (checkpoints only)
            pruned = {k: (v[keep] if k in gsbp_amd.pruning.PER_GAUSSIAN else v) for k, v in splats.items()}
            rep = gsbp_amd.check_proper_pruning(splats, pruned, viewmats, K, W, H, **cam_kw)
            if rank == 0:
                print("Percentage pruned: ", rep["percentage_pruned"])  # utils.py:348-359
                print("Max pixel error: ", rep["max_pixel_error"])
                print("Total pixel error: ", rep["total_pixel_error"])

    if args.votes:
        # get_mask3d (affordance_transfer/demo_affordance_transfer.py) votes on the loaded Gaussians: no prune step
        C, n, stats = gsbp_amd.create_vote_field(means, quats, scales, opac, viewmats, K, W, H, label_fn, args.num_classes,
                                                 method=args.votes, upsample=label_upsample, return_partials=True,
                                                 pixel_weight_fn=pixel_weight_fn, **cam_kw)
        if rank == 0:
            out = {"counts": C.cpu(), "views": n.cpu(), "method": args.votes}
            if args.num_classes == 2:
                out["mask3d"], out["mask3d_inverted"] = (m.cpu() for m in gsbp_amd.mask3d_from_votes(C))
            os.makedirs(args.results_dir, exist_ok=True)
            path = os.path.join(args.results_dir, "votes.pt")
            torch.save(out, path)
            print("saved", path, tuple(C.shape), stats)
        if dist.is_initialized():
            dist.destroy_process_group()
        return

    if not args.no_prune and not args.prune_by_product:
        keep = gsbp_amd.pruning.gradient_mask(splats, viewmats, K, W, H, **cam_kw)
        report_and_check(keep)
        means, quats, scales, opac = means[keep], quats[keep], scales[keep], opac[keep]

    if labels_mode and args.sparse_slots is not None:
        # the same prune step, then every Gaussian's non-zero class fractions in S slots (sparse_label_field.pt)
        field = gsbp_amd.create_sparse_label_field(means, quats, scales, opac, viewmats, K, W, H, label_fn, args.num_classes,
                                                   slots=args.sparse_slots, pixel_weight_fn=pixel_weight_fn,
                                                   upsample=label_upsample, **cam_kw)
        if args.prune_by_product and not args.no_prune:
            keep = field.total > 0
            report_and_check(keep)
            field = gsbp_amd.SparseLabelField(*(t[keep] for t in field))
        over = int((field.spill_fraction > 0).sum())
        stats = {"overflow_rows": over, "slots_in_use": torch.bincount((field.ids >= 0).sum(dim=1),
                                                                       minlength=args.sparse_slots + 1).tolist()}
        if rank == 0:
            os.makedirs(args.results_dir, exist_ok=True)
            path = os.path.join(args.results_dir, "sparse_label_field.pt")
            torch.save({**{k: t.cpu() for k, t in field._asdict().items()}, "num_classes": args.num_classes,
                        "slots": args.sparse_slots, "stats": stats}, path)
            print("saved", path, tuple(field.ids.shape), f"(of {n_all} Gaussians)", stats)
            if over:
                print(f"warning: {over} Gaussians saw more than {args.sparse_slots} classes; their spill_fraction says how much "
                      "weight has no slot (raise --sparse-slots)", file=sys.stderr)
            if keep is not None:
                torch.save(keep.cpu(), os.path.join(args.results_dir, "prune_mask.pt"))
        if dist.is_initialized():
            dist.destroy_process_group()
        return

    if labels_mode:
        # the same prune step, then the [N_kept, K] class fractions of every Gaussian's blend weight (label_field.pt)
        out, F, d, stats = gsbp_amd.create_label_field(means, quats, scales, opac, viewmats, K, W, H, label_fn,
                                                       args.num_classes, upsample=label_upsample, return_partials=True,
                                                       pixel_weight_fn=pixel_weight_fn, **cam_kw)
    elif masks_mode:
        # the feature field of the maps table[labels], built from the masks and their embeddings (features_<feature>.pt)
        out, F, d, stats = gsbp_amd.create_mask_feature_field(means, quats, scales, opac, viewmats, K, W, H, mask_fn, dim,
                                                              reduction=reduction, upsample=label_upsample,
                                                              return_partials=True, pixel_weight_fn=pixel_weight_fn,
                                                              out_dtype=FIELD_DTYPES[args.field_dtype], **cam_kw)
    else:
        out, F, d, stats = gsbp_amd.create_feature_field(means, quats, scales, opac, viewmats, K, W, H, feature_fn, dim,
                                                         reduction=reduction, encoder=encoder, return_partials=True,
                                                         verbose=True, upsample=upsample, pixel_weight_fn=pixel_weight_fn,
                                                         out_dtype=FIELD_DTYPES[args.field_dtype], **cam_kw)
    if args.prune_by_product and not args.no_prune:
        # "the mask comes free from the fused kernel" -- d is the all-reduced denominator of every Gaussian,
        # identical on every rank
        keep = d > 0
        report_and_check(keep)
        out = out[keep]
    if rank == 0:
        name = ("label_field.pt" if labels_mode else "features_lseg_compressed.pt" if encoder is not None
                else f"features_{args.feature}.pt")
        print("saved", scene_io.save_features(out.cpu(), args.results_dir, name), tuple(out.shape),
              f"(of {n_all} Gaussians)", stats)
        if keep is not None:  # the rows of the features file are the kept Gaussians, in order (like the reference's)
            torch.save(keep.cpu(), os.path.join(args.results_dir, "prune_mask.pt"))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
