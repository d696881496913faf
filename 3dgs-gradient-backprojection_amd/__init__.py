"""MI355X-native gradient-weighted feature back-projection (the hot path of backproject.py of
JojiJoseph/3dgs-gradient-backprojection), hand-written HIP kernels behind a C ABI (include/gwbp.h).

    from gsbp_amd import rasterization            # drop-in for `from gsplat import rasterization`
    from gsbp_amd import create_feature_field     # fused counterpart of create_feature_field_lseg/_dino
    from gsbp_amd import create_label_field       # integer label maps -> per-Gaussian class weights
    from gsbp_amd import create_mask_feature_field  # mask maps + one embedding per mask -> feature field
    from gsbp_amd import create_vote_field          # per-view binary / projection / gradient votes -> 3-D masks
    from gsbp_amd import knn_search, transfer_labels  # few-shot labels on a finished field: exact inner-product k-NN + majority
    from gsbp_amd import fit_pca, pca_colors, render_pca  # look at a finished field: PCA fit, colours and frames (visualize_pca.py)
    from gsbp_amd import prompt_mask, probe_pixels, render_prompt_mask, ClickSession  # ask a finished field: prompts and clicks
    from gsbp_amd import render_label_maps, render_label_argmax, score_label_views, miou_recall  # per-Gaussian labels -> 2-D class
    from gsbp_amd import recolor_by_labels          # maps, their mIoU / recall against ground truth, and the scene tinted by label
    from gsbp_amd import render_field_agreement, score_field_views, field_fidelity, agreement_weights  # a field scored against the
                                                    # maps it was lifted from, fused; and the weight map for a second, robust lift
    from gsbp_amd import decoded_loss, decoded_field_gradients, fit_decoded_field, decode_field  # a latent field and its decoder
                                                    # fitted on frozen Gaussians (the reference's Feature-3DGS baseline), fused
    from gsbp_amd import spatial_knn, knn_distances, init_scales  # which Gaussians are next to each other: exact 3-D k-NN on a grid
    from gsbp_amd import smooth_labels, smooth_mask, remove_outliers, smooth_features  # and a finished lift cleaned with it
    from gsbp_amd import fit_kmeans, kmeans_assign, cluster_sums, class_prototypes  # a field clustered without prompts: k-means on
    from gsbp_amd import quantize_field, dequantize_field, codebook_prompt_scores   # the matrix cores; the field as a codebook
    from gsbp_amd import radius_components, radius_count, suggest_radius  # which Gaussians form one object: radius components
    from gsbp_amd import select_components, split_instances  # (DBSCAN on the grid), and masks / label fields split into instances
    from gsbp_amd import associate_masks, associated_label_fn, match_masks, remap_masks  # per-view instance masks with unrelated ids
                                                    # associated into consistent 3-D groups: integer overlap and vote kernels
    from gsbp_amd import new_sparse_votes, sparse_votes_groups, sparse_votes_canonical, sparse_votes_dense, sparse_votes_stats
    from gsbp_amd import create_sparse_label_field, sparse_label_argmax, sparse_label_dense  # the votes in per-Gaussian slot lists:
                                                    # thousands of groups or classes without a dense [N, K] table
    from gsbp_amd import similarity_components, similarity_levels, neighbor_similarity  # regions by geometry AND features: the
    from gsbp_amd import edge_strength, region_prompt_mask  # spatial k-NN graph cut where the features' cosine falls below a threshold
    from gsbp_amd import point_gaussians, sample_field, sample_labels, transfer_field, score_point_labels  # the field and its labels
                                                    # at arbitrary 3-D points, by each Gaussian's own scale, rotation and opacity
    from gsbp_amd import pixel_gaussians, render_id_map, median_depth, pick_gaussians, lookup  # which Gaussians a pixel is made of:
                                                    # per-pixel top-k lists, id maps, median depth, and a click -> Gaussian indices
    from gsbp_amd import project_torch, sh_colors_torch  # rasterization() also trains: gradients w.r.t. means, quats, scales and
                                                    # opacities -- a HIP blend backward, then a HIP projection backward; these are the
                                                    # torch restatements the tests measure them against
    from gsbp_amd import sh_colors                  # the SH colours of a training step and their gradients w.r.t. coefficients (stored
                                                    # in one table or as features_dc + features_rest) and means: a HIP kernel pair
    from gsbp_amd import refine_pose, se3_exp, pose_error  # and it localises: rasterization(camera_grad=True) differentiates the view
                                                    # matrix; refine_pose finds where an image or feature map was taken from
    from gsbp_amd import photometric_loss, image_metrics, ssim_map, image_sums, gaussian_window  # the loss scenes are trained with,
                                                    # (1 - lambda) L1 + lambda (1 - SSIM), and PSNR / SSIM: a fused HIP kernel pair
    from gsbp_amd import polish_scene, score_image_views  # Adam on chosen tensors of a fixed set of Gaussians against images
    from gsbp_amd import train_scene, densify, DensifyState, DensifyConfig, reset_opacity, init_splats_from_points  # and of a set
                                                    # that grows and shrinks: rasterization(means2d_grad=True), gsplat's default
                                                    # densification rule as HIP plan / emit / gather kernels
    from gsbp_amd import MCMCConfig, relocate, sample_add, inject_noise  # or under a fixed budget: gsplat's MCMC strategy
                                                    # (train_scene(strategy=MCMCConfig(cap_max=...))), HIP plan / draw / update / move
    from gsbp_amd import SplatAdam                  # the optimiser step as one HIP kernel per table, optionally on the Gaussians a
                                                    # step's view saw alone (train_scene(adam="fused" | "visible", means_lr_final=...))
    from gsbp_amd import render_latents             # the second render of a Feature-3DGS step: a latent table of up to 128 channels,
                                                    # differentiable in the Gaussians and the table (train_scene(feature_fn=...))
    from gsbp_amd import depth_point_loss, depth_map_loss  # depth supervision: the render's expected depth against the view's
                                                    # triangulated points (scene_io.view_depth_points) or a depth map, a HIP kernel
                                                    # pair each (train_scene(depth_fn=...))
"""
from . import synthetic  # noqa: F401
from ._lib import GwbpError, build, lib  # noqa: F401
from .backproject import ViewPipeline, create_feature_field, create_label_field, create_mask_feature_field, create_vote_field, finalize_reference, mask3d_from_votes, prune_mask, reduce_partials, reduce_partials_sharded  # noqa: F401
from .engine import Engine, bilinear_index, narrow_labels, nearest_index  # noqa: F401
from . import scene_io  # noqa: F401
from .rasterization import rasterization  # noqa: F401
from .projection import project_torch, sh_colors_torch  # noqa: F401
from .sh import sh_colors  # noqa: F401
from .transfer import knn_search, transfer_labels, vote_labels  # noqa: F401
from .pca import PCABasis, fit_pca, pca_colors, pca_transform, render_pca  # noqa: F401
from .segment import ClickSession, apply_mask3d, probe_pixels, prompt_mask, prompt_scores, render_prompt_mask  # noqa: F401
from .label_render import miou_recall, recolor_by_labels, render_label_argmax, render_label_maps, score_label_views  # noqa: F401
from .fidelity import agreement_weights, field_fidelity, render_field_agreement, score_field_views  # noqa: F401
from .decoded_field import decode_field, decoded_field_gradients, decoded_loss, fit_decoded_field  # noqa: F401
from . import spatial  # noqa: F401
from .spatial import init_scales, knn_distances, plan_grid, remove_outliers, smooth_features, smooth_labels, smooth_mask, spatial_knn  # noqa: F401
from . import cluster  # noqa: F401
from .cluster import KMeans, class_prototypes, cluster_sums, codebook_prompt_mask, codebook_prompt_scores, dequantize_field, fit_kmeans, kmeans_assign, quantize_field, synthetic_clusters  # noqa: F401
from . import components  # noqa: F401
from .components import Components, Instances, radius_components, radius_count, select_components, split_instances, suggest_radius, synthetic_instances  # noqa: F401
from . import associate  # noqa: F401
from .associate import Association, associate_masks, associated_label_fn, match_masks, quantize_weights, remap_masks  # noqa: F401
from . import sparse_votes  # noqa: F401
from .associate import create_sparse_label_field  # noqa: F401
from .sparse_votes import SparseLabelField, SparseVotes, new_sparse_votes, sparse_label_argmax, sparse_label_dense, sparse_votes_bytes, sparse_votes_canonical, sparse_votes_dense, sparse_votes_groups, sparse_votes_stats  # noqa: F401
from . import regions  # noqa: F401
from .regions import edge_strength, neighbor_similarity, region_prompt_mask, similarity_components, similarity_levels, synthetic_regions  # noqa: F401
from . import sample  # noqa: F401
from .sample import PointGaussians, neighbor_blend, point_gaussians, sample_field, sample_labels, score_point_labels, suggest_sample_radius, synthetic_points, transfer_field, weighted_vote  # noqa: F401
from . import pixels  # noqa: F401
from .pixels import PixelGaussians, dominance_counts, lookup, median_depth, pick_gaussians, pixel_gaussians, render_id_map  # noqa: F401
from . import pose  # noqa: F401
from .pose import PoseAdjust, pose_error, refine_pose, se3_exp  # noqa: F401
from . import photometric  # noqa: F401
from .photometric import gaussian_window, image_metrics, image_sums, photometric_loss, ssim_map  # noqa: F401
from . import polish  # noqa: F401
from .polish import score_image_views  # noqa: F401
# (gsbp_amd.densify is the function, as gsbp_amd.rasterization is; the module is reached as `from gsbp_amd.densify import ...`)
from .densify import DensifyConfig, DensifyState, densify, init_splats_from_points, reset_opacity  # noqa: F401
from . import mcmc  # noqa: F401
from .mcmc import MCMCConfig, inject_noise, relocate, sample_add  # noqa: F401
from . import adam  # noqa: F401
from .adam import SplatAdam  # noqa: F401
from . import depth  # noqa: F401
from .depth import depth_map_loss, depth_point_loss, sample_expected_depth  # noqa: F401
from . import latent_render  # noqa: F401
from .latent_render import render_latents  # noqa: F401
from . import train  # noqa: F401
from .train import polish_scene, train_scene  # noqa: F401
from .pruning import check_proper_pruning, gradient_mask, prune_by_gradients  # noqa: F401
