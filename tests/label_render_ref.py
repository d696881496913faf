"""numpy reference of the label render (gsbp_amd.label_render) on the CPU oracle as it is, and the seeded cases of its tests.

    maps, alphas = oracle.render(one-hot [N, K] table)        the class opacities the kernel must reproduce within 1e-4
    predicted    = uint8(clip(maps, 0, 1) * 255) > cut          torch_to_cv(...) > 64 of the reference, literally
    counts[k]    = {|predicted & gt == k|, |predicted|, |gt == k|}
    reference_loop(...)                                         evaluate_results' loop and bookkeeping, line by line

A (pixel, class) case is UNDECIDED when the oracle's value lies within TOL = 1e-4 (the project's tolerance for sums against the
oracle) of the threshold (cut + 1) / 255: there a render within the tolerance may fall on either side.
"""
import functools
from collections import defaultdict

import numpy as np
import torch

from gsbp_amd import synthetic as syn
from oracle import oracle as orc

TOL = 1e-4
CUT = 64
CLASS_COUNTS = (1, 2, 8, 33, 64, 65, 150)
W, H = 70, 45  # no multiple of 16: 5 x 3 tiles, the last column 6 pixels wide, the last row 13 high
# dense: tiles with more than 256 records (the staging batch); sparse: tiles with none
SCENES = {"dense": syn.Config("LR-dense", 2000, 3, W, H, 8, 0.08, False), "sparse": syn.Config("LR-sparse", 30, 3, W, H, 8, 0.04, False)}
CASES = [(kind, k) for kind in SCENES for k in CLASS_COUNTS]
CASE_IDS = [f"{kind}-K{k}" for kind, k in CASES]
SCORE_CASE = ("sparse", 8)  # score_label_views / miou_recall end to end: NO undecided case in its views (test_label_render_cpu)
SCENE_SEED = {"dense": 11, "sparse": 10}  # sparse: chosen on the oracle for SCORE_CASE (seeds 1, 4, 9, 12 leave an undecided case)


@functools.lru_cache(maxsize=None)
def scene(kind):
    """Host tensors of the scene: (means, quats, scales, opac), viewmats [3, 4, 4], K [3, 3]."""
    cfg = SCENES[kind]
    gauss = tuple(t.contiguous() for t in syn.activate(syn.make_scene(cfg, seed=SCENE_SEED[kind])))
    return gauss, syn.make_cameras(cfg), syn.intrinsics(cfg)


def labels_of(kind, k):
    """int32 [N] in [-1, k + 1]: -1 and values >= k belong to no class."""
    n = SCENES[kind].n_gaussians
    lab = np.random.default_rng(100 * k + n).integers(-1, k + 2, n).astype(np.int32)
    lab[:3] = (-1, k, k + 1)
    return lab


def gt_of(kind, k, view):
    """int32 [H, W]: 5 x 5 blocks of one random id in [-2, k + 1] (out-of-range values match no class)."""
    rng = np.random.default_rng(1000 * k + 10 * view + len(kind))
    blocks = rng.integers(-2, k + 2, (-(-H // 5), -(-W // 5)))
    blocks[0, :3] = (-2, k, k + 1)
    return np.repeat(np.repeat(blocks, 5, axis=0), 5, axis=1)[:H, :W].astype(np.int32)


def one_hot(labels, k):
    t = np.zeros((labels.shape[0], k), np.float32)
    ok = (labels >= 0) & (labels < k)
    t[np.nonzero(ok)[0], labels[ok]] = 1.0
    return t


@functools.lru_cache(maxsize=None)
def front(kind, view):
    (means, quats, scales, opac), vms, K = scene(kind)
    proj = orc.project(means.numpy(), quats.numpy(), scales.numpy(), vms[view].numpy(), K.numpy(), W, H)
    return proj, orc.bin_sort(proj, W, H)


@functools.lru_cache(maxsize=None)
def oracle_maps(kind, k, view=0):
    """(maps [H, W, k], alphas [H, W]) of the oracle's render of the one-hot table.  Shared: do not write into them."""
    proj, bins = front(kind, view)
    maps, alphas = orc.render(proj, bins, scene(kind)[0][3].numpy(), one_hot(labels_of(kind, k), k), W, H)
    maps.setflags(write=False)
    alphas.setflags(write=False)
    return maps, alphas


def predicted(maps, cut=CUT):
    """torch_to_cv(maps) > cut: clamp to [0, 1], one float32 multiply by 255, truncation to uint8."""
    return (np.clip(np.asarray(maps, np.float32), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8) > cut


def counts_of(maps, gt, cut=CUT):
    """int64 [K, 3]: intersection, predicted, ground truth."""
    k = maps.shape[-1]
    pred = predicted(maps, cut)
    truth = gt[..., None] == np.arange(k)
    return np.stack([(pred & truth).sum(axis=(0, 1)), pred.sum(axis=(0, 1)), truth.sum(axis=(0, 1))], axis=1).astype(np.int64)


def undecided(maps, cut=CUT):
    """bool [H, W, K]."""
    return np.abs(np.asarray(maps, np.float64) - (cut + 1) / 255.0) <= TOL


def reference_loop(maps_of_view, gt_of_view, classes, n_present, cut=CUT):
    """evaluate_results (demo_affordance_transfer.py:1536-1611) on rendered class maps: maps_of_view[v] is [H, W, K] (the
    reference renders channel i as a 3-channel image and keeps channel 0), gt_of_view[v] the label map or None for a skipped view.
    Returns (mIoU, recall)."""
    mIoU, recall = defaultdict(list), defaultdict(list)
    for maps, gt_label in zip(maps_of_view, gt_of_view):
        if gt_label is None:
            continue
        for i in classes:
            output_cv = (np.clip(maps[..., i], 0.0, 1.0).astype(np.float32) * np.float32(255.0)).astype(np.uint8)
            gt_mask = gt_label == i
            affordance_mask = output_cv > cut
            intersection = np.logical_and(gt_mask, affordance_mask).sum()
            union = np.logical_or(gt_mask, affordance_mask).sum()
            if union == 0:
                continue
            if intersection == 0:
                iou = 0
            else:
                iou = intersection / union
            mIoU[i].append(iou)
            if gt_mask.sum() == 0:
                continue
            if intersection == 0:
                rec = 0
            else:
                rec = intersection / gt_mask.sum()
            recall[i].append(rec)
    res = 0
    for i in classes:
        if len(mIoU[i]) == 0:
            continue
        res += np.mean(mIoU[i])
    res /= n_present
    res_recall = 0
    for i in classes:
        if len(recall[i]) == 0:
            continue
        res_recall += np.mean(recall[i])
    res_recall /= n_present
    return float(res), float(res_recall)


def bookkeeping_of_counts(counts, classes, n_present):
    """The same bookkeeping on counts [V, K, 3] (union = predicted + ground truth - intersection), restated line by line."""
    mIoU, recall = defaultdict(list), defaultdict(list)
    for row in np.asarray(counts):
        for i in classes:
            intersection, pred, truth = (int(x) for x in row[i])
            union = pred + truth - intersection
            if union == 0:
                continue
            mIoU[i].append(0 if intersection == 0 else intersection / union)
            if truth == 0:
                continue
            recall[i].append(0 if intersection == 0 else intersection / truth)
    res = sum(np.mean(mIoU[i]) for i in classes if len(mIoU[i])) / n_present
    res_recall = sum(np.mean(recall[i]) for i in classes if len(recall[i])) / n_present
    return float(res), float(res_recall)


def device_scene(kind, dev):
    gauss, vms, K = scene(kind)
    return tuple(t.to(dev) for t in gauss), vms.to(dev), K.to(dev)


def device_labels(kind, k, dev):
    return torch.from_numpy(labels_of(kind, k)).to(dev)
