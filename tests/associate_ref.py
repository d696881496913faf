"""TEST SUPPORT: a numpy reference of the mask association (gsbp_amd.associate), written with plain loops and np.add.at from the
issue's rules and independently of match_masks: per-view (gid, pix, w) triples of the blend (pix = y * W + x, as the oracle's
blend_pairs and Engine.dump_pairs give them) and the views' label maps in, maps / groups / votes / n_groups out."""
import numpy as np

from gsbp_amd.associate import WEIGHT_SCALE, quantize_weights


def overlap_table(gid, pix, w, labels, num_labels, group, n_cols):
    """int64 [num_labels + 1, n_cols]: row = label if in range else num_labels, column = group + 1 if -1 <= group <= n_cols - 2
    else 0.  labels: [H, W] at the view's resolution."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)[pix]
    row = np.where((lab >= 0) & (lab < num_labels), lab, num_labels)
    g = np.asarray(group).astype(np.int64)[gid]
    col = np.where((g >= -1) & (g <= n_cols - 2), g + 1, 0)
    O = np.zeros((num_labels + 1, n_cols), np.int64)
    np.add.at(O, (row, col), quantize_weights(w))
    return O


def add_votes(V, gid, pix, w, labels, remap):
    """V[g, remap[label]] += q in place; labels outside [0, len(remap)) and remap entries outside [0, V.shape[1]) add nothing."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)[pix]
    ok = (lab >= 0) & (lab < len(remap))
    col = np.where(ok, np.asarray(remap).astype(np.int64)[np.where(ok, lab, 0)], -1)
    ok = (col >= 0) & (col < V.shape[1])
    np.add.at(V, (gid[ok], col[ok]), quantize_weights(w)[ok])
    return V


def match_ref(O, n_groups, iou_min=0.2, min_mass=1.0, max_groups=256):
    """(remap int32 [K], n_groups, dropped): the best remaining (mask, group) pair is picked again and again -- largest IoU, then
    smallest mask, then smallest group -- until none reaches iou_min; then the unmatched live masks open groups."""
    K = O.shape[0] - 1
    need = int(np.rint(min_mass * WEIGHT_SCALE))
    A = [int(sum(int(x) for x in O[m])) for m in range(K)]
    B = [int(sum(int(O[r, j + 1]) for r in range(K + 1))) for j in range(n_groups)]
    live = [A[m] >= need for m in range(K)]
    remap = np.full(K, -1, np.int32)
    free_m, free_j = set(m for m in range(K) if live[m]), set(range(n_groups))
    while True:
        best = None
        for m in sorted(free_m):
            for j in sorted(free_j):
                o = int(O[m, j + 1])
                if o <= 0:
                    continue
                iou = float(o) / float(A[m] + B[j] - o)
                if iou >= iou_min and (best is None or iou > best[0]):  # (ascending m, j: the first of equals stays)
                    best = (iou, m, j)
        if best is None:
            break
        remap[best[1]] = best[2]
        free_m.discard(best[1])
        free_j.discard(best[2])
    dropped = 0
    for m in sorted(free_m):
        if n_groups < max_groups:
            remap[m] = n_groups
            n_groups += 1
        else:
            dropped += 1
    return remap, n_groups, dropped


def groups_of(V):
    best = V.max(axis=1)
    return np.where(best > 0, V.argmax(axis=1), -1).astype(np.int32)  # (np.argmax: the first of equals)


def associate_ref(pairs, maps, n, max_masks, max_groups=256, iou_min=0.2, min_mass=1.0, order=None):
    """pairs[v] = (gid, pix, w) and maps[v] = [H, W] integer map of view v.  Returns dict(maps, groups, votes, n_groups, dropped)."""
    order = list(range(len(maps))) if order is None else list(order)
    V = np.zeros((n, max_groups), np.int64)
    group = np.full(n, -1, np.int32)
    out_maps = [np.full(max_masks, -1, np.int32) for _ in maps]
    n_groups, dropped = 0, []
    for v in order:
        gid, pix, w = pairs[v]
        O = overlap_table(gid, pix, w, maps[v], max_masks, group, max_groups + 1)
        remap, n_groups, drop = match_ref(O, n_groups, iou_min, min_mass, max_groups)
        out_maps[v] = remap
        dropped.append(drop)
        add_votes(V, gid, pix, w, maps[v], remap)
        group = groups_of(V)
    return dict(maps=out_maps, groups=group, votes=V, n_groups=n_groups, dropped=dropped)


def purity(groups, instance):
    """(share of the grouped Gaussians that lie in a group whose majority instance is their own, smallest majority share of a
    non-empty group, number of non-empty groups)."""
    groups, instance = np.asarray(groups), np.asarray(instance)
    right, worst, n_groups = 0, 1.0, 0
    for j in np.unique(groups[groups >= 0]):
        inst = instance[groups == j]
        top = int(np.bincount(inst).max())
        right += top
        worst = min(worst, top / len(inst))
        n_groups += 1
    return right / max(1, int((groups >= 0).sum())), worst, n_groups


def clear_maximum(votes, n_entries):
    """bool [N]: rows whose largest vote beats the second by more than the float label kernel can blur.  F * 2^20 lies within
    n_entries / 2 (every entry rounds by at most half a step) + 1e-5 * F * 2^20 (the float kernel's tolerance) of the votes in
    every column, so the two argmaxes agree where top - second > n_entries + 2e-5 * top."""
    part = np.sort(np.asarray(votes), axis=1)[:, -2:] if votes.shape[1] > 1 else np.concatenate([np.zeros_like(votes), votes], 1)
    top, second = part[:, 1].astype(np.float64), part[:, 0].astype(np.float64)
    return (top > 0) & (top - second > np.asarray(n_entries, np.float64) + 2e-5 * top)


def oracle_instance_views(orc, cfg, viewmats, n_instances=4, seed=None, n_ids=None):
    """The fixture of the end-to-end tests on the CPU oracle: (instance [N], maps per view as numpy int32 [H, W], pairs per view)
    of synthetic.make_instance_views with the oracle's render of the one-hot instance table as its argmax, and the oracle's
    blend_pairs of every view."""
    import torch

    from gsbp_amd import synthetic as syn
    means, quats, scales, opac = (t.numpy() for t in syn.activate(syn.make_scene(cfg)))
    K, W, H = syn.intrinsics(cfg).numpy(), cfg.width, cfg.height
    front = {}

    def blended(v):
        if v not in front:
            proj = orc.project(means, quats, scales, viewmats[v].numpy(), K, W, H)
            front[v] = (proj, orc.bin_sort(proj, W, H))
        return front[v]

    def argmax_fn(v, instance):
        proj, bins = blended(v)
        onehot = np.eye(n_instances, dtype=np.float32)[instance.numpy()]
        img, alphas = orc.render(proj, bins, opac, onehot, W, H)
        seg = np.where(img.max(axis=-1) > 0, img.argmax(axis=-1), -1)
        return torch.from_numpy(seg), torch.from_numpy(alphas)

    kw = {} if seed is None else dict(seed=seed)
    instance, maps, _ = syn.make_instance_views(cfg, viewmats, n_instances, n_ids=n_ids, argmax_fn=argmax_fn, **kw)
    pairs = []
    for v in range(viewmats.shape[0]):
        proj, bins = blended(v)
        pairs.append(orc.blend_pairs(proj, bins, opac, W, H)[:3])
    return instance.numpy(), [m.numpy() for m in maps], pairs
