"""Label transfer onto a finished feature field by exact inner-product k-NN search (the reference's transfer_affordance,
affordance_transfer/demo_affordance_transfer.py:1377-1396: faiss.IndexFlatIP + np.bincount(...).argmax()).

    scores, indices = knn_search(features, sources, k)            # faiss.IndexFlatIP(D).search(features, k)
    labels = transfer_labels(features, sources, source_labels, k=5)

Both run gwbp_knn_search / gwbp_knn_vote (csrc/knn.hip) on the caller's current stream and allocate nothing but their outputs.
There is no PyTorch fallback: without the HIP library they raise.
"""
from __future__ import annotations

import ctypes as C
import pickle
from typing import Optional

import numpy as np
import torch

from ._lib import GwbpError, ptr
from ._views import field_rows, ld, rows, run

MAX_K = 32


def knn_search(features: torch.Tensor, sources: torch.Tensor, k: int):
    """faiss's IndexFlatIP.search on device tensors: for every row of features[N, D] the k rows of sources[M, D] of largest inner
    product.  Returns (scores[N, k] float32, indices[N, k] int32 -- not faiss's int64 -- on the device), each row sorted by score
    descending, then index ascending; NaN scores come last.  Exact fp32 (one fused multiply-add chain per score).

    features / sources may have any row stride >= D (a field still in padded storage, a column slice of a wider tensor) and are
    read in place; a tensor whose stride within a row is not 1 is copied with .contiguous().  float16 / bfloat16 FEATURES are read
    as stored and widened exactly in the kernel (the result has the bits of the search on features.float(), and no such copy is
    made); float16 / bfloat16 sources, the small operand, are converted with .float().  1 <= k <= 32, k <= M."""
    (q, ft), s = field_rows(features, "features"), rows(sources, "sources")
    if q.shape[1] != s.shape[1]:
        raise GwbpError(f"features have D = {q.shape[1]}, sources D = {s.shape[1]}")
    if q.device != s.device:
        raise GwbpError("features and sources must be on one device")
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise GwbpError(f"k must be in [1, {MAX_K}], got {k}")
    if k > s.shape[0]:
        raise GwbpError(f"k = {k} exceeds the number of sources M = {s.shape[0]}")
    n, m, d = q.shape[0], s.shape[0], q.shape[1]
    idx = torch.empty(n, k, dtype=torch.int32, device=q.device)
    score = torch.empty(n, k, dtype=torch.float32, device=q.device)
    run("gwbp_knn_search_typed", q.device, C.c_int64(n), m, d, k, ptr(q), ft, C.c_int64(ld(q)), ptr(s), C.c_int64(ld(s)), ptr(idx),
        ptr(score))
    return score, idx


def narrow_source_labels(labels, num_classes: Optional[int] = None):
    """The labels of the example tokens as the int32 [M] device-ready tensor gwbp_knn_vote reads, and the number of classes.
    labels: a tensor or array of M whole numbers, [M] or the reference's [M, 1] float array (load_labels).  Values that are not whole
    numbers are an error; with num_classes given, labels outside [0, num_classes) become -1 (ignored by the vote) BEFORE the
    narrowing, so that no wide value can wrap into range; without it num_classes = max label + 1 (negative labels ignored)."""
    t = torch.as_tensor(np.asarray(labels)) if not torch.is_tensor(labels) else labels
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 1:
        raise GwbpError(f"labels must be [M] or [M, 1], got {tuple(t.shape)}")
    if t.dtype == torch.bool:
        t = t.to(torch.int64)
    if t.is_floating_point():
        if not bool(torch.isfinite(t).all()) or not bool((t == t.round()).all()):
            raise GwbpError("labels must hold whole numbers")
        t = t.to(torch.float64).clamp(-1.0, float(2 ** 62)).to(torch.int64)
    t = t.to(torch.int64)
    if num_classes is None:
        num_classes = int(t.max()) + 1 if t.numel() and int(t.max()) >= 0 else 1
    num_classes = int(num_classes)
    if not 1 <= num_classes < 2 ** 31:
        raise GwbpError(f"num_classes must be in [1, 2^31), got {num_classes}")
    t = torch.where((t < 0) | (t >= num_classes), torch.full_like(t, -1), t).to(torch.int32)
    return t, num_classes


def vote_labels(indices: torch.Tensor, labels: torch.Tensor, num_classes: int, return_counts: bool = False):
    """The majority label of each row of knn_search's indices[N, k]: np.bincount(labels[row]).argmax() (the smallest of equally
    frequent labels), int32 [N]; -1 for a row whose neighbours all carry ignored labels.  labels: int32 [M] on the device
    (narrow_source_labels).  With return_counts also counts[N, num_classes] int32, each row's histogram."""
    if not indices.is_cuda or indices.dtype != torch.int32 or indices.dim() != 2:
        raise GwbpError("indices must be knn_search's int32 [N, k] device tensor")
    if labels.dtype != torch.int32 or labels.dim() != 1 or labels.device != indices.device:
        raise GwbpError("labels must be an int32 [M] tensor on the device of indices")
    indices, labels = indices.contiguous(), labels.contiguous()
    n, k = indices.shape
    out = torch.empty(n, dtype=torch.int32, device=indices.device)
    counts = torch.empty(n, num_classes, dtype=torch.int32, device=indices.device) if return_counts else None
    run("gwbp_knn_vote", indices.device, C.c_int64(n), int(labels.shape[0]), k, ptr(indices), ptr(labels), int(num_classes),
         ptr(out), ptr(counts), C.c_int64(num_classes))
    return (out, counts) if return_counts else out


def transfer_labels(features: torch.Tensor, sources: torch.Tensor, labels, k: int = 5, num_classes: Optional[int] = None,
                    return_counts: bool = False):
    """The reference's transfer_affordance from its two arrays: every row of features[N, D] gets the most frequent label among its
    k nearest (largest inner product) rows of sources[M, D], ties to the smallest label.  Returns labels[N] int32 (with
    return_counts also counts[N, num_classes] int32).  features, sources, k: as knn_search.  labels: [M] or [M, 1], integer or
    whole-valued float (narrow_source_labels); num_classes defaults to max label + 1."""
    s = rows(sources, "sources")
    lab, nc = narrow_source_labels(labels, num_classes)
    if lab.shape[0] != s.shape[0]:
        raise GwbpError(f"{lab.shape[0]} labels for {s.shape[0]} sources")
    _, idx = knn_search(features, s, k)
    return vote_labels(idx, lab.to(idx.device), nc, return_counts)


# ---- example sets (the CLI's --examples / --synthetic) ---------------------------------------------------------------------------

def load_examples(path: str):
    """(features[M, D] float32, labels[M] or [M, 1]) from a .pt (dict with "features" and "labels"), an .npz with the same two
    arrays, or the reference's features_and_labels.pkl (a pickled dict of numpy arrays; only open pickles you trust)."""
    low = path.lower()
    if low.endswith(".npz"):
        with np.load(path) as z:
            data = {key: z[key] for key in z.files}
    elif low.endswith(".pkl"):
        with open(path, "rb") as f:
            data = pickle.load(f)
    else:
        data = torch.load(path, map_location="cpu")
    if not isinstance(data, dict) or "features" not in data or "labels" not in data:
        raise GwbpError(f"{path}: expected a dict with 'features' and 'labels'")
    feats = torch.as_tensor(np.asarray(data["features"])) if not torch.is_tensor(data["features"]) else data["features"]
    labels = torch.as_tensor(np.asarray(data["labels"])) if not torch.is_tensor(data["labels"]) else data["labels"]
    if feats.dim() != 2 or labels.shape[0] != feats.shape[0]:
        raise GwbpError(f"{path}: features {tuple(feats.shape)} and labels {tuple(labels.shape)} do not match")
    return feats.float(), labels


def synthetic_transfer(n: int = 4096, m: int = 512, d: int = 64, num_classes: int = 4, seed: int = 0):
    """A seeded field and example set for tests and the CLI's --synthetic: unit-norm Gaussian sources with random labels, and
    queries that are unit-normalised noisy copies of random sources.  Returns CPU tensors (features[n, d], sources[m, d],
    labels[m] int64)."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(m, d, generator=g)
    src = src / src.norm(dim=1, keepdim=True)
    pick = torch.randint(0, m, (n,), generator=g)
    q = src[pick] + 0.5 * torch.randn(n, d, generator=g) / d ** 0.5
    q = q / q.norm(dim=1, keepdim=True)
    labels = torch.randint(0, num_classes, (m,), generator=g)
    return q, src, labels
