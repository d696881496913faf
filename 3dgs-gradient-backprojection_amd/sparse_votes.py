"""Per-Gaussian slot lists: the integer votes of the label lifts without a dense [N, K] table.

A Gaussian sees a handful of ids -- its own object's and those of the few masks whose borders cross its footprint -- so
gwbp_label_votes_sparse (Engine.label_votes_sparse) keeps S (key, integer sum) slots per Gaussian instead of a row of K columns:
N * (12 * S + 8) bytes (+ 8 * N with total), 104 MB at N = 1 M and S = 8, whatever the number of ids.

    sv = new_sparse_votes(n, slots=8, device=dev)
    eng.label_votes_sparse(view, labels, remap, sv, num_labels)      # per view, after blend_weights
    groups, certain = sparse_votes_groups(sv)

What the lists promise (the contract and the kernel: include/gwbp.h):
  1. a key is never evicted and never appears twice in a row; each slot holds the complete sum of its key over all calls so far;
  2. spill[g] is the complete sum of the keys that found no slot, and spill[g] > 0 exactly when row g has received more than S
     distinct keys: WHICH rows overflow is a function of the input alone;
  3. vals[g].sum() + spill[g] is the dense row's sum;
  4. a row without spill holds, as a set, exactly the non-zero entries of the dense row.  Only the slot order depends on the run;
     sparse_votes_canonical removes that;
  5. in an overflowed row, which S keys hold slots depends on the order of the run.  Such a row is never presented as exact:
     sparse_votes_groups says which rows are certain, sparse_votes_stats counts the others.

Everything here but the kernel call is plain torch on the [N, S] arrays: they are small and not the hot path.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch

from ._lib import SPARSE_MAX_SLOTS, GwbpError

EMPTY_KEY = -1


class SparseVotes(NamedTuple):
    keys: torch.Tensor             # int32 [N, S]: a slot's id, -1 = empty
    vals: torch.Tensor             # int64 [N, S]: the slot's fixed-point sum (vals / WEIGHT_SCALE is blend weight)
    spill: torch.Tensor            # int64 [N]: the sum of what found no slot
    total: Optional[torch.Tensor]  # int64 [N] or None: the sum of every non-zero entry, whatever its label


def sparse_votes_bytes(n: int, slots: int = 8, total: bool = False) -> int:
    """Bytes of new_sparse_votes(n, slots, total=total): n * (12 * slots + 8), + 8 * n with total."""
    return int(n) * (12 * int(slots) + 8 + (8 if total else 0))


def new_sparse_votes(n: int, slots: int = 8, device=None, total: bool = False) -> SparseVotes:
    """An empty accumulator of n rows and `slots` (1 .. 32) slots per row: keys -1, everything else 0."""
    n, slots = int(n), int(slots)
    if not 1 <= slots <= SPARSE_MAX_SLOTS:
        raise GwbpError(f"slots must lie in [1, {SPARSE_MAX_SLOTS}], got {slots}")
    if n < 0:
        raise GwbpError(f"n must not be negative, got {n}")
    return SparseVotes(torch.full((n, slots), EMPTY_KEY, dtype=torch.int32, device=device),
                       torch.zeros(n, slots, dtype=torch.int64, device=device), torch.zeros(n, dtype=torch.int64, device=device),
                       torch.zeros(n, dtype=torch.int64, device=device) if total else None)


def _check(sv) -> SparseVotes:
    keys, vals, spill, total = sv
    if (not torch.is_tensor(keys) or not torch.is_tensor(vals) or not torch.is_tensor(spill) or keys.dtype != torch.int32
            or vals.dtype != torch.int64 or spill.dtype != torch.int64 or keys.dim() != 2 or keys.shape != vals.shape
            or spill.shape != keys.shape[:1]):
        raise GwbpError("a SparseVotes holds keys int32 [N, S], vals int64 [N, S] and spill int64 [N]")
    if total is not None and (not torch.is_tensor(total) or total.dtype != torch.int64 or total.shape != spill.shape):
        raise GwbpError("total must be int64 [N] or None")
    return SparseVotes(keys, vals, spill, total)


def _sort_key(keys: torch.Tensor, vals: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(empties last, value descending, key ascending) as two stable sorts' worth of keys: the slot's rank value and its id."""
    k = keys.to(torch.int64)
    empty = k < 0
    return torch.where(empty, torch.iinfo(torch.int64).min, vals), torch.where(empty, torch.iinfo(torch.int64).max, k)


def sparse_votes_canonical(sv) -> SparseVotes:
    """The same lists in the canonical slot order: value descending, then key ascending, empties last (a new SparseVotes; spill
    and total are shared).  Two runs over the same input agree bit for bit in this form on every row without spill."""
    keys, vals, spill, total = _check(sv)
    rank, ident = _sort_key(keys, vals)
    by_key = torch.argsort(ident, dim=1, stable=True)
    by_val = torch.argsort(torch.gather(rank, 1, by_key), dim=1, descending=True, stable=True)
    order = torch.gather(by_key, 1, by_val)
    return SparseVotes(torch.gather(keys, 1, order), torch.gather(vals, 1, order), spill, total)


def sparse_votes_groups(sv) -> Tuple[torch.Tensor, torch.Tensor]:
    """(groups int32 [N], certain bool [N]).  groups: the key of the row's largest positive value, the smallest key among equals,
    -1 for a row without one -- on a row without spill this is group_of_votes of the dense table.  certain: spill == 0, or the
    best value exceeds the spill (no left-out key can have more than all of the spill), so the dense argmax is the same."""
    keys, vals, spill, _ = _check(sv)
    n = keys.shape[0]
    if keys.shape[1] == 0 or n == 0:
        return torch.full((n,), -1, dtype=torch.int32, device=keys.device), spill == 0
    k = keys.to(torch.int64)
    live = (k >= 0) & (vals > 0)
    v = torch.where(live, vals, 0)
    best = v.max(dim=1).values
    cand = torch.where(live & (v == best[:, None]), k, torch.iinfo(torch.int64).max)
    first = cand.min(dim=1).values
    groups = torch.where(best > 0, first, -1).to(torch.int32)
    return groups, (spill == 0) | (best > spill)


def sparse_votes_dense(sv, n_cols: int) -> torch.Tensor:
    """int64 [N, n_cols] with every slot's value in its key's column (the spill is in no column).  For tests and small cases:
    raises if a key is >= n_cols."""
    keys, vals, _, _ = _check(sv)
    n_cols = int(n_cols)
    k = keys.to(torch.int64)
    live = k >= 0
    if bool(live.any()) and int(k.max()) >= n_cols:
        raise GwbpError(f"the lists hold the key {int(k.max())}, which has no column among {n_cols}")
    out = torch.zeros(keys.shape[0], n_cols + 1, dtype=torch.int64, device=keys.device)  # (column n_cols takes the empties)
    out.scatter_add_(1, torch.where(live, k, n_cols), torch.where(live, vals, 0))
    return out[:, :n_cols].contiguous()


def sparse_votes_stats(sv) -> Dict:
    """{"rows", "slots", "overflow_rows" (spill > 0), "spilled_share" (spill / (vals + spill) over all rows), "slots_in_use"
    (histogram: entry i = rows with i slots taken), "uncertain_rows" (rows whose argmax the spill could change)}."""
    keys, vals, spill, _ = _check(sv)
    used = (keys >= 0).sum(dim=1)
    kept, lost = int(vals.sum()), int(spill.sum())
    _, certain = sparse_votes_groups(sv)
    return dict(rows=int(keys.shape[0]), slots=int(keys.shape[1]), overflow_rows=int((spill > 0).sum()),
                spilled_share=lost / (kept + lost) if kept + lost else 0.0,
                slots_in_use=torch.bincount(used, minlength=keys.shape[1] + 1).tolist(), uncertain_rows=int((~certain).sum()))


class SparseLabelField(NamedTuple):
    ids: torch.Tensor             # int32 [N, S]: class ids in canonical order (largest share first), -1 = empty
    fractions: torch.Tensor       # float32 [N, S]: the class's share of the Gaussian's whole weight (create_label_field's P)
    spill_fraction: torch.Tensor  # float32 [N]: the share of the classes that found no slot (0 on an exact row)
    total: torch.Tensor           # int64 [N]: the Gaussian's whole fixed-point weight over the views, the exact denominator


def sparse_label_field_of(sv) -> SparseLabelField:
    """The label field of an accumulator with total: canonical order, fractions = vals / total in float64, then narrowed."""
    keys, vals, spill, total = sparse_votes_canonical(sv)
    if total is None:
        raise GwbpError("a label field needs the lists' total (new_sparse_votes(..., total=True))")
    den = total.clamp(min=1).to(torch.float64)
    return SparseLabelField(keys, (vals.to(torch.float64) / den[:, None]).to(torch.float32),
                            (spill.to(torch.float64) / den).to(torch.float32), total)


def sparse_label_argmax(field: SparseLabelField) -> torch.Tensor:
    """int64 [N]: the class with the largest share (the smallest id among equals), -1 for a Gaussian no labelled pixel reached.
    Where spill_fraction exceeds the best share a left-out class may be larger: compare the two if the field can overflow."""
    if field.ids.shape[1] == 0:
        return torch.full((field.ids.shape[0],), -1, dtype=torch.int64, device=field.ids.device)
    ids, frac = field.ids[:, 0].to(torch.int64), field.fractions[:, 0]  # canonical: the first slot is the best
    return torch.where((ids >= 0) & (frac > 0), ids, -1)


def sparse_label_dense(field: SparseLabelField, num_classes: int) -> torch.Tensor:
    """float32 [N, num_classes]: create_label_field's P from the lists (for small num_classes; the spilled share is in no column)."""
    K = int(num_classes)
    ids = field.ids.to(torch.int64)
    live = ids >= 0
    if bool(live.any()) and int(ids.max()) >= K:
        raise GwbpError(f"the field holds the class {int(ids.max())}, which is not below num_classes = {K}")
    out = torch.zeros(ids.shape[0], K + 1, dtype=torch.float32, device=ids.device)
    out.scatter_add_(1, torch.where(live, ids, K), torch.where(live, field.fractions, 0.0))
    return out[:, :K].contiguous()
