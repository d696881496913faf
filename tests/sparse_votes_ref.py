"""TEST SUPPORT: a numpy reference of the per-Gaussian slot lists (gsbp_amd.sparse_votes, gwbp_label_votes_sparse), written from the
contract of include/gwbp.h with plain loops: the dense votes by associate_ref.add_votes first, then what the lists must hold for a
given number of slots S -- the canonical lists of the rows that fit, the spill, the overflow set."""
import numpy as np

import associate_ref as ref
from gsbp_amd.associate import quantize_weights


def dense_votes(pairs, labels, remap, n, n_cols, into=None):
    """int64 [n, n_cols]: associate_ref.add_votes of one view's (gid, pix, w) triples (added to `into` when given)."""
    V = np.zeros((n, n_cols), np.int64) if into is None else into
    return ref.add_votes(V, *pairs, labels, remap)


def totals(pairs, n):
    """int64 [n]: the sum of q over every entry of the Gaussian, whatever its label."""
    t = np.zeros(n, np.int64)
    np.add.at(t, pairs[0], quantize_weights(pairs[2]))
    return t


def distinct_keys(V):
    """int64 [n]: the number of non-zero columns of every row."""
    return (np.asarray(V) != 0).sum(axis=1)


def overflow_rows(V, S):
    """bool [n]: the rows that have received more than S distinct keys -- exactly the rows whose spill must be positive."""
    return distinct_keys(V) > S


def canonical_lists(V, S):
    """(keys int32 [n, S], vals int64 [n, S], exact bool [n]): every row's non-zero entries by value descending, then key ascending,
    -1 / 0 behind them.  For a row with more than S entries (exact = False) the lists hold the S first of that order, which is
    ONE of the states the contract allows, not the one a run must reach: compare such rows by the invariants only."""
    V = np.asarray(V)
    n = V.shape[0]
    keys, vals = np.full((n, S), -1, np.int32), np.zeros((n, S), np.int64)
    for g in range(n):
        cols = np.nonzero(V[g])[0]
        order = sorted(cols.tolist(), key=lambda c: (-int(V[g, c]), c))[:S]
        keys[g, :len(order)] = order
        vals[g, :len(order)] = V[g, order]
    return keys, vals, ~overflow_rows(V, S)


def check_invariants(keys, vals, spill, V, S):
    """Invariants 1 to 4 of the contract for lists (numpy: keys [n, S], vals [n, S], spill [n]) against the dense table V; returns
    the overflow set.  Raises AssertionError with the first offending row."""
    keys, vals, spill, V = (np.asarray(a) for a in (keys, vals, spill, V))
    n = V.shape[0]
    assert keys.shape == vals.shape == (n, S) and spill.shape == (n,)
    over = overflow_rows(V, S)
    # 2: the overflowed set is the input's, and the spill of every other row is zero
    assert np.array_equal(spill > 0, over), f"rows with spill {int((spill > 0).sum())}, rows with > {S} keys {int(over.sum())}"
    assert (spill >= 0).all()
    live = keys >= 0
    assert (keys >= -1).all() and (keys[live] < V.shape[1]).all()
    assert (vals[~live] == 0).all(), "an empty slot holds a value"
    # 1: each slot's value is the dense entry of its key (the complete sum), and no key twice in a row
    rows = np.broadcast_to(np.arange(n)[:, None], keys.shape)
    assert np.array_equal(vals[live], V[rows[live], keys[live]]), "a slot's value is not the dense entry of its key"
    assert (vals[live] > 0).all(), "a key was inserted for a zero sum"
    srt = np.sort(np.where(live, keys.astype(np.int64), -np.arange(1, S + 1)[None, :]), axis=1)  # (distinct stand-ins for empties)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "a key appears twice in a row"
    # empties only behind the taken slots: a lane takes the FIRST empty slot in index order
    assert (live[:, :-1] >= live[:, 1:]).all(), "an empty slot lies before a taken one"
    # an overflowed row is full
    assert live[over].all(), "an overflowed row has an empty slot"
    # 3: nothing is lost
    assert np.array_equal(vals.sum(axis=1) + spill, V.sum(axis=1)), "the lists and the spill do not add up to the dense row sum"
    # 4: rows without spill are exact as sets
    assert np.array_equal(live.sum(axis=1)[~over], distinct_keys(V)[~over]), "an exact row misses an entry"
    return over
