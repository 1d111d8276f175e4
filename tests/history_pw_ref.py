"""The law of ultr_history_pw (include/ultr_hip.h) in numpy: per-click weights of a click model whose examination depends on where
the previous click of the same list was.

    last(b, l) = the largest l' < l with labels[l', b] > 0, or -1
    pw[b, l]   = (all_positions or labels[l, b] > 0) ? table[l, last(b, l) + 1] : 0

labels [L, B], table [L, L] (row = position, column = last click + 1), pw [B, L] in the table's dtype: a lookup, so the kernel has to
agree bit for bit."""
import numpy as np


def history_pw(labels_LB, table, all_positions):
    labels = np.asarray(labels_LB)
    L, B = labels.shape
    table = np.asarray(table)
    assert table.shape == (L, L)
    pw = np.zeros((B, L), table.dtype)
    for b in range(B):
        last = -1
        for l in range(L):
            click = bool(labels[l, b] > 0)
            if all_positions or click:
                pw[b, l] = table[l, last + 1]
            if click:
                last = l
    return pw


def position_pw(labels_LB, table, all_positions):
    """The table path (softmax_ce_kernel / prs_loss_kernel with ipw_table): pw[b, l] = (all or click) ? table[min(l, n - 1)] : 0."""
    labels = np.asarray(labels_LB)
    L, B = labels.shape
    table = np.asarray(table)
    col = table[np.minimum(np.arange(L), len(table) - 1)]
    pw = np.broadcast_to(col[None, :], (B, L)).astype(table.dtype).copy()
    if not all_positions:
        pw[~(labels.T > 0)] = 0
    return pw


def distinct_table(rng, L):
    """A random [L, L] float32 table of distinct values (not a click model's: a wrong column cannot coincide with the right value)."""
    t = (1.0 + rng.permutation(L * L).astype(np.float32) / 8.0).reshape(L, L)
    assert len(np.unique(t)) == L * L
    return t
