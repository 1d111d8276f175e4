"""The float64 NDCG restatement of tests/ndcg_ref.py (what the GPU metric tests hold ultr_ndcg to) against the oracle's metric
(oracle/ultr_oracle.py: ndcg, argsort_desc - metrics.py with weights = None) on inputs where the two must agree: no ties, and rows
with NaN scores (where only the key sequence of the order and the value are defined by the oracle)."""
import numpy as np
import pytest
import torch

from oracle import ultr_oracle as O
from tests import ndcg_ref as N


def _inputs(seed, B, L, invalid=0.1):
    rng = np.random.RandomState(seed)
    s = rng.normal(size=(B, L)).astype(np.float32)  # continuous: no ties
    y = rng.randint(0, 5, size=(B, L)).astype(np.float32)
    y[rng.rand(B, L) < 0.2] += 0.5  # fractional labels
    y[rng.rand(B, L) < invalid] = -1.0
    return s, y


@pytest.mark.parametrize("B,L,topn", [(7, 1, [1, 3]), (16, 10, [1, 3, 5, 10]), (9, 65, list(range(1, 17))), (3, 130, [10, 3, 1000, 3])])
def test_restatement_is_the_oracle_without_ties(B, L, topn):
    # invalid labels all take the row minimum - 1e-6: ties, but between label-0 documents - the values are defined, the order is not
    for invalid in (0.0, 0.1):
        s, y = _inputs(B * 1000 + L, B, L, invalid)
        per, order, prep = N.ndcg_per_list(s, y, topn)
        st, yt = torch.from_numpy(s), torch.from_numpy(y)
        np.testing.assert_allclose(per.mean(0), O.ndcg(yt, st, topn).numpy(), rtol=0, atol=2e-6)
        for b in range(B):
            np.testing.assert_allclose(per[b], O.ndcg(yt[b:b + 1], st[b:b + 1], topn).numpy(), rtol=0, atol=2e-6)
        if invalid == 0.0:
            assert all(len(set(r.tolist())) == L for r in prep)  # no ties: the order is defined
            np.testing.assert_array_equal(order, O.argsort_desc(yt, st).numpy())


def test_restatement_edges():
    """Cutoffs clipped to L, 0 when the ideal DCG is 0 (all labels 0 or invalid), PAD masking, ties kept in index order."""
    s = np.array([[0.5, 0.5, 0.5, 0.25], [1.0, 2.0, 3.0, 4.0], [3.0, 2.0, 1.0, 0.0]], np.float32)
    y = np.array([[0, 4, 0, 1], [-1, -1, -1, -1], [0, 0, 0, 0]], np.float32)
    per, order, prep = N.ndcg_per_list(s, y, [1, 2, 1000])
    np.testing.assert_array_equal(order[0], [0, 1, 2, 3])
    g = 2.0 ** np.array([0, 4, 0, 1]) - 1
    disc = 1 / np.log2(np.arange(4) + 2.0)
    ideal = np.sort(g)[::-1]
    np.testing.assert_allclose(per[0], [0.0, g[1] * disc[1] / (ideal[:2] @ disc[:2]), (g @ disc) / (ideal @ disc)], rtol=1e-12)
    np.testing.assert_array_equal(per[1:], 0.0)
    np.testing.assert_array_equal(prep[1], np.float32(-1e-6) + np.float32(1.0))
    m = N.masked_scores(s, np.array([[0, 9, 0], [9, 1, 1], [2, 2, 2], [3, 3, 9]]), 9)
    assert m[1, 0] == m[0, 1] == m[2, 3] == N.PAD_SCORE and m[0, 0] == 0.5


@pytest.mark.parametrize("invalid", [False, True])
def test_restatement_orders_nan_like_the_oracle(invalid):
    """A NaN score sorts above every number in torch's descending sort, and torch.min carries it into the row minimum that invalid
    labels take: the restatement's order has the oracle's key sequence and its NDCG is the oracle's."""
    rng = np.random.RandomState(5 + invalid)
    B, L = 6, 12
    s = rng.normal(size=(B, L)).astype(np.float32)
    y = rng.randint(0, 5, size=(B, L)).astype(np.float32)
    for b in range(B):
        nan_at = rng.choice(L, size=1 + b % 2, replace=False)
        s[b, nan_at] = np.nan
        if b % 2 == 0:
            y[b, nan_at] = 0.0  # one label among the NaN positions (with the invalid ones): the value does not depend on their order
        if invalid:
            y[b, rng.choice(L, size=2, replace=False)] = -1.0
    topn = [1, 3, 5, 10]
    per, order, prep = N.ndcg_per_list(s, y, topn)
    st, yt = torch.from_numpy(s), torch.from_numpy(y)
    o_order = O.argsort_desc(yt, st).numpy()
    compared = 0
    for b in range(B):
        keys = np.take(prep[b], order[b])
        o_prep = O._prepare(yt[b:b + 1], st[b:b + 1], [1])[1][0].numpy()
        np.testing.assert_array_equal(prep[b], o_prep)  # NaN propagated to the invalid positions exactly as the oracle does
        np.testing.assert_array_equal(keys, np.take(o_prep, o_order[b]))
        n_nan = int(np.isnan(prep[b]).sum())
        assert np.isnan(keys[:n_nan]).all() and not np.isnan(keys[n_nan:]).any()
        assert sorted(order[b].tolist()) == list(range(L))
        if len(set(np.maximum(y[b], 0)[np.isnan(prep[b])].tolist())) == 1:  # the oracle's order among NaNs is unspecified: compare
            np.testing.assert_allclose(per[b], O.ndcg(yt[b:b + 1], st[b:b + 1], topn).numpy(), rtol=0, atol=2e-6)  # where it is moot
            compared += 1
    assert compared >= 3
