"""The restatement of the device online draw (tests/online_draw_ref.py) against the host online feeds, without a GPU: its
deterministic order is DeterministicOnlineSimulationFeed.rerank's, its label / cutoff handling and oracle mode are
OnlineSimulationFeed.simulate_clicks_online's, its race keys draw the Plackett-Luce distribution, and its Philox counters are
disjoint from those of the offline draws (tests/draw_ref.py) and match the kernel's source."""
import itertools
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import draw_ref as D
from tests import online_draw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_rerank(scores, n):
    from ultra_pytorch_amd.input_layer import DeterministicOnlineSimulationFeed
    return DeterministicOnlineSimulationFeed.rerank(object.__new__(DeterministicOnlineSimulationFeed), scores, n)


@pytest.mark.parametrize("n", [1, 2, 7, 50, 130, 256])
def test_deterministic_order_is_the_host_rerank(n):
    rng = np.random.RandomState(n)
    for trial in range(20):
        s = rng.randn(n).astype(np.float32)
        if trial % 2:
            s = (np.round(s * 2) / 2).astype(np.float32)  # many ties
        pads = rng.rand(n) < 0.2  # interior PADs: all the model's score of the zero row
        s[pads] = np.float32(0.125)
        if trial % 5 == 0:
            s[rng.rand(n) < 0.2] = np.float32(-0.0)
            s[rng.rand(n) < 0.2] = np.float32(0.0)
        got = R.rank_by_keys(R.order_key(s))
        assert list(got) == list(_host_rerank(s, n))


def test_order_key_places_nan_above_infinity():
    s = np.array([1.0, np.nan, np.inf, -np.inf, np.nan, -0.0, 0.0], np.float32)
    assert list(R.rank_by_keys(R.order_key(s))) == [1, 4, 2, 0, 5, 6, 3]


class _Model:
    def __init__(self, scores, M, cutoff):
        self._scores = scores
        self.letor_features_name = "letor_features"
        self.docid_inputs_name = ["docid_input%d" % l for l in range(M)]
        self.labels_name = ["label%d" % l for l in range(M)]
        self.max_candidate_num, self.rank_list_size = M, cutoff

    def validation(self, feed, is_online_simulation=False):
        return None, torch.from_numpy(self._scores), {}


def _host_feed(M, cutoff, oracle, scores, click_model=None):
    from ultra_pytorch_amd.input_layer import DeterministicOnlineSimulationFeed
    f = object.__new__(DeterministicOnlineSimulationFeed)
    f.model = _Model(scores, M, cutoff)
    f.max_candidate_num, f.rank_list_size = M, cutoff
    f.hparams = types.SimpleNamespace(oracle_mode=oracle)
    f.click_model = click_model
    return f


def _case(seed, B, M, n_docs=1000):
    """Candidates with ragged tails and interior PADs, graded labels, scores with ties."""
    rng = np.random.RandomState(seed)
    ids = rng.randint(0, n_docs, size=(M, B)).astype(np.int32)
    lens = rng.randint(0, M + 1, size=B)
    ids[np.arange(M)[:, None] >= lens[None, :]] = n_docs
    ids[rng.rand(M, B) < 0.15] = n_docs
    y = np.where(ids == n_docs, 0, rng.randint(0, 5, size=(M, B))).astype(np.float32)
    s = (np.round(rng.randn(B, M) * 3) / 3).astype(np.float32)
    s[(ids == n_docs).T] = np.float32(-0.25)
    return ids, y, s


def _host_run(feed, ids, y, n_docs, check_validation=True):
    M, B = ids.shape
    inp = {"letor_features": np.zeros((n_docs, 3), np.float32)}
    for l in range(M):
        inp["docid_input%d" % l] = ids[l].astype(np.float32).copy()
        inp["label%d" % l] = y[l].copy()
    out = feed.simulate_clicks_online(inp, check_validation=check_validation)
    return (np.stack([out["docid_input%d" % l] for l in range(M)]).astype(np.int64),
            np.stack([out["label%d" % l] for l in range(M)]).astype(np.float32))


@pytest.mark.parametrize("M,cutoff", [(10, 10), (10, 4), (40, 7), (256, 10)])
def test_oracle_mode_matches_the_host_feed(M, cutoff):
    n_docs, B = 1000, 24
    ids, y, s = _case(M + cutoff, B, M, n_docs)
    got_ids, got_y, perm, _ = R.rerank(ids, y, s, n_docs, 1, 2, R.DETERMINISTIC, 1, cutoff, 100, True, D.PBM,
                                       [1.0], 1, [1.0])
    want_ids, want_y = _host_run(_host_feed(M, cutoff, True, s), ids, y, n_docs)
    np.testing.assert_array_equal(got_ids, want_ids)
    np.testing.assert_array_equal(got_y, want_y)


class _Recorder:
    """A click model that records the label lists it is asked to click and clicks every position."""

    def __init__(self):
        self.lists = []

    def sampleClicksForOneList(self, labels):
        self.lists.append([float(v) for v in labels])
        return [1.0] * len(labels), None, None


@pytest.mark.parametrize("M,cutoff", [(10, 10), (10, 4), (40, 7), (130, 64)])
def test_clicked_labels_and_cutoff_match_the_host_feed(M, cutoff):
    n_docs, B = 1000, 24
    ids, y, s = _case(7 * M + cutoff, B, M, n_docs)
    rec = _Recorder()
    want_ids, want_y = _host_run(_host_feed(M, cutoff, False, s, rec), ids, y, n_docs, check_validation=False)  # one call per list
    exam = np.ones(M, np.float32)
    cprob = np.array([1.0], np.float32)  # every position clicked: the same click lists as the recorder's
    got_ids, got_y, perm, kept = R.rerank(ids, y, s, n_docs, 5, 9, R.DETERMINISTIC, 1, cutoff, 100, False, D.PBM, exam, M, cprob)
    np.testing.assert_array_equal(got_ids, want_ids)
    np.testing.assert_array_equal(got_y, want_y)
    lens = R.list_len(ids, n_docs)
    assert len(rec.lists) == B
    for b in range(B):
        cut = min(int(lens[b]), cutoff)
        assert rec.lists[b] == [float(v) for v in y[perm[:cut, b], b]]  # the labels the host clicked are the restatement's
        assert not got_y[cut:, b].any()


def test_redraws_only_the_clicks_and_keeps_an_empty_list():
    """Under check_validation only the clicks are redrawn, on the same order; 1 + 100 empty attempts keep the click-less list."""
    n_docs, M, B = 50, 8, 6
    ids = np.tile(np.arange(M, dtype=np.int32)[:, None], (1, B))
    y = np.zeros((M, B), np.float32)
    y[2, :3] = 1.0
    s = np.tile(np.linspace(1, 0, M, dtype=np.float32)[None, :], (B, 1))
    cprob = np.array([0.0, 0.05], np.float32)
    out_ids, out_y, perm, kept = R.rerank(ids, y, s, n_docs, 3, 4, R.DETERMINISTIC, 1, M, 100, False, D.PBM, np.ones(M, np.float32), M,
                                          cprob)
    assert (kept[3:] == 100).all() and not out_y[:, 3:].any()
    assert (out_y[:, :3].sum(0) <= 1).all() and (perm == np.arange(M)[:, None]).all()
    assert (kept[:3][out_y[:, :3].sum(0) > 0] < 100).all()


def test_pick_is_uniform_over_the_eligible_queries():
    eligible = np.array([3, 8, 9, 20], np.int64)
    q = R.pick(11, 0, 40000, 25, eligible)
    assert set(np.unique(q)) == set(eligible)
    counts = np.array([(q == e).sum() for e in eligible])
    assert np.abs(counts - 10000).max() < 5 * np.sqrt(10000 * 0.75)
    q_all = R.pick(11, 0, 40000, 25)
    assert set(np.unique(q_all)) == set(range(25))
    assert not np.array_equal(R.pick(11, 1, 64, 25), R.pick(11, 0, 64, 25))


def _pl_probability(w, order):
    p, rest = 1.0, float(np.sum(w))
    for i in order:
        p *= w[i] / rest
        rest -= w[i]
    return p


@pytest.mark.parametrize("tau", [1, 2])
def test_race_keys_draw_the_plackett_luce_distribution(tau):
    rng = np.random.RandomState(tau)
    s = np.array([0.3, -0.4, 0.9, 0.0], np.float32)
    n, draws = len(s), 40000
    counts = {}
    for _ in range(draws):
        order = tuple(R.stochastic_order(s, tau, rng.randint(0, 2 ** 24, size=n).astype(np.float32) * np.float32(2 ** -24))[0])
        counts[order] = counts.get(order, 0) + 1
    w = np.exp(tau * (s.astype(np.float64) - s.max()))
    chi2 = 0.0
    for perm in itertools.permutations(range(n)):
        e = draws * _pl_probability(w, perm)
        chi2 += (counts.get(perm, 0) - e) ** 2 / e
    df = 23
    assert chi2 < df + 6 * np.sqrt(2 * df), chi2  # p ~ 1e-5 for chi-square with 23 degrees of freedom


def test_underflowed_documents_follow_in_index_order():
    s = np.array([-500.0, 1.0, -400.0, 0.5, -300.0], np.float32)
    order, keys, zero, _ = R.stochastic_order(s, 1, np.full(5, 0.5, np.float32))
    assert list(zero) == [True, False, True, False, True]
    assert set(order[:2]) == {1, 3} and list(order[2:]) == [0, 2, 4]


def test_counters_are_disjoint_from_the_offline_draws_and_match_the_kernel():
    # the offline click draw uses words 3 = QUERY_TAG / CLICK_TAG, RegressionEM (b, l, REGEM_TAG, 1): a shared counter needs equal word 3
    offline = {D.QUERY_TAG, D.CLICK_TAG, 1}
    assert not offline & set(R.TAGS) and len(set(R.TAGS)) == 3
    src = open(os.path.join(ROOT, "ultra_pytorch_amd", "csrc", "ultr_online.hip")).read()
    tags = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define ONLINE_(\w+)_TAG (0x[0-9A-Fa-f]+)u", src)}
    assert tags == {"QUERY": R.QUERY_TAG, "RACE": R.RACE_TAG, "CLICK": R.CLICK_TAG}
    feed_src = open(os.path.join(ROOT, "ultra_pytorch_amd", "csrc", "ultr_feed.h")).read()
    for t in R.TAGS:
        assert ("0x%08X" % t) not in feed_src.upper()
