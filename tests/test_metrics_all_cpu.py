"""The float64 restatement of tests/metrics_ref.py (what the GPU tests hold ultr_metrics_report to) against the oracle's metrics
(oracle/ultr_oracle.py - metrics.py with weights = None) on inputs without ties between documents of different labels, and against the
reference's own recorded values (tests/golden/metrics_host.npz); the C header's declarations of the launch."""
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import ultr_oracle as O
from tests import metrics_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(seed, B, L, invalid=0.1):
    rng = np.random.RandomState(seed)
    s = rng.normal(size=(B, L)).astype(np.float32)  # continuous: no ties
    y = rng.randint(0, 5, size=(B, L)).astype(np.float32)
    y[rng.rand(B, L) < 0.2] += 0.5  # fractional labels
    y[rng.rand(B, L) < invalid] = -1.0
    if B >= 3:
        y[1] = np.where(y[1] >= 1, 0.0, y[1])  # a list without a relevant document
    return s, y


def _oracle(y, s, topn, max_label):
    yt, st = torch.from_numpy(y), torch.from_numpy(s)
    return {"ndcg": O.ndcg(yt, st, topn), "mrr": O.mrr(yt, st, topn), "err": O.err(yt, st, topn, max_label),
            "map": O.mean_average_precision(yt, st, topn), "arp": O.average_relevance_position(yt, st, topn),
            "ordered_pair_accuracy": O.ordered_pair_accuracy(yt, st, topn),
            "precision": O.precision_whole_list(yt, st).repeat(len(topn))}


@pytest.mark.parametrize("B,L,topn", [(7, 1, [1, 3]), (16, 10, [1, 3, 5, 10]), (9, 15, [10, 3, 1000, 3]), (9, 65, list(range(1, 17))), (3, 130, [10, 3, 1000, 3])])
def test_restatement_is_the_oracle_without_ties(B, L, topn):
    # (invalid labels all take the row minimum - 1e-6: ties, but between label-0 documents - every value is defined)
    for invalid in (0.0, 0.1):
        s, y = _inputs(B * 1000 + L, B, L, invalid)
        per, _ = M.per_list(s, y, topn, max_label=5.0)  # fractional labels up to 4.5 keep rel < 1
        means = M.batch_means(per)
        for name, ref in _oracle(y, s, topn, 5.0).items():
            if name == "arp" and L > 16:
                # the oracle is float32 and a list's ARP reaches L: above 16 its own rounding (half an ulp, 1e-6 at 16) is past
                # the bar, so the long lists pin the seven bounded metrics and the short ones ARP as well
                continue
            np.testing.assert_allclose(means[name], np.asarray(ref, dtype=np.float64).reshape(-1), rtol=0, atol=2e-6, err_msg=name)
        for k, n in enumerate(topn):  # dcg: the oracle's own helper (the reference's dcg entry raises, utils/metrics.py)
            yt, st = O._prepare(torch.from_numpy(y), torch.from_numpy(s), [n])[:2]
            ref = O._dcg(st, yt, [min(n, L)]).numpy()[:, 0].astype(np.float64)
            np.testing.assert_allclose(per["dcg"][:, k], ref, rtol=2e-6, atol=2e-6)


def test_restatement_is_the_reference_on_its_recorded_cases():
    d = np.load(os.path.join(ROOT, "tests", "golden", "metrics_host.npz"))
    meta = json.loads(str(d["meta"]))
    for tag in ("a", "b"):
        per, _ = M.per_list(d[tag + "_scores"], d[tag + "_labels"], meta["topn"], max_label=meta["max_label"])
        means = M.batch_means(per)
        for key in meta["keys"]:
            ref = d["%s_%s" % (tag, key)]
            np.testing.assert_allclose(means[key], np.broadcast_to(ref, means[key].shape), rtol=0, atol=1e-6, err_msg=tag + " " + key)


def test_restatement_edges():
    """A tie keeps index order, an invalid label is no partner of a pair, a list without a relevant document scores 0."""
    s = np.array([[0.5, 0.5, 0.25, 0.75], [3.0, 2.0, 1.0, 0.0]], np.float32)
    y = np.array([[0, 2, 1, -1], [0, 0, 0.5, 0]], np.float32)
    per, order = M.per_list(s, y, [1, 2, 9], max_label=2.0)
    np.testing.assert_array_equal(order[0], [0, 1, 2, 3])  # the invalid document: 0.25 - 1e-6, last
    assert per["mrr"][0, 0] == 0.5 and per["precision"][0, 0] == 0.5
    np.testing.assert_allclose(per["map"][0], (1 / 2 + 2 / 3) / 2)
    np.testing.assert_allclose(per["arp"][0], (2 * 2 + 3 * 1) / 3.0)
    np.testing.assert_allclose(per["ordered_pair_accuracy"][0], 1 / 16.0)  # (1, 2) only: (1, 0) ties, the 0.75 is invalid
    np.testing.assert_allclose(per["err"][0], [0.0, 0.75 / 2, 0.75 / 2 + 0.25 * 0.25 / 3])
    np.testing.assert_allclose(per["dcg"][0], [0.0, 3 / np.log2(3), 3 / np.log2(3) + 1 / 2.0])
    for name in ("mrr", "map", "precision"):
        np.testing.assert_array_equal(per[name][1], 0.0)  # label 0.5 is not relevant (>= 1 is)
    np.testing.assert_allclose(per["arp"][1], 3.0)


def test_header_declares_the_metric_launch():
    h = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", h).group(1)) == 8
    ids = {"NDCG": 0, "DCG": 1, "MRR": 2, "ERR": 3, "MAP": 4, "ARP": 5, "PRECISION": 6, "OPA": 7}
    for name, v in ids.items():
        assert int(re.search(r"#define\s+ULTR_METRIC_%s\s+(\d+)" % name, h).group(1)) == v
    assert int(re.search(r"#define\s+ULTR_MAX_METRICS\s+(\d+)", h).group(1)) == 8
    assert re.search(r"\bint\s+ultr_metrics_report\s*\(", h) and re.search(r"\bint\s+ultr_dnn_forward_metrics\s*\(", h)
    assert [M.IDS[n] for n in M.NAMES] == list(range(8)) and M.IDS["ordered_pair_accuracy"] == ids["OPA"]
    from ultra_pytorch_amd import _lib, engine
    assert "ultr_metrics_report" in _lib.SIGNATURES and "ultr_dnn_forward_metrics" in _lib.SIGNATURES
    assert engine.METRIC_IDS == M.IDS
