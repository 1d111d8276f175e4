"""A float64 restatement of the eight validation metrics of ultr_metrics_report (csrc/ultr_metrics.hip), written from utils/metrics.py's
definitions with weights = None: per-list values and their batch means.  The order and the prepared scores are those of
tests/ndcg_ref.py (stable descending, NaN first), so ties and invalid labels fall where the kernel documents them."""
import numpy as np

from tests import ndcg_ref as N

NAMES = ("ndcg", "dcg", "mrr", "err", "map", "arp", "precision", "ordered_pair_accuracy")
IDS = {name: k for k, name in enumerate(NAMES)}  # ULTR_METRIC_* (include/ultr_hip.h)
UNBOUNDED = ("dcg", "arp")  # every other metric lies in [0, 1]


def per_list(scores, labels_BL, topn, max_label=4.0):
    """{name: float64 [B, len(topn)]} of masked scores [B, L] and labels [B, L]; the permutation [B, L]."""
    ndcg, order, s = N.ndcg_per_list(scores, labels_BL, topn)
    raw = np.asarray(labels_BL, dtype=np.float32)
    m = np.array(scores, dtype=np.float32)
    valid = raw >= 0
    y = np.where(valid, raw, np.float32(0)).astype(np.float64)
    B, L = y.shape
    K = len(topn)
    sl = np.take_along_axis(y, order, axis=1)  # validated labels by predicted rank
    pos = np.arange(1, L + 1, dtype=np.float64)
    out = {"ndcg": ndcg}
    gain = (np.exp2(sl) - 1.0) / np.log2(pos + 1.0)
    rel = (np.exp2(sl) - 1.0) / 2.0 ** float(max_label)
    excl = np.concatenate([np.ones((B, 1)), np.cumprod(1.0 - rel, axis=1)[:, :-1]], axis=1)  # prod over the ranks before
    err_terms = rel * excl / pos
    out["dcg"], out["err"] = np.zeros((B, K)), np.zeros((B, K))
    for k, n in enumerate(topn):
        n = min(int(n), L)
        out["dcg"][:, k] = gain[:, :n].sum(1)
        out["err"][:, k] = err_terms[:, :n].sum(1)
    hit = sl >= 1.0
    nhit = hit.sum(1)
    mrr = np.where(nhit > 0, 1.0 / (np.argmax(hit, axis=1) + 1.0), 0.0)
    ap = (np.cumsum(hit, axis=1) / pos * hit).sum(1)
    mapv = np.where(nhit > 0, ap / np.maximum(nhit, 1), 0.0)
    den = sl.sum(1)
    arp = np.where(den == 0, 0.0, (pos * sl).sum(1) / np.where(den == 0, 1.0, den))
    prec = nhit / float(L)
    with np.errstate(invalid="ignore"):
        pair = (y[:, :, None] > y[:, None, :]) & (m[:, :, None] > m[:, None, :]) & valid[:, :, None] & valid[:, None, :]
    opa = pair.sum((1, 2)) / float(L * L)
    for name, v in (("mrr", mrr), ("map", mapv), ("arp", arp), ("precision", prec), ("ordered_pair_accuracy", opa)):
        out[name] = np.repeat(np.asarray(v, dtype=np.float64)[:, None], K, axis=1)  # no cutoff: the value once per cutoff
    return out, order


def batch_means(per):
    return {name: v.mean(0) for name, v in per.items()}
