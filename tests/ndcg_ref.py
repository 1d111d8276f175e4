"""A float64 restatement of validation's NDCG@k (ultr_ndcg / ultr_ndcg_report / ultr_dnn_forward_ndcg, csrc/ultr_metrics.hip), written
from metrics.py's definition with weights = None and the kernel's documented tie rule: a STABLE descending order (equal scores keep
index order).  NaN orders above every number and a NaN in a row propagates through the row minimum given to invalid labels - what
torch's sort and min (the oracle, metrics.py) do."""
import numpy as np

PAD_SCORE = np.float32(-100000.0)


def masked_scores(scores, docids_LB=None, n_docs=None):
    """remove_padding_for_metric_eval: float32 [B, L] with PAD positions (docid == n_docs) at -100000."""
    s = np.array(scores, dtype=np.float32)
    if docids_LB is not None:
        s[np.asarray(docids_LB).T == n_docs] = PAD_SCORE
    return s


def prepare(scores, labels_BL):
    """metrics.py:251-264: labels < 0 -> 0, their prediction -> float32 row minimum - 1e-6 (NaN when the row holds a NaN)."""
    s = np.array(scores, dtype=np.float32)
    y = np.asarray(labels_BL, dtype=np.float32)
    ok = y >= 0
    mn = np.min(s, axis=1, keepdims=True)  # propagates NaN like torch.min
    s = np.where(ok, s, np.float32(-1e-6) + mn).astype(np.float32)
    return s, np.where(ok, y, np.float32(0)).astype(np.float32)


def stable_order(s):
    """Descending, NaN first, ties by index: [B, L] int64."""
    s = np.asarray(s, dtype=np.float32)
    nan = np.isnan(s)
    idx = np.broadcast_to(np.arange(s.shape[1]), s.shape)
    return np.lexsort((idx, -np.where(nan, 0, s).astype(np.float64), ~nan), axis=-1)


def ndcg_per_list(scores, labels_BL, topn):
    """Per-list NDCG@k [B, len(topn)] in float64, the permutation [B, L], the prepared scores [B, L]."""
    s, y = prepare(scores, labels_BL)
    B, L = s.shape
    order = stable_order(s)
    gain = np.exp2(y.astype(np.float64)) - 1.0
    disc = 1.0 / np.log2(np.arange(L, dtype=np.float64) + 2.0)
    dcg = np.cumsum(np.take_along_axis(gain, order, axis=1) * disc, axis=1)
    idcg = np.cumsum(-np.sort(-gain, axis=1) * disc, axis=1)
    out = np.zeros((B, len(topn)))
    for k, n in enumerate(topn):
        n = min(int(n), L)
        d, i = dcg[:, n - 1], idcg[:, n - 1]
        out[:, k] = np.where(i == 0, 0.0, d / np.where(i == 0, 1.0, i))
    return out, order, s
