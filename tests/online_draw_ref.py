"""Host restatement of the online draw (csrc/ultr_online.hip): the query pick and candidate gather of online_pick_kernel, and the
re-ranking and clicks of online_rerank_kernel.  The uniforms come from tests/philox_ref.py (bit-exact); the query pick, the
deterministic stable sort and the click decisions are restated in the kernel's float32 arithmetic, so they match bit for bit; the
Plackett-Luce race keys and the zero-probability test are restated in float64 (the kernel's fp32 ones agree wherever two
keys, or a log-probability and the zero threshold, are not within rounding)."""
import numpy as np

from tests import draw_ref as D
from tests import philox_ref as P

DETERMINISTIC, STOCHASTIC = 0, 1
QUERY_TAG, RACE_TAG, CLICK_TAG = 0x0F1A3E01, 0x0F1A3E02, 0x0F1A3E03
TAGS = (QUERY_TAG, RACE_TAG, CLICK_TAG)


def pick(seed, step, B, n_queries, eligible=None):
    """Query index of every slot: uniform over `eligible` (an index array) or over all n_queries."""
    k = P.key(seed, step)
    b = np.arange(B, dtype=np.uint64)
    u = P.u01(P.philox4x32(b, 0, 0xFFFFFFFF, QUERY_TAG, *k)[0])
    n = len(eligible) if eligible is not None else n_queries
    i = np.minimum(np.floor(u.astype(np.float64) * np.float64(n)).astype(np.int64), n - 1)
    return (np.asarray(eligible, np.int64)[i] if eligible is not None else i).astype(np.int64)


def gather(lists, labels, q, M, n_docs):
    """Candidates of the picked queries: docids [M, B] int32 (PAD = n_docs), labels [M, B] float32 (0 at a PAD)."""
    lists, labels = np.asarray(lists, np.int32), np.asarray(labels, np.float32)
    lmax = lists.shape[1]
    B = len(q)
    d = np.full((M, B), -1, np.int64)
    y = np.zeros((M, B), np.float32)
    m = min(M, lmax)
    d[:m] = lists[q, :m].T
    y[:m] = labels[q, :m].T
    valid = d >= 0
    return np.where(valid, d, n_docs).astype(np.int32), np.where(valid, y, np.float32(0)).astype(np.float32)


def list_len(cand_docids, n_docs):
    """1 + the last non-PAD position of every slot [B]."""
    valid = np.asarray(cand_docids) != n_docs
    M = valid.shape[0]
    last = np.where(valid.any(0), M - 1 - np.argmax(valid[::-1], axis=0), -1)
    return last + 1


def order_key(s):
    """The kernel's unsigned order key of float32 scores: NaN above +inf, -0 == +0 (rank_order_key, ndcg_list_kernel's too)."""
    s = np.asarray(s, np.float32)
    s = np.where(s == 0, np.float32(0), s).astype(np.float32)
    u = s.view(np.uint32).astype(np.uint64)
    k = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(s), 0xFFFFFFFF, k).astype(np.uint64)


def rank_by_keys(keys):
    """Candidate index at each rank: descending unsigned keys, ties by index (the kernel's rank by counting)."""
    keys = np.asarray(keys, np.uint64).astype(np.int64)
    return np.lexsort((np.arange(len(keys)), -keys))


def race_uniforms(seed, step, b, n):
    """u[l] of slot b for l < n: word l & 3 of Philox(b, 0, l >> 2, RACE_TAG)."""
    k = P.key(seed, step)
    groups = (n + 3) // 4
    w = P.philox4x32(b, 0, np.arange(groups, dtype=np.uint64), RACE_TAG, *k)
    return P.u01(np.stack(w, axis=1).reshape(-1)[:n])


LN_ZERO_PROB = np.float64(np.float32(-103.97208))  # ln 2^-150: an fp32 probability below it rounds to 0


def race_keys(scores, tau, u):
    """float64 race keys tau (s - max) - log E, E = -log(1 - u); the zero-probability mask (log p = tau (s - max) - log sum below
    ln 2^-150, the underflow rule); and each document's distance from that threshold."""
    s32 = np.asarray(scores, np.float32)
    mx = np.max(s32)
    lw32 = (np.float32(tau) * (s32 - mx)).astype(np.float32)
    lp = lw32.astype(np.float64) - np.log(np.exp(lw32.astype(np.float64)).sum())
    e = -np.log1p(-np.asarray(u, np.float64))
    with np.errstate(divide="ignore"):
        keys = lw32.astype(np.float64) - np.log(e)
    return keys, lp < LN_ZERO_PROB, np.abs(lp - LN_ZERO_PROB)


def stochastic_order(scores, tau, u):
    """Drawn documents by descending race key, then the zero-probability ones in index order.  Returns the order, the keys, the
    zero mask and the distances from the zero threshold."""
    keys, zero, margin = race_keys(scores, tau, u)
    drawn = np.flatnonzero(~zero)
    drawn = drawn[np.argsort(-keys[drawn], kind="stable")]
    return np.concatenate([drawn, np.flatnonzero(zero)]).astype(np.int64), keys, zero, margin


def click_uniforms(seed, step, b, attempt, n):
    k = P.key(seed, step)
    groups = (n + 3) // 4
    w = P.philox4x32(b, attempt, np.arange(groups, dtype=np.uint64), CLICK_TAG, *k)
    return P.u01(np.stack(w, axis=1).reshape(-1)[:n])


def decide(y, u, model, exam, n_exam, cprob):
    """click_decide (csrc/ultr_feed.h) over one list: labels y [n] float32, uniforms u [n] float32."""
    y, u = np.asarray(y, np.float32), np.asarray(u, np.float32)
    exam, cprob = np.asarray(exam, np.float32).reshape(-1), np.asarray(cprob, np.float32)
    n, n_rel = len(y), len(cprob)
    lab = np.where(y > 0, np.trunc(y), 0).astype(np.int64)
    cp = cprob[np.minimum(lab, n_rel - 1)]
    if model == D.UBM:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = (u / cp).astype(np.float32)
        ck, last = np.zeros(n, np.float32), -1
        for r in range(n):
            ex = D.ubm_exam(exam, n_exam, r, np.int64(r - last))
            if ratio[r] < ex:
                ck[r], last = 1.0, r
        return ck
    ck = (u < (exam[np.minimum(np.arange(n), n_exam - 1)] * cp).astype(np.float32)).astype(np.float32)
    if model == D.CASCADE and ck.any():
        first = int(np.argmax(ck))
        ck = np.zeros(n, np.float32)
        ck[first] = 1.0
    return ck


def rerank(cand_docids, cand_labels, scores, n_docs, seed, step, mode, tau, rank_list_size, max_redraws, oracle_mode,
           model, exam, n_exam, cprob):
    """What ultr_online_rerank_args writes: docids [M, B], labels [M, B], perm [M, B]; plus the attempt each slot kept [B]."""
    cand_docids, cand_labels = np.asarray(cand_docids, np.int32), np.asarray(cand_labels, np.float32)
    scores = np.asarray(scores, np.float32)
    M, B = cand_docids.shape
    lens = list_len(cand_docids, n_docs)
    docids = np.full((M, B), n_docs, np.int32)
    labels = np.zeros((M, B), np.float32)
    perm = np.tile(np.arange(M, dtype=np.int32)[:, None], (1, B))
    kept = np.zeros(B, np.int64)
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        if mode == DETERMINISTIC:
            order = rank_by_keys(order_key(scores[b, :n]))
        else:
            order = stochastic_order(scores[b, :n], tau, race_uniforms(seed, step, b, n))[0]
        perm[:n, b] = order
        docids[:n, b] = cand_docids[order, b]
        cut = min(n, rank_list_size)
        if cut <= 0:
            continue
        y = cand_labels[order[:cut], b]
        if oracle_mode:
            labels[:cut, b] = y
            continue
        for attempt in range(1 + max_redraws):
            ck = decide(y, click_uniforms(seed, step, b, attempt, cut), model, exam, n_exam, cprob)
            kept[b] = attempt
            if ck.sum() > 0:
                break
        labels[:cut, b] = ck
    return docids, labels, perm, kept
