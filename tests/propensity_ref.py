"""Host restatement of ultr_propensity_count (csrc/ultr_propensity.hip), integer for integer: the session law of include/ultr_hip.h in
numpy, vectorised over sessions, on the Philox stream of tests/philox_ref.py and with the click decisions of tests/draw_ref.py (the
kernel's float32 arithmetic; ubm_exam and the model and tag constants are draw_ref's).  draw_ref keeps its PBM / cascade / UBM
decisions inline in click_draw, for one list length L per batch and with its redraw loop around them, so they cannot be imported as
a function: they are restated here per session with L = n (the `valid` mask), line for line in draw_ref's arithmetic.  Also: the
reference's first / agg / IPW_list formula (propensity_estimator.py:119-131) transcribed literally in float64, and the analytic
expectation of the counts under the position-biased model."""
import numpy as np

from tests import philox_ref as P
from tests.draw_ref import CASCADE, CLICK_TAG, PBM, QUERY_TAG, UBM, ubm_exam

SHUFFLE_TAG = 0x53485546  # csrc/ultr_feed.h: ULTR_SHUFFLE_TAG


def _words(k, lo, hi, n_pos, tag):
    """w[l, i]: word l & 3 of Philox(lo[i], hi[i], l >> 2, tag) for l < n_pos."""
    groups = (n_pos + 3) // 4
    g = np.arange(groups, dtype=np.uint64)[:, None]
    w = P.philox4x32(lo[None, :], hi[None, :], g, tag, *k)
    return np.stack(w, axis=1).reshape(groups * 4, -1)[:n_pos]


def sessions(labels, lengths, exam, n_exam, cprob, model, seed, s):
    """The sessions s (uint64 array): q [S], n [S], perm [lmax, S] (rank -> index, ranks >= n meaningless), clicks [lmax, S] bool."""
    labels, lengths = np.asarray(labels, np.float32), np.asarray(lengths, np.int64)
    exam, cprob = np.asarray(exam, np.float32).reshape(-1), np.asarray(cprob, np.float32)
    n_queries, lmax = labels.shape
    n_rel = len(cprob)
    s = np.asarray(s, np.uint64)
    lo, hi = s & P.MASK, s >> np.uint64(32)
    k = P.key(seed, 0)
    uq = P.u01(P.philox4x32(lo, hi, 0xFFFFFFFF, QUERY_TAG, *k)[0])
    q = np.minimum(np.floor(uq.astype(np.float64) * np.float64(n_queries)).astype(np.int64), n_queries - 1)
    n = lengths[q]
    pos = np.arange(lmax)
    valid = pos[:, None] < n[None, :]
    # descending by key, ties by index; positions >= n behind every valid one
    keys = np.where(valid, _words(k, lo, hi, lmax, SHUFFLE_TAG).astype(np.int64), -1)
    perm = np.argsort(-keys, axis=0, kind="stable")
    y = np.where(valid, labels[q[None, :], perm], np.float32(0))
    u = P.u01(_words(k, lo, hi, lmax, CLICK_TAG))
    lab = np.where(y > 0, np.trunc(y), 0).astype(np.int64)
    cp = cprob[np.minimum(lab, n_rel - 1)]
    if model == UBM:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = u / cp
        ck = np.zeros(valid.shape, bool)
        last = np.full(len(s), -1, np.int64)
        for r in range(lmax):
            hit = (ratio[r] < ubm_exam(exam, n_exam, r, r - last)) & valid[r]
            ck[r] = hit
            last = np.where(hit, r, last)
    else:
        ex = exam[np.minimum(pos, n_exam - 1)][:, None]
        ck = (u < (ex * cp).astype(np.float32)) & valid
        if model == CASCADE:
            first = np.where(ck.any(0), ck.argmax(0), lmax)
            ck = pos[:, None] == first[None, :]
    return q, n, perm, ck


def click_count(labels, lengths, exam, n_exam, cprob, model, seed, first_session, n_sessions, chunk=1 << 16):
    """What ultr_propensity_count adds to a zero table: int64 [lmax, lmax], row = list length - 1, column = position."""
    lmax = np.asarray(labels).shape[1]
    count = np.zeros(lmax * lmax, np.int64)
    pos = np.arange(lmax)[:, None]
    for at in range(0, n_sessions, chunk):
        m = min(chunk, n_sessions - at)
        s = (np.arange(m, dtype=np.uint64) + np.uint64((first_session + at) & (2 ** 64 - 1)))
        _, n, _, ck = sessions(labels, lengths, exam, n_exam, cprob, model, seed, s)
        idx = ((n[None, :] - 1) * lmax + pos)[ck]
        count += np.bincount(idx, minlength=lmax * lmax)
    return count.reshape(lmax, lmax)


def ipw_formula(click_count):
    """propensity_estimator.py:119-131 on a square table of counts (the reference's rows are ragged: row y holds y + 1 entries; the
    entries beyond are never read), in float64."""
    n = len(click_count)
    first_click_count = [0 for _ in range(n)]
    agg_click_count = [0 for _ in range(n)]
    for x in range(n):
        for y in range(x, n):
            first_click_count[x] += int(click_count[y][0])
            agg_click_count[x] += int(click_count[y][x])
    return [min(first_click_count[x] / (agg_click_count[x] + 10e-6), first_click_count[x]) for x in range(n)]


def pbm_expectation(labels, lengths, exam, cprob, n_sessions):
    """Position-biased model: (E[first_x], E[agg_x], the true weight exam[0] / exam[min(x, n_exam - 1)]) per position, float64.
    A session picks list q with probability 1 / n_queries; after a uniform shuffle the label at any position is uniform over the
    list, so a click on position x of a list that has one has probability exam[min(x, n_exam - 1)] * mean click probability."""
    labels, lengths = np.asarray(labels), np.asarray(lengths, np.int64)
    exam, cprob = np.asarray(exam, np.float64), np.asarray(cprob, np.float64)
    n_queries, lmax = labels.shape
    mean_cp = np.zeros(n_queries)
    for q in range(n_queries):
        lab = np.clip(np.asarray(labels[q, :lengths[q]], np.int64), 0, len(cprob) - 1)
        mean_cp[q] = cprob[lab].mean() if lengths[q] > 0 else 0.0
    first, agg, true = np.zeros(lmax), np.zeros(lmax), np.zeros(lmax)
    for x in range(lmax):
        mass = mean_cp[lengths > x].sum() / n_queries * n_sessions
        e = exam[min(x, len(exam) - 1)]
        first[x], agg[x], true[x] = mass * exam[0], mass * e, exam[0] / e
    return first, agg, true


def six_sigma(ipw, e_first, e_agg):
    """6 sigma_x, sigma_x = IPW[x] * sqrt(1 / E[first_x] + 1 / E[agg_x]): the ratio of two counts with these means."""
    return 6.0 * np.asarray(ipw, np.float64) * np.sqrt(1.0 / e_first + 1.0 / e_agg)
