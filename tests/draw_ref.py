"""Host restatements of the device draws, bit for bit: click_draw (csrc/ultr_feed.h) and the Bernoulli pseudo-labels of regem_kernel
(csrc/ultr_loss.hip) with uniforms == NULL.  Both are pure functions of (seed, step, counter), so numpy reproduces them exactly:
the uniforms through tests/philox_ref.py, the click decisions in the kernel's float32 arithmetic."""
import numpy as np

from tests import philox_ref as P

PBM, CASCADE, UBM = 0, 1, 2
QUERY_TAG, CLICK_TAG = 0x51ED270B, 0x2545F491
REGEM_TAG = 0x5245454D


def click_uniforms(k, b, attempt, L):
    """u[l, i] of slot b[i] at attempt[i]: word l & 3 of Philox(b, attempt, l >> 2, CLICK_TAG)."""
    groups = (L + 3) // 4
    g = np.arange(groups, dtype=np.uint64)[:, None]
    w = P.philox4x32(b[None, :], attempt[None, :], g, CLICK_TAG, *k)  # 4 x [groups, n]
    return np.stack(w, axis=1).reshape(groups * 4, -1)[:L]              # row 4 g + j = word j of group g


def ubm_exam(exam, n_exam, rank, dist):
    """The kernel's lookup in the dense [n_exam][n_exam] image (rank, dist arrays of one position for every slot)."""
    if rank < n_exam:
        return exam[rank * n_exam + dist - 1]
    far = dist > rank  # no click before this position
    col = np.where(dist < n_exam - 1, dist - 1, n_exam - 2 if n_exam >= 2 else 0)
    return np.where(far, exam[(n_exam - 1) * n_exam + n_exam - 1], exam[(n_exam - 1) * n_exam + col])


def click_draw(lists, labels, n_docs, exam, n_exam, cprob, model, seed, step, B, L, max_tries):
    """What ultr_click_batch writes.  lists / labels [n_queries, lmax] (int32 / float32), exam float32 ([n_exam] for PBM and
    cascade, the flat [n_exam * n_exam] image for UBM), cprob float32 [n_rel].  Returns docids [L, B] int32, clicks [L, B] float32,
    query_idx [B] int32, and for the second check: the attempt each slot kept [B], its uniforms [L, B] float32, labels used [L, B]."""
    lists, labels = np.asarray(lists, np.int32), np.asarray(labels, np.float32)
    exam, cprob = np.asarray(exam, np.float32).reshape(-1), np.asarray(cprob, np.float32)
    n_queries, lmax = lists.shape
    n_rel = len(cprob)
    k = P.key(seed, step)
    docids = np.zeros((L, B), np.int32)
    clicks = np.zeros((L, B), np.float32)
    qidx = np.zeros(B, np.int32)
    kept = np.zeros(B, np.int64)
    u_kept = np.zeros((L, B), np.float32)
    y_kept = np.zeros((L, B), np.float32)
    active = np.arange(B, dtype=np.int64)
    pos = np.arange(L)
    for attempt in range(max_tries):
        if active.size == 0:
            break
        n = active.size
        bb = active.astype(np.uint64)
        at = np.full(n, attempt, np.uint64)
        uq = P.u01(P.philox4x32(bb, at, 0xFFFFFFFF, QUERY_TAG, *k)[0])
        q = np.floor(uq.astype(np.float64) * np.float64(n_queries)).astype(np.int64)  # (int64)((double)u * (double)n_queries)
        q = np.minimum(q, n_queries - 1)
        d = np.full((L, n), -1, np.int64)
        inside = pos < lmax
        d[inside] = lists[q][:, pos[inside]].T
        valid = d >= 0
        ids = np.where(valid, d, n_docs).astype(np.int32)
        y = np.zeros((L, n), np.float32)
        y[inside] = labels[q][:, pos[inside]].T
        y = np.where(valid, y, np.float32(0))
        lab = np.where(y > 0, np.trunc(y), 0).astype(np.int64)  # (int)y for y > 0, else 0
        cp = cprob[np.minimum(lab, n_rel - 1)]
        u = P.u01(click_uniforms(k, bb, at, L))
        if model == UBM:
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = u / cp  # float32 division, correctly rounded like the kernel's; cp == 0 -> inf / NaN: never a click
            ck = np.zeros((L, n), np.float32)
            last = np.full(n, -1, np.int64)
            for r in range(L):
                ex = ubm_exam(exam, n_exam, r, r - last)
                hit = ratio[r] < ex
                ck[r] = hit
                last = np.where(hit, r, last)
        else:
            ex = exam[np.minimum(pos, n_exam - 1)][:, None]
            ck = (u < (ex * cp).astype(np.float32)).astype(np.float32)
            if model == CASCADE:
                first = np.where(ck.any(0), ck.argmax(0), L)
                ck = (pos[:, None] == first[None, :]).astype(np.float32)
        docids[:, active], clicks[:, active], qidx[active], kept[active] = ids, ck, q, attempt
        u_kept[:, active], y_kept[:, active] = u, y
        active = active[ck.sum(0) == 0]
    return docids, clicks, qidx, kept, u_kept, y_kept


def regem_uniforms(seed, step, B, L):
    """u[b, l] = u01(word 0 of Philox(b, l, REGEM_TAG, 1))."""
    b = np.arange(B, dtype=np.uint64)[:, None]
    l = np.arange(L, dtype=np.uint64)[None, :]
    return P.u01(P.philox4x32(b, l, REGEM_TAG, 1, *P.key(seed, step))[0])
