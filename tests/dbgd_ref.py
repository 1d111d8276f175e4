"""Host restatement of the DBGD / MGD kernels (csrc/ultr_dbgd.hip): the candidate noise of dbgd_noise_kernel (Philox normals through
Box-Muller and F.normalize, in float64), the rankings, team-draft multileave, clicks and winners of dbgd_interleave_kernel (in the
kernel's float32 arithmetic where it decides: bit for bit in deterministic mode), and the ranker weights of dbgd_grad_kernel.
The uniforms come from tests/philox_ref.py; the click decisions from tests/online_draw_ref.py."""
import numpy as np

from tests import online_draw_ref as O
from tests import philox_ref as P

NOISE_TAG, RACE_TAG, SHUFFLE_TAG, CLICK_TAG = 0x0DB6D001, 0x0DB6D002, 0x0DB6D003, 0x0DB6D004
DETERMINISTIC, STOCHASTIC = O.DETERMINISTIC, O.STOCHASTIC


def layout(F, hidden):
    """Per Linear layer (off_gamma, K, off_w, M, off_bias) of the flat DNN vector (ranking_model/dnn.py: gamma | beta | W | bias)."""
    dims = list(zip([F] + list(hidden), list(hidden) + [1]))
    out, off = [], 0
    for k, m in dims:
        out.append((off, k, off + 2 * k, m, off + 2 * k + m * k))
        off += 2 * k + m * k + m
    return out, off


def normals(seed, step, R, P_):
    """z [R, P] in float64: Box-Muller on word 0 (u1 in (0, 1]) and word 1 (u2 in [0, 1)) of Philox(e, r, 0, NOISE_TAG)."""
    k = P.key(seed, step)
    e = np.arange(P_, dtype=np.uint64)
    z = np.empty((R, P_), np.float64)
    for r in range(R):
        w = P.philox4x32(e, r, 0, NOISE_TAG, *k)
        u1 = ((w[0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (w[1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        z[r] = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return z


def normalize(z, F, hidden, eps=1e-12):
    """create_noisy_param (dbgd.py:224-231): F.normalize(z, dim=0) per Linear weight [out, in] (per column) and bias; 0 on LayerNorm."""
    lay, P_ = layout(F, hidden)
    z = np.asarray(z, np.float64).reshape(-1, P_)
    u = np.zeros_like(z)
    for (og, k, ow, m, ob) in lay:
        W = z[:, ow:ow + m * k].reshape(-1, m, k)
        u[:, ow:ow + m * k] = (W / np.maximum(np.sqrt((W ** 2).sum(1, keepdims=True)), eps)).reshape(-1, m * k)
        bvec = z[:, ob:ob + m]
        u[:, ob:ob + m] = bvec / np.maximum(np.sqrt((bvec ** 2).sum(1, keepdims=True)), eps)
    return u


def list_len(docids_col, n_docs):
    valid = np.flatnonzero(np.asarray(docids_col) != n_docs)
    return int(valid[-1]) + 1 if valid.size else 0


def race_uniforms(seed, step, b, j, n):
    k = P.key(seed, step)
    w = P.philox4x32(b, j, np.arange((n + 3) // 4, dtype=np.uint64), RACE_TAG, *k)
    return P.u01(np.stack(w, axis=1).reshape(-1)[:n])


def ranking(scores, n, mode, tau=1.0, seed=0, step=0, b=0, j=0):
    """Ranker j's order of the first n candidates of list b (the online feeds' stable sort / race, ultr_rank.h)."""
    s = np.asarray(scores, np.float32)[:n]
    if mode == DETERMINISTIC:
        return O.rank_by_keys(O.order_key(s)).astype(np.int64)
    return O.stochastic_order(s, tau, race_uniforms(seed, step, b, j, n))[0]


def philox_shuffle(seed, step, b):
    """The kernel's Fisher-Yates shuffle of the current assignment, round t of list b: uniforms Philox(b, t, i / 4, SHUFFLE_TAG)."""
    k = P.key(seed, step)

    def shuffle(t, asg):
        asg = list(asg)
        n = len(asg)
        if n < 2:
            return asg
        w = P.philox4x32(b, t, np.arange((n - 1 + 3) // 4, dtype=np.uint64), SHUFFLE_TAG, *k)
        u = P.u01(np.stack(w, axis=1).reshape(-1))
        for t_, i in enumerate(range(n - 1, 0, -1)):
            s = min(int(np.float32(u[t_]) * np.float32(i + 1)), i)
            asg[i], asg[s] = asg[s], asg[i]
        return asg
    return shuffle


def team_draft(rankings, shuffle):
    """TeamDraftInterleaving.interleave (team_draft_interleave.py:15-43) with the shuffle supplied: shuffle(round, assignment) ->
    the new assignment.  rankings [NR, n]; returns (multileaved [n], teams [n])."""
    rk = np.asarray(rankings, np.int64)
    NR, n = rk.shape
    ml, teams = np.zeros(n, np.int64), np.zeros(n, np.int64)
    p = 0
    while p < n and np.all(rk[1:, p] == rk[0, p]):
        ml[p], teams[p] = rk[0, p], -1
        p += 1
    idx = [p] * NR
    asg, ai, rnd = list(range(NR)), NR, 0
    placed = set(ml[:p].tolist())
    while p < n:
        if ai == NR:
            asg, ai, rnd = shuffle(rnd, asg), 0, rnd + 1
        r = asg[ai]
        i = idx[r]
        while i < n and rk[r, i] in placed:
            i += 1
        ml[p], teams[p] = rk[r, i], r
        placed.add(int(rk[r, i]))
        idx[r] = i + 1
        p += 1
        ai += 1
    return ml, teams


def click_uniforms(seed, step, b, attempt, n):
    k = P.key(seed, step)
    w = P.philox4x32(b, attempt, np.arange((n + 3) // 4, dtype=np.uint64), CLICK_TAG, *k)
    return P.u01(np.stack(w, axis=1).reshape(-1)[:n])


def winners(teams, clicks, NR):
    """infer_winner (:46-51) in the kernel's float32: clicks of team r / (clicks of all teams + 1e-7)."""
    rc = np.array([np.float32(sum(float(c) for t, c in zip(teams, clicks) if t == r)) for r in range(NR)], np.float32)
    tot = np.float32(0)
    for v in rc:
        tot = np.float32(tot + v)
    return (rc / np.float32(tot + np.float32(1e-7))).astype(np.float32)


def interleave(scores, docids, labels, n_docs, rank_list_size, mode, tau, seed, step, max_redraws, model, exam, n_exam, cprob,
               shuffles=None, clicks_in=None):
    """What dbgd_interleave_kernel writes: winners [B, NR], interleaved / teams / clicks [M, B].  scores [NR, B, M]; docids, labels
    [M, B]; shuffles [B, M, NR] and clicks_in [M, B] replace the Philox draws when given."""
    scores = np.asarray(scores, np.float32)
    NR, B, M = scores.shape
    W = np.zeros((B, NR), np.float32)
    inter = np.full((M, B), -1, np.int64)
    teams = np.full((M, B), -2, np.int64)
    clicks = np.zeros((M, B), np.float32)
    for b in range(B):
        n = list_len(docids[:, b], n_docs)
        rk = np.stack([ranking(scores[j, b], n, mode, tau, seed, step, b, j) for j in range(NR)]) if n else np.zeros((NR, 0), np.int64)
        sh = (lambda t, asg, b=b: list(shuffles[b, t])) if shuffles is not None else philox_shuffle(seed, step, b)
        ml, tm = team_draft(rk, sh)
        inter[:n, b], teams[:n, b] = ml, tm
        cut = min(n, rank_list_size)
        if cut > 0:
            if clicks_in is not None:
                ck = np.asarray(clicks_in, np.float32)[:cut, b]
            else:
                y = np.asarray(labels, np.float32)[ml[:cut], b]
                for attempt in range(1 + max_redraws):
                    ck = O.decide(y, click_uniforms(seed, step, b, attempt, cut), model, exam, n_exam, cprob)
                    if ck.sum() > 0:
                        break
            clicks[:cut, b] = ck
        W[b] = winners(tm[:cut], clicks[:cut, b], NR)
    return W, inter, teams, clicks


def ranker_weights(winners_BR=None, ndcg=None):
    """c_r of dbgd_grad_kernel: the batch mean of winners[:, r]; or, from the per-ranker batch NDCGs, the reference's batch-level
    winners w = ceil(ndcg_r - ndcg_0) / (sum + 1e-9) broadcast against [1, R + 1, ...] (dbgd.py:138-149, 196-222): mean_a w_a for
    every ranker."""
    if winners_BR is not None:
        return np.asarray(winners_BR, np.float64).mean(0)
    nd = np.asarray(ndcg, np.float32)
    g = np.ceil((nd - nd[0]).astype(np.float32)).astype(np.float32)
    w = g / np.float32(g.sum(dtype=np.float32) + np.float32(1e-9))
    return np.full(len(nd), np.float64(w.sum(dtype=np.float32)) / len(nd))


def gradient(u, c):
    """The direction the update applies: grads = -sum_{r >= 1} c_r u_r (u [R, P], c [R + 1]); the reference's parameter.grad is -grads."""
    u = np.asarray(u, np.float64)
    return -np.tensordot(np.asarray(c, np.float64)[1:], u, axes=1)
