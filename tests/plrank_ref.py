"""Yardstick of PLRank (csrc/ultr_plrank.hip): the law in numpy float64, with the sampled orders as an INPUT.

  reference()        dscores, sum |terms| per output, the per-list loss and the step tail head, from scores, rho, validity and orders
  host_orders()      the race restated on the host: tests/philox_ref.py uniforms under PLRANK_TAG, tests/online_draw_ref.py keys
  enumerate_exact()  all permutations of a short list: the exact reward, the estimator's expectation and its standard deviation
  kernel_f32()       the kernel's float32 arithmetic restated in numpy (staging in two factors, the wave scans in trips of 64)
  update_ref()       the step tail of the update launch for this algorithm (D counts lists, l2_loss, the clip over the full gradient)
"""
import itertools

import numpy as np

from tests import online_draw_ref as OD
from tests import philox_ref as P

PLRANK_TAG = 0x504C524B
MAX_L = 465          # the longest list of PlRankLds (160 KiB)
LOSS_JW = 16
F32_TINY = float(np.finfo(np.float32).tiny)  # below it a float32 has no relative precision: the floor of every dscores bar
SHIFT, SPLIT = np.float32(64.0), np.float32(-80.0)


def gain_of(y, gain):
    y = np.asarray(y, np.float32).astype(np.float64)
    if gain == "linear":
        return y
    if gain == "exp2":
        return np.exp2(y) - 1.0
    raise ValueError(gain)


def valid_of(docids_LB, n_docs):
    """[B, L] bool: a docid in [0, n_docs)."""
    d = np.asarray(docids_LB).T
    return (d >= 0) & (d < n_docs)


def rho_of(labels_LB, valid, gain="linear", pw=None, ipw=None):
    """[B, L] float64 rho = w gain(y), 0 at a PAD.  w: pw [B, L], else ipw[min(l, n - 1)], else 1 (float32 inputs, float64 product)."""
    y = np.asarray(labels_LB, np.float32).T
    B, L = y.shape
    if pw is not None:
        w = np.asarray(pw, np.float32).astype(np.float64).reshape(B, L)
    elif ipw is not None:
        t = np.asarray(ipw, np.float32).astype(np.float64)
        w = np.broadcast_to(t[np.minimum(np.arange(L), len(t) - 1)], (B, L))
    else:
        w = np.ones((B, L))
    return np.where(valid, w * gain_of(y, gain), 0.0)


def cutoff_of(cutoff, L):
    return L if cutoff == 0 or cutoff > L else int(cutoff)


def n_pos_of(scores, valid):
    """Per list: the number of drawn documents (valid, float32 probability not 0 by the log rule of online_draw_ref.race_keys), and the
    smallest distance of a valid document's log-probability from the zero threshold."""
    scores, valid = np.asarray(scores, np.float32), np.asarray(valid, bool)
    B = scores.shape[0]
    n_pos, margin = np.zeros(B, np.int64), np.full(B, np.inf)
    for b in range(B):
        if valid[b].any():
            s = np.where(valid[b], scores[b], np.float32(-np.inf)).astype(np.float32)
            _, zero, m = OD.race_keys(s, 1.0, np.full(len(s), 0.5, np.float32))
            n_pos[b] = int((~zero).sum())
            margin[b] = float(np.min(m[valid[b]]))
    return n_pos, margin


def race_uniforms(seed, step, b, n, L):
    """u[l] of list b, sample n: word l & 3 of Philox(key(seed, step); b, n, l >> 2, PLRANK_TAG)."""
    k = P.key(seed, step)
    w = P.philox4x32(b, n, np.arange((L + 3) // 4, dtype=np.uint64), PLRANK_TAG, *k)
    return P.u01(np.stack(w, axis=1).reshape(-1)[:L])


def order_of(scores_b, valid_b, u):
    """One sample of one list from its uniforms: (order [L], separated).  PADs are staged as -inf; `separated` is the existing rule -
    every two drawn float64 keys more than 1e-4 apart and every valid log-probability more than 1e-4 from the zero threshold."""
    L = len(scores_b)
    if not valid_b.any():
        return np.arange(L, dtype=np.int64), True
    s = np.where(valid_b, scores_b, np.float32(-np.inf)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        order, keys, zero, margin = OD.stochastic_order(s, 1.0, u)
    k = np.sort(keys[~zero])
    sep = (len(k) < 2 or float(np.min(np.diff(k))) > 1e-4) and float(np.min(margin[valid_b])) > 1e-4
    return order, bool(sep)


def host_orders(scores, valid, seed, step, N):
    """orders [B, N, L] int64 and separated [B, N] bool of the device draw, restated on the host."""
    scores, valid = np.asarray(scores, np.float32), np.asarray(valid, bool)
    B, L = scores.shape
    orders, sep = np.zeros((B, N, L), np.int64), np.zeros((B, N), bool)
    for b in range(B):
        for n in range(N):
            orders[b, n], sep[b, n] = order_of(scores[b], valid[b], race_uniforms(seed, step, b, n, L))
    return orders, sep


def _suffix(x):
    return np.flip(np.cumsum(np.flip(x, -1), -1), -1)


def per_sample(scores, rho, valid, orders, K, n_pos):
    """g [B, N, L] (by document) and its sum |terms|, FR_0 [B, N]: the law per sample, float64, vectorised over lists and samples."""
    s = np.asarray(scores, np.float32).astype(np.float64)
    rho, valid, orders = np.asarray(rho, np.float64), np.asarray(valid, bool), np.asarray(orders, np.int64)
    B, N, L = orders.shape
    mx = np.max(np.where(valid, s, -np.inf), axis=1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(valid, np.exp(np.where(valid, s - mx, 0.0)), 0.0)  # [B, L]
    k_eff = np.minimum(K, np.asarray(n_pos, np.int64))[:, None, None]  # [B, 1, 1]
    ranks = np.arange(L)[None, None, :]
    theta = 1.0 / np.log2(ranks + 2.0)
    take = lambda a: np.take_along_axis(np.broadcast_to(a[:, None, :], (B, N, L)), orders, axis=2)  # noqa: E731
    e_r, rho_r, v_r = take(e), take(rho), take(valid)
    inside = ranks < k_eff
    Z = _suffix(e_r)
    FR = np.concatenate([_suffix(np.where(inside, theta * rho_r, 0.0)), np.zeros((B, N, 1))], axis=2)  # [B, N, L + 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        RI = np.cumsum(np.where(inside, FR[..., :L] / np.where(inside, Z, 1.0), 0.0), axis=2)
        DR = np.cumsum(np.where(inside, theta / np.where(inside, Z, 1.0), 0.0), axis=2)
    # (terms at ranks >= K_eff are 0: the running sums at rank r are those at i = min(r, K_eff - 1))
    direct = np.where(inside, FR[..., 1:], 0.0)
    g_r = np.where(v_r, direct + e_r * (rho_r * DR - RI), 0.0)
    t_r = np.where(v_r, np.abs(direct) + e_r * np.abs(rho_r) * DR + e_r * np.abs(RI), 0.0)
    live = (k_eff > 0)
    g_r, t_r = np.where(live, g_r, 0.0), np.where(live, t_r, 0.0)
    g, t = np.zeros((B, N, L)), np.zeros((B, N, L))
    np.put_along_axis(g, orders, g_r, axis=2)
    np.put_along_axis(t, orders, t_r, axis=2)
    return g, t, np.where(live[..., 0], FR[..., 0], 0.0)


def reference(scores, rho, valid, orders, cutoff, n_pos=None):
    """dict: dscores [B, L] = -(1 / N) sum_n g, terms [B, L] = (1 / N) sum_n sum |terms|, loss_b [B] = -(1 / N) sum_n FR_0, and the
    step tail head [sum_b loss_b, B] (D counts lists)."""
    scores = np.asarray(scores, np.float32)
    B, L = scores.shape
    if n_pos is None:
        n_pos = n_pos_of(scores, valid)[0]
    g, t, fr0 = per_sample(scores, rho, valid, orders, cutoff_of(cutoff, L), n_pos)
    loss_b = -fr0.mean(axis=1)
    return dict(dscores=-g.mean(axis=1), terms=t.mean(axis=1), loss_b=loss_b, tail=np.array([loss_b.sum(), float(B)]))


def dscores_bar(ref, terms, rtol):
    """The project's terms bar for dscores, with float32's smallest normal as floor."""
    return rtol * (np.abs(ref) + terms) + F32_TINY


# ---- exact enumeration of a short list -----------------------------------------------------------------------------------------
def enumerate_exact(scores, rho, K):
    """All L! rankings of one all-valid list: (reward, expectation of g [L], standard deviation of g [L]) under PL(scores)."""
    s = np.asarray(scores, np.float64)
    L = len(s)
    e = np.exp(s - s.max())
    perms = np.array(list(itertools.permutations(range(L))), np.int64)  # [M, L]
    e_r = e[perms]
    prob = np.prod(e_r / _suffix(e_r), axis=1)
    s32 = s.astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), s), "enumerate_exact: scores must be float32 values"
    g, _, fr0 = per_sample(s32[None], np.asarray(rho, np.float64)[None], np.ones((1, L), bool), perms[None], K, np.array([L]))
    g, fr0 = g[0], fr0[0]
    mean = (prob[:, None] * g).sum(axis=0)
    var = (prob[:, None] * g * g).sum(axis=0) - mean * mean
    return float((prob * fr0).sum()), mean, np.sqrt(np.maximum(var, 0.0))


def exact_reward(scores, rho, K):
    """E[sum_{k < K} theta_k rho_{y_k}] by enumeration, float64 scores (for central differences)."""
    s = np.asarray(scores, np.float64)
    L = len(s)
    e = np.exp(s - s.max())
    perms = np.array(list(itertools.permutations(range(L))), np.int64)
    e_r = e[perms]
    prob = np.prod(e_r / _suffix(e_r), axis=1)
    theta = 1.0 / np.log2(np.arange(L) + 2.0)
    rew = (np.where(np.arange(L) < K, theta, 0.0)[None, :] * np.asarray(rho, np.float64)[perms]).sum(axis=1)
    return float((prob * rew).sum())


# ---- the kernel's float32 arithmetic ---------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, np.float32)


def stage_f32(scores, valid):
    """ea, eb [B, L] float32: e * exp(SHIFT) in two factors, as plrank_kernel stages it (two-term sums for s - max and the shift)."""
    s = _f32(scores)
    valid = np.asarray(valid, bool)
    mx = np.max(np.where(valid, s, np.float32(-np.inf)), axis=1, keepdims=True).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sv = np.where(valid, s, mx).astype(np.float32)
        hi = _f32(sv - mx)
        bb = _f32(hi - sv)
        lo = _f32(_f32(sv - _f32(hi - bb)) - _f32(mx + bb))
        t = _f32(hi + SHIFT)
        tb = _f32(t - hi)
        lo = _f32(lo + _f32(_f32(hi - _f32(t - tb)) + _f32(SHIFT - tb)))
        ea = _f32(np.exp(np.maximum(t, SPLIT), dtype=np.float32) * _f32(np.float32(1.0) + lo))
        eb = np.exp(np.minimum(_f32(t - SPLIT), np.float32(0.0)), dtype=np.float32)
    return np.where(valid, ea, np.float32(0)).astype(np.float32), np.where(valid, eb, np.float32(0)).astype(np.float32)


def _wave_scan(x, suffix):
    """Inclusive Hillis-Steele scan over the 64 lanes of the last axis in float32, the order of wave_suffix2 / wave_prefix2."""
    x = x.copy()
    o = 1
    while o < 64:
        y = x.copy()
        if suffix:
            y[..., :64 - o] = _f32(x[..., :64 - o] + x[..., o:])
        else:
            y[..., o:] = _f32(x[..., o:] + x[..., :64 - o])
        x, o = y, o * 2
    return x


def _trip_scan(x, suffix):
    """x [..., L] float32: the kernel's scan over ranks in trips of 64 lanes with a carry (suffix: from the last trip to the first)."""
    L = x.shape[-1]
    T = (L + 63) // 64
    pad = np.zeros(x.shape[:-1] + (T * 64,), np.float32)
    pad[..., :L] = x
    out = np.zeros_like(pad)
    carry = np.zeros(x.shape[:-1] + (1,), np.float32)
    for t in (range(T - 1, -1, -1) if suffix else range(T)):
        v = _f32(_wave_scan(pad[..., t * 64:(t + 1) * 64], suffix) + carry)
        out[..., t * 64:(t + 1) * 64] = v
        carry = v[..., :1] if suffix else v[..., 63:]
    return out[..., :L]


def kernel_f32(scores, rho, valid, orders, cutoff, n_pos):
    """g [B, N, L] float32 per sample and FR_0 [B, N], in the kernel's arithmetic and order of operations."""
    scores, valid, orders = _f32(scores), np.asarray(valid, bool), np.asarray(orders, np.int64)
    B, N, L = orders.shape
    K = cutoff_of(cutoff, L)
    ea, eb = stage_f32(scores, valid)
    rho32 = _f32(rho)
    k_eff = np.minimum(K, np.asarray(n_pos, np.int64))[:, None, None]
    ranks = np.arange(L)[None, None, :]
    theta = _f32(np.float32(1.0) / np.log2(_f32(ranks + 2.0), dtype=np.float32))
    take = lambda a: np.take_along_axis(np.broadcast_to(a[:, None, :], (B, N, L)), orders, axis=2)  # noqa: E731
    ea_r, eb_r, rho_r, v_r = take(ea), take(eb), take(rho32), take(valid)
    inside = ranks < k_eff
    Z = _trip_scan(_f32(ea_r * eb_r), True)
    FRs = _trip_scan(np.where(inside, _f32(theta * rho_r), np.float32(0)).astype(np.float32), True)
    FR = np.concatenate([FRs, np.zeros((B, N, 1), np.float32)], axis=2)
    zs = np.where(inside, Z, np.float32(1)).astype(np.float32)
    RI = _trip_scan(np.where(inside, _f32(FR[..., :L] / zs), np.float32(0)).astype(np.float32), False)
    DR = _trip_scan(np.where(inside, _f32(theta / zs), np.float32(0)).astype(np.float32), False)
    direct = np.where(inside, FR[..., 1:], np.float32(0)).astype(np.float32)
    with np.errstate(under="ignore"):
        A = _f32(_f32(rho_r * DR) - RI)
        g_r = _f32(direct + _f32(_f32(ea_r * A) * eb_r))
    g_r = np.where(v_r & (k_eff > 0), g_r, np.float32(0)).astype(np.float32)
    g = np.zeros((B, N, L), np.float32)
    np.put_along_axis(g, orders, g_r, axis=2)
    return g, np.where(k_eff[..., 0] > 0, FR[..., 0], np.float32(0))


# ---- the update launch for this algorithm ------------------------------------------------------------------------------------------
def update_ref(p, g_raw, state, tail, optimizer, lr, max_norm, l2_loss, adam_t=1):
    """One update launch in float64: g = g_raw / D (+ l2_loss p), the clip over the FULL gradient (the project's own algorithm: no
    exhausted-generator quirk), then SGD, Adagrad (eps 1e-10) or Adam (tests/adam_ref.adam64).  Returns a dict: p, state (None for
    SGD), loss, norm (pre-clip), coef, g (what the optimizer got) and g_terms (the magnitudes of its terms, for adam_ref's bars)."""
    from tests import adam_ref as A
    p, g_raw = np.asarray(p, np.float64), np.asarray(g_raw, np.float64)
    D = float(tail[1])
    g, terms = g_raw / D, np.abs(g_raw) / D
    loss = float(tail[0]) / D
    if l2_loss > 0:
        g, terms = g + l2_loss * p, terms + l2_loss * np.abs(p)
        loss += l2_loss * 0.5 * float((p * p).sum())
    norm = float(np.sqrt((g * g).sum()))
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    g, terms = g * coef, terms * coef
    out = dict(loss=loss, norm=norm, coef=coef, g=g, g_terms=terms)
    n = len(p)
    if optimizer == "sgd":
        out.update(p=p - lr * g, state=None)
    elif optimizer == "ada":
        acc = np.asarray(state, np.float64)[:n] + g * g
        out.update(p=p - lr * g / (np.sqrt(acc) + 1e-10), state=acc)
    elif optimizer == "adam":
        st = np.asarray(state, np.float64)
        pn, m, v = A.adam64(p, g, st[:n], st[n:2 * n], adam_t, lr, float(np.float32(A.EPS)))
        out.update(p=pn, state=np.concatenate([m, v]))
    else:
        raise ValueError(optimizer)
    return out
