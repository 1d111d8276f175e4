"""Host twins of the trust-bias click model and of AffineRank, for the tests.

  * decide / click_draw / sessions / click_count / replay: the trust-bias decision of csrc/ultr_click.h (click_decide_tables,
    ULTR_CLICK_TRUST) restated in numpy float32 - p = fl(fl(alpha_k cp) + beta_k), click iff u < p - on the uniforms, the query pick
    and the shuffles of tests/draw_ref.py / tests/propensity_ref.py / tests/online_draw_ref.py (their helpers are imported, their
    loops repeated around the new decision): bit for bit.
  * loss_parts: the law of csrc/ultr_affine.hip in torch float64, gradients from autograd.
  * step_ref: one whole AffineRank step in float64 - the loss twin on given scores, the DNN's gradient by autograd through the
    oracle's DNN where one is given, then the update launch (tests/plrank_ref.update_ref: 1 / D, the L2 term, the clip over the full
    gradient, SGD / Adagrad / Adam), in the manner of tests/twotower_ref.py.

The bars are tests/loss_ref.py's and tests/adam_ref.py's, unchanged; excess() is tests/twotower_ref.excess (loss_ref.terms_excess
with the float32 subnormal floor)."""
import numpy as np
import torch

from tests import draw_ref as D
from tests import loss_ref as R
from tests import philox_ref as P
from tests import propensity_ref as PR
from tests.plrank_ref import update_ref  # the update launch of the project's own learners: 1 / D, L2, the clip over the full gradient
from tests.twotower_ref import excess, live_mask  # noqa: F401  (re-exported for the tests)

TRUST = 3
TAIL_FIXED = R.TAIL_FIXED
f32 = np.float32


# ---- the click decision -----------------------------------------------------------------------------------------------------------
def click_prob_of(y, cprob):
    """cprob[min(max((int)y, 0), n_rel - 1)] as click_prob_of (csrc/ultr_click.h)."""
    cprob = np.asarray(cprob, f32)
    lab = np.where(y > 0, np.trunc(y), 0).astype(np.int64)
    return cprob[np.minimum(lab, len(cprob) - 1)]


def threshold(image, n_exam, cp):
    """p [L, ...] of positions 0 .. L - 1 along axis 0: fl(fl(alpha_k cp) + beta_k), k = min(l, n_exam - 1); image = [alpha | beta]."""
    image = np.asarray(image, f32).reshape(-1)
    assert image.size == 2 * n_exam
    k = np.minimum(np.arange(cp.shape[0]), n_exam - 1)
    shape = (-1,) + (1,) * (cp.ndim - 1)
    prod = (image[k].reshape(shape) * cp.astype(f32)).astype(f32)
    return (prod + image[n_exam + k].reshape(shape)).astype(f32)


def decide(y, u, image, n_exam, cprob):
    """Clicks (float32, the shape of y) of labels y and uniforms u, positions along axis 0."""
    y, u = np.asarray(y, f32), np.asarray(u, f32)
    return (u < threshold(image, n_exam, click_prob_of(y, cprob))).astype(f32)


def click_draw(lists, labels, n_docs, image, n_exam, cprob, seed, step, B, L, max_tries):
    """What ultr_click_batch writes under ULTR_CLICK_TRUST: draw_ref.click_draw's loop around decide().  Returns docids [L, B],
    clicks [L, B], query_idx [B], the attempt kept [B], the kept uniforms and labels [L, B]."""
    lists, labels = np.asarray(lists, np.int32), np.asarray(labels, f32)
    n_queries, lmax = lists.shape
    k = P.key(seed, step)
    docids, clicks = np.zeros((L, B), np.int32), np.zeros((L, B), f32)
    qidx, kept = np.zeros(B, np.int32), np.zeros(B, np.int64)
    u_kept, y_kept = np.zeros((L, B), f32), np.zeros((L, B), f32)
    active = np.arange(B, dtype=np.int64)
    pos = np.arange(L)
    inside = pos < lmax
    for attempt in range(max_tries):
        if active.size == 0:
            break
        n = active.size
        bb, at = active.astype(np.uint64), np.full(n, attempt, np.uint64)
        uq = P.u01(P.philox4x32(bb, at, 0xFFFFFFFF, D.QUERY_TAG, *k)[0])
        q = np.minimum(np.floor(uq.astype(np.float64) * np.float64(n_queries)).astype(np.int64), n_queries - 1)
        d = np.full((L, n), -1, np.int64)
        d[inside] = lists[q][:, pos[inside]].T
        valid = d >= 0
        ids = np.where(valid, d, n_docs).astype(np.int32)
        y = np.zeros((L, n), f32)
        y[inside] = labels[q][:, pos[inside]].T
        y = np.where(valid, y, f32(0))
        u = P.u01(D.click_uniforms(k, bb, at, L))
        ck = decide(y, u, image, n_exam, cprob)
        docids[:, active], clicks[:, active], qidx[active], kept[active] = ids, ck, q, attempt
        u_kept[:, active], y_kept[:, active] = u, y
        active = active[ck.sum(0) == 0]
    return docids, clicks, qidx, kept, u_kept, y_kept


def host_probability(hm, y, L):
    """P(click) [L, ...] of the host TrustBiasModel in float64, from its own three tables (not from the device image)."""
    cp = np.asarray(hm.click_prob, np.float64)
    lab = np.where(y > 0, np.trunc(y), 0).astype(np.int64)
    gamma = cp[np.minimum(lab, len(cp) - 1)]
    k = np.minimum(np.arange(L), len(hm.exam_prob) - 1)
    shape = (-1,) + (1,) * (gamma.ndim - 1)
    ex, tp, tn = (np.asarray(t, np.float64)[k].reshape(shape) for t in (hm.exam_prob, hm.trust_pos, hm.trust_neg))
    return ex * (tn + (tp - tn) * gamma)


def replay(hm, clicks, u, y, margin):
    """The second check: the host model's float64 law on the kernel's uniforms.  Returns the number of draws within `margin` of
    their threshold (left out); asserts agreement on every other draw."""
    p = host_probability(hm, y, u.shape[0])
    u = u.astype(np.float64)
    close = np.abs(u - p) <= margin
    np.testing.assert_array_equal(clicks[~close], (u < p)[~close].astype(f32))
    return int(close.sum())


def sessions_clicks(labels, lengths, image, n_exam, cprob, seed, s):
    """propensity_ref.sessions under ULTR_CLICK_TRUST: (n [S], clicks [lmax, S] bool) of the sessions s."""
    labels, lengths = np.asarray(labels, f32), np.asarray(lengths, np.int64)
    n_queries, lmax = labels.shape
    s = np.asarray(s, np.uint64)
    lo, hi = s & P.MASK, s >> np.uint64(32)
    k = P.key(seed, 0)
    uq = P.u01(P.philox4x32(lo, hi, 0xFFFFFFFF, D.QUERY_TAG, *k)[0])
    q = np.minimum(np.floor(uq.astype(np.float64) * np.float64(n_queries)).astype(np.int64), n_queries - 1)
    n = lengths[q]
    valid = np.arange(lmax)[:, None] < n[None, :]
    keys = np.where(valid, PR._words(k, lo, hi, lmax, PR.SHUFFLE_TAG).astype(np.int64), -1)
    perm = np.argsort(-keys, axis=0, kind="stable")
    y = np.where(valid, labels[q[None, :], perm], f32(0))
    u = P.u01(PR._words(k, lo, hi, lmax, D.CLICK_TAG))
    return n, (decide(y, u, image, n_exam, cprob) > 0) & valid


def click_count(labels, lengths, image, n_exam, cprob, seed, first_session, n_sessions):
    """What ultr_propensity_count adds to a zero table under ULTR_CLICK_TRUST: int64 [lmax, lmax] (row = length - 1, column = position)."""
    lmax = np.asarray(labels).shape[1]
    s = np.arange(n_sessions, dtype=np.uint64) + np.uint64(first_session)
    n, ck = sessions_clicks(labels, lengths, image, n_exam, cprob, seed, s)
    idx = ((n[None, :] - 1) * lmax + np.arange(lmax)[:, None])[ck]
    return np.bincount(idx, minlength=lmax * lmax).reshape(lmax, lmax).astype(np.int64)


def redrawn_clicks(y, uniforms_of_attempt, image, n_exam, cprob, max_redraws):
    """The clicks of one list of labels y [n] as the online kernels draw them: attempts 0 .. max_redraws until one has a click."""
    for attempt in range(1 + max_redraws):
        ck = decide(y, uniforms_of_attempt(attempt), image, n_exam, cprob)
        if ck.sum() > 0:
            break
    return ck, attempt


# ---- the loss ---------------------------------------------------------------------------------------------------------------------
def weights(labels_LB, alpha, beta, live):
    """w [B, L] float64 = (c - beta_k) / alpha_k at the live positions, 0 at a PAD; k = min(l, n - 1); alpha, beta as float32 hold them."""
    c = torch.as_tensor(np.asarray(labels_LB, np.float64)).t()
    a, b = np.asarray(alpha, f32).astype(np.float64), np.asarray(beta, f32).astype(np.float64)
    k = np.minimum(np.arange(c.shape[1]), len(a) - 1)
    w = (c - torch.as_tensor(b[k])) / torch.as_tensor(a[k])
    return torch.where(torch.as_tensor(np.asarray(live)), w, torch.zeros_like(w))


def loss_parts(scores, labels_LB, alpha, beta, docids_LB=None, n_docs=None):
    """What ultr_affine_loss emits, in float64: dict(ds [B, L] (x D), ds_abs, tail [4 + 2 L], tail_abs, loss, live, w, W)."""
    s = torch.as_tensor(np.asarray(scores, np.float64)).clone().requires_grad_(True)
    B, L = s.shape
    live = live_mask(docids_LB, n_docs, B, L)
    w = weights(labels_LB, alpha, beta, live.numpy())
    nls = -torch.log_softmax(s, dim=1)  # the softmax over all L positions: a PAD stays in the denominator
    total = (w * nls).sum()
    total.backward()
    total = total.detach()
    with torch.no_grad():
        p = torch.softmax(s, dim=1)
        W = w.sum(1, keepdim=True)
        ds_abs = (p * W).abs() + w.abs()  # the two terms of  p W - w
        closed = p * W - w
        assert float((closed - s.grad).abs().max()) <= 1e-9 * max(1.0, float(ds_abs.max()))
    tail, tail_abs = np.zeros(TAIL_FIXED + 2 * L), np.zeros(TAIL_FIXED + 2 * L)
    tail[0], tail[1] = float(total), float(B)
    tail_abs[0], tail_abs[1] = float((w * nls).detach().abs().sum()), float(B)
    return dict(ds=s.grad.numpy(), ds_abs=ds_abs.numpy(), tail=tail, tail_abs=tail_abs, loss=float(total) / B, live=live.numpy(),
                w=w.numpy(), W=W.numpy().ravel())


# ---- a whole step -----------------------------------------------------------------------------------------------------------------
def step_ref(p0, state0, scores, labels_LB, alpha, beta, docids_LB, n_docs, mask_padding, g_raw, optimizer, lr, max_norm, l2_loss,
             adam_t, dnn=None, tail=None):
    """One step in float64 from where the device stood: the loss twin on the device's scores (`loss`), the update on the device's
    float32 gradient g_raw and folded step tail (`update`; tail None: the twin's own), and - dnn = (features, F, hidden) - the scores and the gradient of the DNN by autograd through
    the oracle's float64 DNN (`dnn_scores`, `dnn_grad`, the latter for the MEAN over lists)."""
    ref = loss_parts(scores, labels_LB, alpha, beta, docids_LB if mask_padding else None, n_docs)
    out = dict(loss=ref)
    if dnn is not None:
        from oracle import ultr_oracle as O
        feats, F, hidden = dnn
        L, B = np.asarray(docids_LB).shape
        x = O.gather_rows(np.asarray(feats, f32), docids_LB).double()
        p = torch.tensor(np.asarray(p0, np.float64), requires_grad=True)
        s = O.dnn_forward(p, F, hidden, x, "elu").view(L, B).t()
        (s * torch.tensor(ref["ds"] / B)).sum().backward()
        out.update(dnn_scores=s.detach().numpy(), dnn_grad=p.grad.numpy())
    out["update"] = update_ref(p0, g_raw, state0, ref["tail"] if tail is None else tail, optimizer, lr, max_norm, l2_loss, adam_t)
    return out


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
def shipped_model():
    from ultra_pytorch_amd.utils import click_models as CM
    return CM.TrustBiasModel(0.1, 1.0, 4, 1.0)


def image_of(hm):
    """(the float32 [2 n] image alpha | beta, n) as click_models.device_tables builds it, on the host."""
    a, b = hm.affine_parameters(len(hm.exam_prob))
    return np.asarray([a, b], f32).reshape(-1), len(a)
