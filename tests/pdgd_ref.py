"""PDGD's pair weights, loss and score gradient restated from the definition (pdgd.py:107-205), for the tests.

Per list b over its M scored positions (scores s fp32, labels y, valid = docid != n_docs):
    e_j = exp(tau (s_j - max s)) in float32 (as the reference and the kernel form it; it decides which terms underflow), 0 for a
          PAD at j < cutoff only;  D_p = sum_{q >= p} e_q  (float64 from here on)
    pairs (l, k): l < cutoff valid with y_l > 0, k in 0 .. l+1, k < cutoff valid with y_k < y_l - in the reference's order:
          l descending, k ascending
    w = 1 / (1 + exp(min(delta, 20))), delta = sum over the flipped list's log suffix sums minus the original's (terms of a zero
          suffix sum count 0); only p in (min(k,l), max(k,l)] differ
    loss = sum_pairs -w e^{s_l} / (e^{s_l} + e^{s_k})  on the raw scores, d loss / d s by autograd (w constant).
`delta_bruteforce` is the reference's formula itself: the full flipped cumsum, all M positions.
"""
import numpy as np
import torch

from oracle import ultr_oracle as O


def exp_scores(s, valid, cutoff, tau):
    s = np.asarray(s, dtype=np.float32)
    e = np.exp(np.float32(tau) * (s - np.max(s))).astype(np.float32)
    for j in range(min(cutoff, len(s))):
        if not valid[j]:
            e[j] = 0.0
    return e.astype(np.float64)


def _lg(x):
    return np.log(x, out=np.zeros_like(x), where=x > 0)


def delta_local(e, a, b):
    """Only the suffix sums in (a, b] differ.  The flipped ones are summed from the end as the reference's cumsum sums them:
    F_b = D_{b+1} + e_a, F_p = F_{p+1} + e_p (subtracting e_b from D_p instead cancels catastrophically where e_b dominates)."""
    D = np.cumsum(e[::-1])[::-1]
    f = D[b + 1] if b + 1 < len(e) else 0.0
    f += e[a]
    delta = 0.0
    for p in range(b, a, -1):
        if p < b:
            f += e[p]
        delta += float(_lg(np.array([f]))[0] - _lg(np.array([D[p]]))[0])
    return delta


def delta_bruteforce(e, k, l):
    D = np.cumsum(e[::-1])[::-1]
    f = e.copy()
    f[k], f[l] = e[l], e[k]
    F = np.cumsum(f[::-1])[::-1]
    return float(np.sum(_lg(F)) - np.sum(_lg(D)))


def list_pairs(s, y, valid, cutoff, tau, brute=False):
    """[(l, k, w)] of one list in the reference's order."""
    M = len(s)
    c = min(cutoff, M)
    e = exp_scores(s, valid, c, tau)
    out = []
    for l in range(c - 1, -1, -1):
        if not valid[l] or not y[l] > 0:
            continue
        for k in range(l + 2):
            if k < c and y[k] < y[l] and valid[k]:
                delta = delta_bruteforce(e, k, l) if brute else delta_local(e, min(k, l), max(k, l))
                out.append((l, k, 1.0 / (1.0 + np.exp(min(delta, 20.0)))))
    return out


def batch_pairs(scores_BM, labels_MB, docids_MB, n_docs, cutoff, tau, brute=False):
    """[(b, l, k, w)] over the batch; scores [B, M], labels / docids position-major [M, B]."""
    scores_BM = np.asarray(scores_BM, dtype=np.float32)
    y = np.asarray(labels_MB, dtype=np.float64).T
    valid = np.asarray(docids_MB).T != n_docs
    out = []
    for b in range(scores_BM.shape[0]):
        out += [(b, l, k, w) for (l, k, w) in list_pairs(scores_BM[b], y[b], valid[b], cutoff, tau, brute)]
    return out


def pair_loss(scores, pairs, dtype=torch.float64):
    """scores [B, M] tensor (may require grad) -> the weighted pair loss."""
    if not pairs:
        return scores.sum() * 0.0
    idx = torch.tensor([(b, l, k) for (b, l, k, _) in pairs], dtype=torch.int64)
    w = torch.tensor([p[3] for p in pairs], dtype=dtype)
    s = scores.to(dtype)
    sl, sk = s[idx[:, 0], idx[:, 1]], s[idx[:, 0], idx[:, 2]]
    return torch.sum(-torch.exp(sl) / (torch.exp(sl) + torch.exp(sk)) * w)


def pdgd_score_grad(scores_BM, labels_MB, docids_MB, n_docs, cutoff, tau, dtype=torch.float64):
    """(loss, d loss / d scores [B, M] float64, pairs)."""
    pairs = batch_pairs(scores_BM, labels_MB, docids_MB, n_docs, cutoff, tau)
    s = torch.as_tensor(np.asarray(scores_BM), dtype=dtype).clone().requires_grad_(True)
    loss = pair_loss(s, pairs, dtype)
    (g,) = torch.autograd.grad(loss, s)
    return float(loss.detach()), g.double().numpy(), pairs


def pdgd_step(params, state_sum, F_, hidden, features, docids_MB, labels_MB, cutoff, tau, lr, max_norm, l2_loss, strategy):
    """One PDGD step on the CPU: the oracle's DNN / Linear forward (float32), the pair loss (float64) + l2_loss * sum p^2 / 2,
    autograd, clip_grad_norm_ over ALL parameters (PDGD clips with l2_loss > 0 too) + Adagrad / SGD (oracle.apply_update)."""
    p = torch.as_tensor(np.asarray(params), dtype=torch.float32).clone().requires_grad_(True)
    scores = O.ranking_scores(p, F_, hidden or [], features, docids_MB, "elu")
    n_docs = np.asarray(features).shape[0]
    pairs = batch_pairs(scores.detach().numpy(), labels_MB, docids_MB, n_docs, cutoff, tau)
    loss = pair_loss(scores, pairs)
    if l2_loss > 0:
        loss = loss + l2_loss * torch.sum(p.double() ** 2) / 2
    (g,) = torch.autograd.grad(loss, p)
    with torch.no_grad():
        p2, s2, n, _ = O.apply_update(p.detach(), g.float(), torch.as_tensor(np.asarray(state_sum), dtype=torch.float32), lr,
                                      max_norm, strategy)
    return dict(loss=float(loss.detach()), scores=scores.detach().numpy(), grads=g.float().numpy(), norm=float(n),
                params=p2.numpy(), state=s2.numpy(), pairs=pairs)
