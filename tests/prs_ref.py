"""PRSrank's loss restated from its definition (prs_rank.py:94-176, 207-251), for the tests.

Per list: ipw[l] = IPW[min(l, len - 1)] for every presentation position, pw = 1 / ipw (0 where ipw == 0); sort by score,
descending (stable: ties keep the presentation order); for the sorted pairs i < j
    prs_ij = ipw_i pw_j,  t_ij = (1 + clamp(y_i - y_j, -1, 1)) / 2,  x_ij = 1 / (exp(-sigma (s_i - s_j)) + 1),
    w_ij = |g_i - g_j| / IDCG * |1/log2(i+2) - 1/log2(j+2)|,  g = 2^y - 1,  IDCG = sum over the WHOLE batch of ideal DCG,
loss = sum prs_ij * BCE(x_ij, t_ij; weight w_ij), BCE with both logs clamped at -100, summed in float64.

`dtype` is the precision of the scores-to-loss chain.  float64 is the default; float32 reproduces the reference's own
arithmetic where it matters - the saturated regime (x rounds to 1 above a gap of ~16.6 / sigma and the gradient explodes,
exp overflows in the lower triangle above ~88.7 / sigma and the gradient is NaN).  x is formed on the full L x L matrix and
the upper triangle selected from it, so autograd meets the overflowed lower-triangle exp exactly as it does there.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ultr_oracle as O


def ipw_of_positions(ipw_list, L):
    ipw = np.asarray([float(ipw_list[min(l, len(ipw_list) - 1)]) for l in range(L)], dtype=np.float64)
    pw = np.where(ipw == 0.0, 0.0, 1.0 / np.where(ipw == 0.0, 1.0, ipw))
    return torch.from_numpy(ipw), torch.from_numpy(pw)


def batch_idcg(labels):
    """sum_b sum_r (2^y - 1) / ln(r + 1) over the labels sorted descending, r 1-based."""
    ideal = torch.sort(labels.double(), dim=1, descending=True)[0]
    r = torch.arange(1, labels.shape[1] + 1, dtype=torch.float64)
    return ((torch.pow(2.0, ideal) - 1.0) / torch.log(r + 1.0)).sum()


def prs_loss(scores, labels, ipw_list, sigma=1.0, dtype=torch.float64):
    """scores [B, L] (may require grad), labels [B, L] -> float64 scalar loss."""
    B, L = scores.shape
    s = scores.to(dtype)
    y = labels.to(dtype)
    ipw, pw = ipw_of_positions(ipw_list, L)
    order = torch.sort(s.detach(), dim=1, descending=True, stable=True)[1]
    ps = torch.gather(s, 1, order)
    ys = torch.gather(y, 1, order)
    ipws = ipw[order]  # [B, L] float64, gathered by presentation position
    pws = pw[order]
    iu = torch.triu_indices(L, L, 1)
    x = 1.0 / (torch.exp(-sigma * (ps[:, :, None] - ps[:, None, :])) + 1.0)
    t = 0.5 * (1.0 + torch.clamp(ys[:, :, None] - ys[:, None, :], -1.0, 1.0))
    idcg = batch_idcg(labels).to(dtype)
    gn = (torch.pow(2.0, ys) - 1.0) / idcg
    disc = 1.0 / torch.log2(torch.arange(L, dtype=dtype) + 2.0)
    w = (gn[:, :, None] - gn[:, None, :]).abs() * (disc[:, None] - disc[None, :]).abs()
    xu, tu, wu = x[:, iu[0], iu[1]], t[:, iu[0], iu[1]], w[:, iu[0], iu[1]]
    prs = ipws[:, iu[0]] * pws[:, iu[1]]
    bce = F.binary_cross_entropy(xu, tu, wu, reduction="none")  # logs clamped at -100
    return (bce.double() * prs).sum()


def prs_score_grad(scores, labels, ipw_list, sigma=1.0, dtype=torch.float64):
    """(loss, d loss / d scores [B, L] as numpy float64)."""
    s = torch.as_tensor(np.asarray(scores), dtype=dtype).clone().requires_grad_(True)
    lab = torch.as_tensor(np.asarray(labels), dtype=dtype)
    loss = prs_loss(s, lab, ipw_list, sigma, dtype)
    (g,) = torch.autograd.grad(loss, s)
    return float(loss.detach()), g.double().numpy()


def prs_step(params, state_sum, forward, labels_LB, ipw_list, lr=0.05, max_norm=5.0, sigma=1.0, strategy="ada"):
    """One PRSrank training step on the CPU: forward(p) -> scores [B, L] (the oracle's DNN or SetRank forward, float32),
    the float64 loss, autograd, clip_grad_norm_ + Adagrad / SGD (oracle.apply_update)."""
    p = torch.as_tensor(np.asarray(params), dtype=torch.float32).clone().requires_grad_(True)
    scores = forward(p)
    labels = torch.from_numpy(np.ascontiguousarray(np.transpose(labels_LB))).float()
    loss = prs_loss(scores, labels, ipw_list, sigma)
    (g,) = torch.autograd.grad(loss, p)
    with torch.no_grad():
        p2, s2, n, _ = O.apply_update(p.detach(), g, torch.as_tensor(np.asarray(state_sum), dtype=torch.float32), lr, max_norm,
                                      strategy)
    return dict(loss=float(loss.detach()), scores=scores.detach().numpy(), grads=g.numpy(), norm=float(n), params=p2.numpy(),
                state=s2.numpy())


def dnn_forward(F_, hidden, features, docids, act="elu"):
    return lambda p: O.ranking_scores(p, F_, hidden or [], features, docids, act)


def setrank_forward(cfg, features, docids):
    return lambda p: O.setrank_forward(p, *cfg, features, docids)


def setrank_cfg(m):
    """(feature_size, d_model, num_heads, num_layers, dff) of a fixture's SetRank model."""
    shapes = dict(zip(m["param_keys"], m["param_shapes"]))
    dff, F_ = shapes["Encoder_layer.input_embedding.0.weight"]
    d_model = shapes["Encoder_layer.input_embedding.2.weight"][0]
    n_layers = sum(1 for k in m["param_keys"] if k.endswith("mha.dense.weight"))
    heads = int(dict(kv.split("=") for kv in m["model_hparams"].split(",") if kv)["num_heads"])
    return (F_, d_model, heads, n_layers, dff)


def fixture_step(d, m, t):
    """prs_step on step t of a prs_* fixture."""
    p = "s%d_" % t
    if m["model"] == "SetRank":
        fwd = setrank_forward(setrank_cfg(m), d[p + "features"], d[p + "docids"])
    else:
        fwd = dnn_forward(m["F"], m["hidden"], d[p + "features"], d[p + "docids"])
    return prs_step(d[p + "pre_params"], d[p + "pre_adagrad"], fwd, d[p + "labels"], d["ipw_list"], lr=m["lr"],
                    max_norm=m["max_gradient_norm"], sigma=m["sigma"], strategy=m["grad_strategy"])
