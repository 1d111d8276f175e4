"""A torch float64 restatement of SetRank's forward and the list-wise softmax cross entropy with autograd - the reference of the
streaming attention backward (csrc/ultr_sr_attn_long.hip) - and a numpy float64 restatement of that kernel's tiled two-role walk for one
(list, head) slice.  Parameter layout: oracle.ultr_oracle.setrank_layout.  Not a test module: tests/test_sr_attn_bwd_long_cpu.py proves
it against tests/sr_attn_long_ref.py, the fp32 oracle and direct autograd; tests/test_gpu_setrank_long_train.py measures the kernels
against it."""
import math

import numpy as np
import torch


def gather(features, docids):
    """x [B, L, F] float64: row docids[l, b] of features, the zero row for a PAD (id == n_docs)."""
    feats = np.asarray(features, dtype=np.float64).reshape(-1, np.shape(features)[-1])
    table = np.concatenate((feats, np.zeros((1, feats.shape[1]))), axis=0)
    L, B = np.shape(docids)
    x = table[np.asarray(docids, np.int64).reshape(-1)].reshape(L, B, -1)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2)))


def setrank_forward(params, F, d, H, nl, dff, features, docids, detach_probabilities=False):
    """scores [B, L] (torch float64, differentiable in `params`): oracle.setrank_forward operation for operation, every number a
    float64 - the root of the head depth included.  detach_probabilities: the softmax output is a constant of the graph, so a gradient
    taken through these scores lacks the logit path (dS = P (dP - t) / sqrt(dh) and the dq + dk chain behind it); the scores are the same."""
    from oracle import ultr_oracle as O
    params = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, np.float64))
    W = {n: params[o:o + int(np.prod(sh))].reshape(sh) for n, sh, o in O.setrank_layout(F, d, nl, dff)}
    ln = torch.nn.functional.layer_norm
    x = gather(features, docids)
    B, L = x.shape[0], x.shape[1]
    e = "Encoder_layer."
    x = ln(x, (F,), W[e + "input_layer_norm.weight"], W[e + "input_layer_norm.bias"], 1e-6)
    x = torch.relu(x @ W[e + "input_embedding.0.weight"].T + W[e + "input_embedding.0.bias"])
    x = x @ W[e + "input_embedding.2.weight"].T + W[e + "input_embedding.2.bias"]
    depth = d // H
    for i in range(nl):
        l = e + "enc_layers.encoder%d." % i
        q = x.reshape(B, L, H, depth).permute(0, 2, 1, 3)
        prob = torch.softmax((q @ q.transpose(-1, -2)) / math.sqrt(depth), dim=-1)
        att = (prob.detach() if detach_probabilities else prob) @ q
        att = att.permute(0, 2, 1, 3).reshape(B, L, d)
        o = att @ W[l + "mha.dense.weight"].T + W[l + "mha.dense.bias"]
        out1 = ln(x + o, (d,), W[l + "layernorm1.weight"], W[l + "layernorm1.bias"], 1e-6)
        f = torch.relu(out1 @ W[l + "ffn.0.weight"].T + W[l + "ffn.0.bias"])
        f = f @ W[l + "ffn.2.weight"].T + W[l + "ffn.2.bias"]
        x = ln(out1 + f, (d,), W[l + "layernorm2.weight"], W[l + "layernorm2.bias"], 1e-6)
    o = torch.relu(x @ W[e + "output_layer.0.weight"].T + W[e + "output_layer.0.bias"])
    o = o @ W[e + "output_layer.2.weight"].T + W[e + "output_layer.2.bias"]
    return o[..., 0]


def softmax_loss(scores, labels, pw=None):
    """oracle.softmax_loss: the 1e-7 label smoothing, the GLOBAL normaliser."""
    w = (labels + 0.0000001) * (torch.ones_like(labels) if pw is None else pw)
    dis = torch.nan_to_num(w / torch.sum(w, 1, keepdim=True))
    loss = torch.sum(-dis * torch.nn.functional.log_softmax(scores, -1), -1) * torch.sum(w, 1)
    return torch.sum(loss) / torch.sum(w)


def train_step(params, cfg, features, docids, labels_LB, ipw_list=None, detach_probabilities=False):
    """Scores, loss and gradient of one NA (ipw_list None) / IPW step: dict(scores [B, L], loss, grads [P]) in float64.  The
    propensity weights are the float32 numbers IPWrank builds (oracle.ipw_weights), widened.  detach_probabilities: the gradient without
    the logit path of every attention (setrank_forward); the difference to the default gradient is that path's contribution."""
    from oracle import ultr_oracle as O
    p = torch.as_tensor(np.asarray(params), dtype=torch.float64).clone().requires_grad_(True)
    scores = setrank_forward(p, *cfg, features, docids, detach_probabilities=detach_probabilities)
    labels = torch.from_numpy(np.ascontiguousarray(np.transpose(labels_LB))).double()
    pw = None if ipw_list is None else O.ipw_weights(labels_LB, ipw_list).double()
    loss = softmax_loss(scores, labels, pw)
    (g,) = torch.autograd.grad(loss, p)
    return dict(scores=scores.detach().numpy(), loss=float(loss.detach()), grads=g.numpy())


# ---- one (list, head) slice -------------------------------------------------------------------------------------------------------------
def attention_backward_autograd(x, dA):
    """dx of A = softmax(x x^T / sqrt(dh)) x for the upstream gradient dA, by autograd in float64: x, dA [L, dh] -> dx [L, dh]."""
    xt = torch.as_tensor(np.asarray(x, np.float64)).clone().requires_grad_(True)
    A = torch.softmax((xt @ xt.T) / math.sqrt(xt.shape[1]), dim=-1) @ xt
    (g,) = torch.autograd.grad(A, xt, torch.as_tensor(np.asarray(dA, np.float64)))
    return g.numpy()


def attention_backward_tiled(x, dA, tile=128, own=16):
    """The streaming kernel's walk in float64.  The forward leaves lse (P_ij = exp(scale S_ij - lse_i)) and A; a pre-pass forms
    t_i = dA_i . A_i.  Then every block of `own` tokens meets the whole list as partner tiles of `tile` rows, staged whole: rows past
    L are zero rows with lse = +inf (a padding QUERY has P = 0 by itself) and t = 0; padding KEYS are masked where the own token is the
    query.  Own rows past L (the last own block) carry lse = +inf too and are not written.  Per tile, with the own block in both roles:
        S = x_partner x_own^T (symmetric: one tile serves both roles),  dP^T = x_partner dA_own^T,  dP = dA_partner x_own^T,
        Pa = exp(scale S - lse_own) (own as query), Pb = exp(scale S - lse_partner) (own as key),
        dx_own += scale (Pa (dP^T - t_own) + Pb (dP - t_partner))^T x_partner  +  Pb^T dA_partner
    - dq + dk in one chain, dv in another, summed at the end."""
    x, dA = np.asarray(x, np.float64), np.asarray(dA, np.float64)
    L, dh = x.shape
    scale = 1.0 / np.sqrt(float(dh))
    s = (x @ x.T) * scale
    mx = s.max(axis=1, keepdims=True)
    e = np.exp(s - mx)
    den = e.sum(axis=1, keepdims=True)
    A, lse = (e / den) @ x, (mx + np.log(den))[:, 0]
    t = (dA * A).sum(axis=1)
    dx = np.zeros_like(x)

    def staged(a, r0, n, fill=0.0):
        out = np.full((n,) + a.shape[1:], fill, dtype=np.float64)
        m = max(0, min(n, L - r0))
        out[:m] = a[r0:r0 + m]
        return out

    for q0 in range(0, L, own):
        xo, go = staged(x, q0, own), staged(dA, q0, own)
        lo, to = staged(lse, q0, own, np.inf), staged(t, q0, own)
        acc, acv = np.zeros((own, dh)), np.zeros((own, dh))
        for k0 in range(0, L, tile):
            xp, gp = staged(x, k0, tile), staged(dA, k0, tile)
            lp, tp = staged(lse, k0, tile, np.inf), staged(t, k0, tile)
            S = xp @ xo.T                               # [partner, own]
            dpt, dpn = xp @ go.T, gp @ xo.T
            pa = np.exp(scale * S - lo[None, :])        # exp(-inf) = 0 for a padding own row ...
            pb = np.exp(scale * S - lp[:, None])        # ... and for a padding partner as query
            pa[np.arange(tile) + k0 >= L, :] = 0.0      # padding keys: only the last tile has any
            acc += (scale * (pa * (dpt - to[None, :]) + pb * (dpn - tp[:, None]))).T @ xp
            acv += pb.T @ gp
        n = min(own, L - q0)
        dx[q0:q0 + n] = (acc + acv)[:n]
    return dx
