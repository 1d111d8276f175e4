"""A float64 restatement of the DNN (plain numpy): the forward and the closed-form backward of oracle.ultr_oracle.dnn_forward /
dnn_backward_manual, the NA / IPW softmax loss in closed form, and what a test needs around them.

    forward(params, F, hidden, x, act)            scores [N], every hidden pre-activation z_j [N, M_j] and the scale
                                                   S_j = |b| + sum_k |u_k| |W_mk| its fp32 evaluation errs in proportion to
    backward(params, F, hidden, x, dscore, act)   the flat gradient and, per entry, the sum of |terms| the entry is a sum of
                                                   (what dnn_backward_manual(abs_terms=True) returns)
    softmax_loss(scores, labels, pw)              loss, d(loss)/d(scores), the normaliser D
    central_differences(...)                      the gradient of sum(dscore * scores) by float64 central differences
    condition_relu(...)                           redraw the feature rows whose ReLU pre-activations sit within fp32 rounding of 0

Parameters are the flat vector in the reference's order (per layer: LayerNorm weight, LayerNorm bias, Linear weight [M, K], Linear
bias); rows of x are documents.  Everything is computed in float64 from the float32 inputs as they are, so it is the exact value of
the function the kernels evaluate up to ~1e-15 - the GPU bars (1e-5) and the fp32 oracle's own error are both measured against it."""
import numpy as np

LN_EPS = 1e-5  # nn.LayerNorm's default (oracle.ultr_oracle.LN_EPS)
ACTS = ("elu", "relu", "tanh", "sigmoid")
f8 = np.float64


def layer_dims(F, hidden):
    dims, k = [], int(F)
    for m in list(hidden) + [1]:
        dims.append((k, int(m)))
        k = int(m)
    return dims


def layout(F, hidden):
    """[(offset of ln.weight, ln.bias, linear.weight, linear.bias)] per layer, and the parameter count."""
    out, off = [], 0
    for k, m in layer_dims(F, hidden):
        out.append((off, off + k, off + 2 * k, off + 2 * k + m * k))
        off += 2 * k + m * k + m
    return out, off


def _split(params, F, hidden):
    params = np.asarray(params, f8)
    lay, P = layout(F, hidden)
    assert params.shape == (P,), (params.shape, P)
    out = []
    for (og, ob, ow, obias), (k, m) in zip(lay, layer_dims(F, hidden)):
        out.append((params[og:og + k], params[ob:ob + k], params[ow:ow + m * k].reshape(m, k), params[obias:obias + m]))
    return out


def _activate(z, act):
    if act == "elu":
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))
    if act == "relu":
        return np.maximum(z, 0)
    if act == "tanh":
        return np.tanh(z)
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    raise ValueError(act)


def _dact(a, act):
    """The activation's derivative from its OUTPUT a (what the kernels keep)."""
    if act == "elu":
        return np.where(a > 0, 1.0, a + 1.0)
    if act == "relu":
        return (a > 0).astype(f8)
    if act == "tanh":
        return 1.0 - a * a
    return a * (1.0 - a)


def forward(params, F, hidden, x, act="elu"):
    """dict(scores [N], z: [z_j [N, M_j]] and S: [S_j [N, M_j]] for the hidden layers j, and the walk's intermediates)."""
    assert act in ACTS
    h = np.asarray(x, f8)
    xs, xhats, rstds, us, zs, Ss = [], [], [], [], [], []
    layers = _split(params, F, hidden)
    for j, (g, b, W, bias) in enumerate(layers):
        mu = h.mean(axis=1, keepdims=True)
        r = 1.0 / np.sqrt(((h - mu) ** 2).mean(axis=1, keepdims=True) + LN_EPS)
        xhat = (h - mu) * r
        u = xhat * g + b
        z = u @ W.T + bias
        xs.append(h), xhats.append(xhat), rstds.append(r), us.append(u)
        if j != len(layers) - 1:
            zs.append(z)
            Ss.append(np.abs(u) @ np.abs(W).T + np.abs(bias))
            h = _activate(z, act)
    return dict(scores=z.reshape(-1), z=zs, S=Ss, xs=xs, xhats=xhats, rstds=rstds, us=us)


def backward(params, F, hidden, x, dscore, act="elu", fwd=None):
    """(grads [P], terms [P]) of sum(dscore * scores): the closed-form backward, and per entry the sum of the absolute values of
    the per-row terms it sums (|dz|^T |u| for a weight, sum |dz| for a bias, sum |du xhat| / sum |du| for the LayerNorm pair)."""
    fw = forward(params, F, hidden, x, act) if fwd is None else fwd
    layers = _split(params, F, hidden)
    lay, P = layout(F, hidden)
    grads, terms = np.zeros(P, f8), np.zeros(P, f8)
    dz = np.asarray(dscore, f8).reshape(-1, 1)
    for j in reversed(range(len(layers))):
        g, _, W, _ = layers[j]
        og, ob, ow, obias = lay[j]
        k, m = W.shape[1], W.shape[0]
        u, xhat = fw["us"][j], fw["xhats"][j]
        grads[ow:ow + m * k] = (dz.T @ u).reshape(-1)
        terms[ow:ow + m * k] = (np.abs(dz).T @ np.abs(u)).reshape(-1)
        grads[obias:obias + m] = dz.sum(axis=0)
        terms[obias:obias + m] = np.abs(dz).sum(axis=0)
        du = dz @ W
        grads[og:og + k] = (du * xhat).sum(axis=0)
        terms[og:og + k] = np.abs(du * xhat).sum(axis=0)
        grads[ob:ob + k] = du.sum(axis=0)
        terms[ob:ob + k] = np.abs(du).sum(axis=0)
        if j == 0:
            break
        dxhat = du * g
        dx = fw["rstds"][j] * (dxhat - dxhat.mean(axis=1, keepdims=True) - xhat * (dxhat * xhat).mean(axis=1, keepdims=True))
        dz = dx * _dact(fw["xs"][j], act)
    return grads, terms


def gather(features, docids):
    """Rows of the position-major batch: row l * B + b = features[docids[l, b]], the zero PAD row for an id outside [0, n_docs)."""
    feats = np.asarray(features, f8)
    ids = np.asarray(docids).astype(np.int64).reshape(-1)
    table = np.concatenate((feats, np.zeros((1, feats.shape[1]), f8)), axis=0)
    return table[np.where((ids >= 0) & (ids < feats.shape[0]), ids, feats.shape[0])]


def scores_BL(scores, B, L):
    return np.asarray(scores).reshape(L, B).T


def softmax_loss(scores, labels, pw=None):
    """The NA / IPW loss of scores [B, L] (base_algorithm.py:309-330 in closed form): w = (y + 1e-7) pw, S_b = sum_l w, D = sum w,
    loss = -sum w log_softmax(s) / D, d(loss)/d(s) = (softmax(s) S_b - w) / D.  Returns (loss, dscores [B, L], D).  The 1e-7 is the
    reference's fp32 constant, and w is formed in fp32 as every implementation forms it (labels + 1e-7 rounds for labels >= 1)."""
    s = np.asarray(scores, f8)
    y = np.asarray(labels, np.float32)
    w32 = (y + np.float32(0.0000001)) * (np.ones_like(y) if pw is None else np.asarray(pw, np.float32))
    w = w32.astype(f8)
    Sb = w.sum(axis=1, keepdims=True)
    D = w.sum()
    sm = s - s.max(axis=1, keepdims=True)
    lsm = sm - np.log(np.exp(sm).sum(axis=1, keepdims=True))
    return float(-(w * lsm).sum() / D), (np.exp(lsm) * Sb - w) / D, float(D)


def ipw_weights(labels_LB, ipw_table):
    """pw [B, L] = ipw_table[min(l, n - 1)] where labels[l, b] > 0, else 0 (ipw_rank.py:115-138)."""
    L = labels_LB.shape[0]
    t = np.asarray(ipw_table, np.float32)
    table = t[np.minimum(np.arange(L), len(t) - 1)]
    return np.where(np.asarray(labels_LB).T > 0, table[None, :], np.float32(0)).astype(np.float32)


def central_differences(params, F, hidden, x, dscore, act="elu", h=1e-6):
    """d sum(dscore * scores) / d params by float64 central differences, one parameter at a time (tiny nets only)."""
    p = np.asarray(params, f8).copy()
    w = np.asarray(dscore, f8).reshape(-1)
    out = np.zeros_like(p)
    for i in range(p.size):
        keep = p[i]
        p[i] = keep + h
        up = float(w @ forward(p, F, hidden, x, act)["scores"])
        p[i] = keep - h
        dn = float(w @ forward(p, F, hidden, x, act)["scores"])
        p[i] = keep
        out[i] = (up - dn) / (2 * h)
    return out


def relu_margin(K):
    """|z| <= relu_margin(K_j) S is "within fp32 rounding of zero".  An fp32 sum of K_j products errs by at most K_j 2^-24 S.  The
    bound is doubled, for the rounding of u itself, and 16 units of 2^-23 S are added, which cover the 22-bit split-half operands
    (at most 2^-21 S = 4 x 2^-23 S): (K_j + 16) 2^-23 S."""
    return (K + 16) * 2.0 ** -23


def near_zero_rows(params, F, hidden, x, act="relu"):
    """bool [N]: the rows with some hidden unit |z| <= relu_margin(K_j) S."""
    fw = forward(params, F, hidden, x, act)
    bad = np.zeros(np.asarray(x).shape[0], bool)
    for (k, _), z, S in zip(layer_dims(F, hidden), fw["z"], fw["S"]):
        bad |= (np.abs(z) <= relu_margin(k) * S).any(axis=1)
    return bad


def condition_relu(rng, params, F, hidden, features, docids, max_rounds=30):
    """Redraw (uniform(-1, 1), as synthetic.make_batch draws) the feature row of every document that gives some hidden unit a
    pre-activation within relu_margin of zero, until none is left (at most max_rounds rounds).  The PAD row is all zeros and cannot
    be redrawn: when IT is flagged, the first LayerNorm's bias - all the network sees of a PAD - is redrawn instead (params is
    returned as a fresh array then) and every row is looked at again.
    Returns (features, params, share of the documents redrawn at least once).  Raises AssertionError if rows are left."""
    feats = np.array(features, np.float32, copy=True)
    params = np.array(params, np.float32, copy=True)
    n_docs = feats.shape[0]
    ids = np.asarray(docids).astype(np.int64).reshape(-1)
    has_pad = bool(((ids < 0) | (ids >= n_docs)).any())
    todo = np.arange(n_docs)  # documents to look at
    redrawn = np.zeros(n_docs, bool)
    check_pad = has_pad
    for _ in range(max_rounds):
        if check_pad and near_zero_rows(params, F, hidden, np.zeros((1, F)), "relu")[0]:
            params[F:2 * F] += rng.normal(scale=0.2, size=F).astype(np.float32)
            todo, check_pad = np.arange(n_docs), True
            continue
        check_pad = False
        bad = todo[near_zero_rows(params, F, hidden, feats[todo], "relu")] if todo.size else todo
        if bad.size == 0:
            break
        feats[bad] = rng.uniform(-1.0, 1.0, size=(bad.size, F)).astype(np.float32)
        redrawn[bad] = True
        todo = bad
    left = int(near_zero_rows(params, F, hidden, gather(feats, docids), "relu").sum())
    assert left == 0, "%d rows still have a ReLU pre-activation within fp32 rounding of zero after %d rounds" % (left, max_rounds)
    return feats, params, float(redrawn.mean()) if n_docs else 0.0
