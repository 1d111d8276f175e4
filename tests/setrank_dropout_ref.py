"""Host restatement of SetRank's dropout: the mask law of csrc/ultr_sr_dropout.h on tests/philox_ref, and a float64
torch-autograd SetRank (the reference's Encoder / EncoderLayer forward, SetRank.py:106-117, 143-153) that multiplies by explicit
masks at the 1 + 2 * num_layers sites.  Written from the law and the model's equations; no reference text."""
import numpy as np
import torch

from tests import philox_ref as P

SR_DROPOUT_TAG = 0x5352444F  # csrc/ultr_sr_dropout.h


def scale_of(rate):
    """1.0f / (1.0f - rate), formed once in float32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))


def keep(seed, step, stream, site, B, L, d, rate):
    """keep[b, l, c] (bool): word c & 3 of Philox(key(seed, step); t = l * B + b, (stream << 8) | site, c >> 2, TAG), u01(word) >= rate."""
    k0, k1 = P.key(seed, step)
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    l = np.arange(L, dtype=np.uint64)[None, :, None]
    q = np.arange((d + 3) // 4, dtype=np.uint64)[None, None, :]
    words = P.philox4x32(l * np.uint64(B) + b, (int(stream) << 8) | int(site), q, SR_DROPOUT_TAG, k0, k1)
    u = np.stack([P.u01(w) for w in words], axis=-1).reshape(B, L, -1)[:, :, :d]
    return u >= np.float32(rate)


def mask(seed, step, stream, site, B, L, d, rate):
    """The multiplier [B, L, d] in float32: scale where kept, 0 where dropped."""
    return np.where(keep(seed, step, stream, site, B, L, d, rate), scale_of(rate), np.float32(0.0)).astype(np.float32)


def masks(seed, step, stream, B, L, d, num_layers, rate):
    """The 1 + 2 * num_layers multipliers of one training forward, by site; None at rate 0."""
    if float(rate) == 0.0:
        return None
    return [mask(seed, step, stream, s, B, L, d, rate) for s in range(1 + 2 * num_layers)]


def layout(F, d, nl, dff):
    """[(state_dict key, shape, offset)] of the flat parameter vector (Encoder_layer.* in registration order)."""
    out, off = [], 0

    def add(name, shape):
        nonlocal off
        out.append((name, tuple(shape), off))
        off += int(np.prod(shape))

    e = "Encoder_layer."
    add(e + "input_layer_norm.weight", (F,)); add(e + "input_layer_norm.bias", (F,))
    add(e + "input_embedding.0.weight", (dff, F)); add(e + "input_embedding.0.bias", (dff,))
    add(e + "input_embedding.2.weight", (d, dff)); add(e + "input_embedding.2.bias", (d,))
    add(e + "output_layer.0.weight", (dff, d)); add(e + "output_layer.0.bias", (dff,))
    add(e + "output_layer.2.weight", (1, dff)); add(e + "output_layer.2.bias", (1,))
    for i in range(nl):
        l = e + "enc_layers.encoder%d." % i
        add(l + "mha.dense.weight", (d, d)); add(l + "mha.dense.bias", (d,))
        add(l + "ffn.0.weight", (dff, d)); add(l + "ffn.0.bias", (dff,))
        add(l + "ffn.2.weight", (d, dff)); add(l + "ffn.2.bias", (d,))
        add(l + "layernorm1.weight", (d,)); add(l + "layernorm1.bias", (d,))
        add(l + "layernorm2.weight", (d,)); add(l + "layernorm2.bias", (d,))
    return out


def gather(features, docids):
    """x [B, L, F] float64: row docids[l, b] of features, the zero row for a PAD (id == n_docs)."""
    feats = np.asarray(features, dtype=np.float32).reshape(-1, np.shape(features)[-1])
    table = np.concatenate((feats, np.zeros((1, feats.shape[1]), np.float32)), axis=0)
    L, B = np.shape(docids)
    x = np.take(table, np.asarray(docids).astype(np.int64).reshape(-1), axis=0).reshape(L, B, -1)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).double()


def forward(params, cfg, x, drop=None):
    """scores [B, L] (float64) of x [B, L, F]; drop: None or the list of multipliers by site (masks())."""
    F, d, H, nl, dff = cfg
    W = {n: params[o:o + int(np.prod(sh))].reshape(sh) for n, sh, o in layout(F, d, nl, dff)}
    ln = torch.nn.functional.layer_norm
    B, L = x.shape[0], x.shape[1]

    def D(v, site):
        return v if drop is None else v * torch.from_numpy(np.asarray(drop[site])).double()

    e = "Encoder_layer."
    x = ln(x, (F,), W[e + "input_layer_norm.weight"], W[e + "input_layer_norm.bias"], 1e-6)
    x = torch.relu(x @ W[e + "input_embedding.0.weight"].T + W[e + "input_embedding.0.bias"])
    x = D(x @ W[e + "input_embedding.2.weight"].T + W[e + "input_embedding.2.bias"], 0)
    depth = d // H
    root = torch.sqrt(torch.tensor(float(depth)))  # float32, as the reference forms it (SetRank.py:181-182)
    for i in range(nl):
        l = e + "enc_layers.encoder%d." % i
        q = x.reshape(B, L, H, depth).permute(0, 2, 1, 3)
        att = torch.softmax((q @ q.transpose(-1, -2)) / root, dim=-1) @ q
        att = att.permute(0, 2, 1, 3).reshape(B, L, d)
        o = D(att @ W[l + "mha.dense.weight"].T + W[l + "mha.dense.bias"], 1 + 2 * i)
        out1 = ln(x + o, (d,), W[l + "layernorm1.weight"], W[l + "layernorm1.bias"], 1e-6)
        f = torch.relu(out1 @ W[l + "ffn.0.weight"].T + W[l + "ffn.0.bias"])
        f = D(f @ W[l + "ffn.2.weight"].T + W[l + "ffn.2.bias"], 2 + 2 * i)
        x = ln(out1 + f, (d,), W[l + "layernorm2.weight"], W[l + "layernorm2.bias"], 1e-6)
    o = torch.relu(x @ W[e + "output_layer.0.weight"].T + W[e + "output_layer.0.bias"])
    o = o @ W[e + "output_layer.2.weight"].T + W[e + "output_layer.2.bias"]
    return o[..., 0]


def ipw_weights(labels_LB, ipw_list):
    """pw [B, L]: the table's entry (its last beyond its end) at clicked positions, in float32 as IPWrank builds them."""
    L, B = np.shape(labels_LB)
    table = np.asarray([ipw_list[l] if l < len(ipw_list) else ipw_list[-1] for l in range(L)], dtype=np.float64)
    pw = np.where(np.asarray(labels_LB).T > 0, table[None, :], 0.0)
    return torch.as_tensor(pw.tolist()).double()


def softmax_loss(scores, labels, pw=None):
    """The list-wise softmax cross entropy with the 1e-7 label smoothing and the GLOBAL normaliser."""
    w = (labels + 0.0000001) * (torch.ones_like(labels) if pw is None else pw)
    dis = torch.nan_to_num(w / torch.sum(w, 1, keepdim=True))
    loss = torch.sum(-dis * torch.nn.functional.log_softmax(scores, -1), -1) * torch.sum(w, 1)
    return torch.sum(loss) / torch.sum(w)


def train_step(params, state_sum, cfg, features, docids, labels_LB, ipw_list=None, rate=0.0, seed=0, step=0, stream=0, lr=0.05,
               max_norm=5.0, drop=None):
    """One NA (ipw_list None) / IPW step with Adagrad in float64: dict(loss, scores, grads, norm, params, state).
    drop overrides the restated masks of (rate, seed, step, stream)."""
    F, d, H, nl, dff = cfg
    L, B = np.shape(docids)
    if drop is None:
        drop = masks(seed, step, stream, B, L, d, nl, rate)
    p = torch.as_tensor(np.asarray(params), dtype=torch.float64).clone().requires_grad_(True)
    scores = forward(p, cfg, gather(features, docids), drop)
    labels = torch.from_numpy(np.ascontiguousarray(np.transpose(labels_LB))).double()
    pw = None if ipw_list is None else ipw_weights(labels_LB, ipw_list)
    loss = softmax_loss(scores, labels, pw)
    (g,) = torch.autograd.grad(loss, p)
    with torch.no_grad():
        n = torch.linalg.vector_norm(g, 2)
        gc = g * min(1.0, float(max_norm / (n + 1e-6))) if max_norm > 0 else g
        s2 = torch.as_tensor(np.asarray(state_sum), dtype=torch.float64) + gc * gc
        p2 = p.detach() - lr * gc / (s2.sqrt() + 1e-10)
    return dict(loss=float(loss.detach()), scores=scores.detach().numpy(), grads=g.numpy(), norm=float(n), params=p2.numpy(),
                state=s2.numpy())
