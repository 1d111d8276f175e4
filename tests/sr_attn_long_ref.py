"""A numpy restatement of the streaming attention forward (csrc/ultr_sr_attn_long.hip) and of SetRank's forward around it, in any
float type: the recurrence tile by tile - running row maximum and sum, the rescale of the accumulator when the maximum rises, key rows
past the list masked before the maximum is taken, the first tile without a rescale factor formed from infinities.  Not a test module:
tests/test_sr_attn_long_cpu.py proves it against the direct softmax and the oracle, tests/test_gpu_setrank_long.py uses its float64
forward as the reference of the peaked-attention cases."""
import numpy as np


def direct_attention(x):
    """softmax(x x^T / sqrt(dh)) x for one (list, head) slice x [L, dh]; returns (A [L, dh], lse [L])."""
    s = (x @ x.T) / np.sqrt(x.dtype.type(x.shape[1]))
    mx = s.max(axis=1, keepdims=True)
    e = np.exp(s - mx)
    den = e.sum(axis=1, keepdims=True)
    return (e / den) @ x, (mx + np.log(den))[:, 0]


def streamed_attention(x, tile):
    """The same, with the keys in tiles of `tile` rows as the kernels walk them.  A tile is staged whole: rows past L are zero rows whose
    scores are masked to -inf BEFORE the tile's maximum (they would score 0, which may exceed every real score of the tile)."""
    L, dh = x.shape
    ft = x.dtype.type
    scale = ft(1.0) / np.sqrt(ft(dh))
    m = np.full(L, -np.inf, dtype=x.dtype)
    den = np.zeros(L, dtype=x.dtype)
    acc = np.zeros((L, dh), dtype=x.dtype)
    for k0 in range(0, L, tile):
        keys = np.zeros((tile, dh), dtype=x.dtype)
        n = min(tile, L - k0)
        keys[:n] = x[k0:k0 + n]
        s = (x @ keys.T) * scale
        s[:, n:] = -np.inf
        mn = np.maximum(m, s.max(axis=1))
        assert np.isfinite(mn).all()  # key k0 is a real key of every tile
        # first tile: m = -inf and nothing to rescale - the factor is 0 by definition, not exp(-inf - ...)
        alpha = np.zeros(L, dtype=x.dtype) if k0 == 0 else np.exp(m - mn)
        p = np.exp(s - mn[:, None])  # exactly 0 for the masked keys
        den = den * alpha + p.sum(axis=1)
        acc = acc * alpha[:, None] + p @ keys
        m = mn
    return acc / den[:, None], m + np.log(den)


def _layer_norm(x, g, b, eps=1e-6):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + x.dtype.type(eps)) * g + b


def setrank_forward(params, F, d, H, nl, dff, features, docids, dtype=np.float64, tile=None):
    """SetRank's forward (oracle.setrank_forward, SetRank.py:143-156, 229-255) in `dtype`; tile=None: direct softmax, else the
    streamed recurrence with that tile size.  docids [L, B] position-major, PAD = n_docs gathers a zero row; PADs are ordinary keys.
    Returns scores [B, L]."""
    from oracle import ultr_oracle as O
    params = np.asarray(params, dtype=dtype)
    P = {n: params[o:o + int(np.prod(sh))].reshape(sh) for n, sh, o in O.setrank_layout(F, d, nl, dff)}
    e = "Encoder_layer."
    table = np.concatenate((np.asarray(features, dtype=dtype).reshape(-1, F), np.zeros((1, F), dtype=dtype)), axis=0)
    L, B = docids.shape
    x = table[np.asarray(docids, np.int64).reshape(-1)].reshape(L, B, F).transpose(1, 0, 2)  # [B, L, F]
    x = _layer_norm(x, P[e + "input_layer_norm.weight"], P[e + "input_layer_norm.bias"])
    x = np.maximum(x @ P[e + "input_embedding.0.weight"].T + P[e + "input_embedding.0.bias"], 0)
    x = x @ P[e + "input_embedding.2.weight"].T + P[e + "input_embedding.2.bias"]
    dh = d // H
    for i in range(nl):
        l = e + "enc_layers.encoder%d." % i
        att = np.empty_like(x)
        for b in range(B):
            for h in range(H):
                xs = np.ascontiguousarray(x[b, :, h * dh:(h + 1) * dh])
                att[b, :, h * dh:(h + 1) * dh] = (direct_attention(xs) if tile is None else streamed_attention(xs, tile))[0]
        att = att @ P[l + "mha.dense.weight"].T + P[l + "mha.dense.bias"]
        out1 = _layer_norm(x + att, P[l + "layernorm1.weight"], P[l + "layernorm1.bias"])
        f = np.maximum(out1 @ P[l + "ffn.0.weight"].T + P[l + "ffn.0.bias"], 0)
        f = f @ P[l + "ffn.2.weight"].T + P[l + "ffn.2.bias"]
        x = _layer_norm(out1 + f, P[l + "layernorm2.weight"], P[l + "layernorm2.bias"])
    o = np.maximum(x @ P[e + "output_layer.0.weight"].T + P[e + "output_layer.0.bias"], 0)
    o = o @ P[e + "output_layer.2.weight"].T + P[e + "output_layer.2.bias"]
    return o[..., 0]


def peaked(params, shape, gain=8.0):
    """The default initialisation gives near-uniform attention; input_embedding.2.weight and every layernorm2.weight times `gain` spread
    the logits (layer 0: about -24 .. 72 at gain 8) so that the running maximum really moves.  Returns a copy."""
    p = np.array(params, dtype=np.float32, copy=True)
    for name, shp, off in shape.layout():
        if name.endswith("input_embedding.2.weight") or name.endswith("layernorm2.weight"):
            p[off:off + int(np.prod(shp))] *= np.float32(gain)
    return p


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _fma32(a, b, c):
    """fl32(a * b + c) for float32 a, b, c: the product of two float32 is exact in float64, the sum is rounded there and then to float32."""
    return _f32(a.astype(np.float64) * np.float64(b) + c.astype(np.float64))


def streamed_attention_f32(x, tile, nq=None, rescale="offsets"):
    """The matrix-core kernel's arithmetic in float32, step for step, for the first nq queries of x [L, dh] against every key:
    probabilities as 2^(fma(S, c1, -m2)) with c1 = fl(log2(e) / sqrt(dh)) and m2 = fl(m * c1) the ROUNDED offset of the running maximum
    of the raw scores, sums and the accumulator in float32, the division at the end.  rescale = "offsets": the factor of what the
    earlier tiles hold is 2^(m2_old - m2_new), exactly 1 while the maximum stands - what the kernel does.  rescale = "fma": the factor as
    2^(fma(m_old, c1, -m2_new)), which leaves the rounding residue of m * c1 in the exponent when the maximum stands: a factor 2^delta of one
    sign per tile, an error that grows with the tile count.  Kept to show that the test below sees that defect.  Returns A [nq, dh]."""
    x = _f32(x)
    L, dh = x.shape
    nq = L if nq is None else nq
    q = x[:nq]
    c1 = np.float32(np.float32(1.0 / np.sqrt(np.float32(dh))) * np.float32(1.44269504088896341))
    m = np.full(nq, -np.inf, dtype=np.float32)
    m2 = np.zeros(nq, dtype=np.float32)
    den = np.zeros(nq, dtype=np.float32)
    acc = np.zeros((nq, dh), dtype=np.float32)
    for k0 in range(0, L, tile):
        keys = np.zeros((tile, dh), dtype=np.float32)
        n = min(tile, L - k0)
        keys[:n] = x[k0:k0 + n]
        s = _f32(q @ keys.T)  # raw scores (float32 accumulation, as the fp32 matrix cores)
        s[:, n:] = -np.inf
        mn = np.maximum(m, s.max(axis=1))
        mn2 = _f32(mn * c1)
        if k0 == 0:
            alpha = np.zeros(nq, dtype=np.float32)
        elif rescale == "offsets":
            alpha = np.exp2(_f32(m2 - mn2))
        else:
            alpha = np.exp2(_fma32(m, c1, -mn2))
        p = np.exp2(_fma32(s, c1, -mn2[:, None]))
        den = _f32(den * alpha + p.sum(axis=1, dtype=np.float32))
        acc = _f32(acc * alpha[:, None] + _f32(p @ keys))
        m, m2 = mn, mn2
    return acc / den[:, None]
