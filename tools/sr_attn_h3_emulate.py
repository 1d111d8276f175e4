"""CPU: a float64 restatement of the split-half attention backward (sr_attn_bwd_h3_kernel) inside the float64 autograd step, to see
which of its ingredients moves a gradient how far - the 22-bit hi + lo operands, or the sum inside v_mfma_f32_16x16x32_f16, modelled as
"align the 32 products and the accumulator to the largest, truncate `bits` bits below it, add" (tools/mfma_f16_accum_test.hip: about
25) - and in which of the five products (S, dP / dP^T, dq + dk, dv).  The forward is restated in fp32 as sr_attn_fwd_mfma_kernel
computes it (lse and A are consistent with ITS S); element-wise algebra in fp32.  The model of the adder is a guess at the magnitude,
not the instruction's bits.  Figures: DESIGN.md section 4, "The one-pass attention kernels at peaked attention".
    python tools/sr_attn_h3_emulate.py 3,64,24,64,1,2,16 8"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from oracle import ultr_oracle as O  # noqa: E402
from tests import sr_attn_bwd_ref as RB  # noqa: E402
from tests import test_setrank_peaked_cpu as C  # noqa: E402

f32, f16, f64 = np.float32, np.float16, np.float64
LOG2E = f32(1.44269504088896341)
PRODUCTS = ("S", "dP", "acc", "acv")


def pow2_scale(amax, target):
    """srs_pow2_scale: the power of two that brings amax just below 2^target."""
    return f32(2.0 ** (target - 1 - math.floor(math.log2(float(amax)))))


def split(v):
    """hi = fp16(v), lo = fp16(v - hi), as float64 arrays."""
    v = v.astype(f32)
    hi = v.astype(f16)
    lo = (v - hi.astype(f32)).astype(f32).astype(f16)
    return [hi.astype(f64), lo.astype(f64)]


def mfma(a, b, acc, bits):
    """One instruction: acc[m, n] + a[m, 32] . b[n, 32], the result an fp32 number.  bits None: an exact sum."""
    prod = a[:, None, :] * b[None, :, :]  # fp16 x fp16: exact in float64
    if bits is None:
        return (prod.sum(-1) + acc).astype(f32).astype(f64)
    mx = np.maximum(np.abs(prod).max(-1), np.abs(acc))
    quantum = 2.0 ** (np.floor(np.log2(np.where(mx > 0, mx, 1.0))) - bits)
    total = (np.trunc(prod / quantum[..., None]) * quantum[..., None]).sum(-1) + np.trunc(acc / quantum) * quantum
    return total.astype(f32).astype(f64)


def product(A, B, bits):
    """sum_k A[m, k] B[n, k] over split operands, 32 indices per instruction, the kernel's order hi.lo, lo.hi, hi.hi."""
    m, K = A[0].shape
    acc = np.zeros((m, B[0].shape[0]))
    for k0 in range(0, K, 32):
        for ia, ib in ((0, 1), (1, 0), (0, 0)):
            a, b = np.zeros((m, 32)), np.zeros((B[0].shape[0], 32))
            w = min(32, K - k0)
            a[:, :w], b[:, :w] = A[ia][:, k0:k0 + w], B[ib][:, k0:k0 + w]
            acc = mfma(a, b, acc, bits)
    return acc


def forward_fp32(x):
    """sr_attn_fwd_mfma_kernel for one (list, head) slice: (A, lse), fp32 values."""
    x32 = x.astype(f32)
    S = (x32.astype(f64) @ x32.astype(f64).T).astype(f32)
    mx = S.max(1)
    scale = f32(1.0 / np.sqrt(f32(x.shape[1])))
    c1 = f32(scale * LOG2E)
    mx2 = (mx * c1).astype(f32)
    p = np.exp2((S.astype(f64) * float(c1) - mx2[:, None].astype(f64)).astype(f32).astype(f64)).astype(f32)
    sm = p.sum(1, dtype=f64).astype(f32)
    pv = (p * (f32(1.0) / sm)[:, None]).astype(f32)
    A = (pv.astype(f64) @ x32.astype(f64)).astype(f32)
    lse = ((mx * scale).astype(f32) + np.log(sm.astype(f64)).astype(f32)).astype(f32)
    return A.astype(f64), lse.astype(f64)


def backward_h3(x, dA, Aout, lse, exact_operands=False, bits=None, only=None):
    """sr_attn_bwd_h3_kernel for one slice: dx [L, dh].  exact_operands: fp32 operands, unsplit; bits: the adder's model, in the
    product named by `only` or in all of them."""
    L, dh = x.shape
    x32, g32, A32 = x.astype(f32), dA.astype(f32), Aout.astype(f32)
    lse2 = (lse.astype(f32) * LOG2E).astype(f32)
    t = (g32.astype(f64) * A32.astype(f64)).sum(1).astype(f32)
    sx, sg = pow2_scale(np.abs(x32).max(), 10), pow2_scale(np.abs(g32).max(), 4)
    isx, isg = f32(1.0) / sx, f32(1.0) / sg
    scale = f32(1.0 / np.sqrt(f32(dh)))
    adder = {k: (bits if only in (None, k) else None) for k in PRODUCTS}

    def operands(v):
        return [v.astype(f32).astype(f64), np.zeros(v.shape)] if exact_operands else split(v)

    X, G = operands(x32 * sx), operands(g32 * sg)
    sc = product(X, X, adder["S"]).astype(f32)      # [partner j, own i]: sx^2 S
    dpt = product(X, G, adder["dP"]).astype(f32)    # x[j] . dA[i]
    dpn = product(G, X, adder["dP"]).astype(f32)    # dA[j] . x[i]
    c1 = f32(f32(f32(scale * isx) * isx) * LOG2E)
    tsg = (t * sg).astype(f32)

    def prob(l):
        return np.exp2((sc.astype(f64) * float(c1) - l.astype(f64)).astype(f32).astype(f64)).astype(f32)

    pa, pb = prob(lse2[None, :]), prob(lse2[:, None])
    dsa = ((scale * pa).astype(f32) * ((dpt * isx).astype(f32) - tsg[None, :]).astype(f32)).astype(f32)
    dsb = ((scale * pb).astype(f32) * ((dpn * isx).astype(f32) - tsg[:, None]).astype(f32)).astype(f32)
    a = (dsa + dsb).astype(f32)
    acc = product(operands(a.T), [p.T.copy() for p in X], adder["acc"])                       # [own i, c]
    acv = product(operands((pb * f32(4096.0)).T), [p.T.copy() for p in G], adder["acv"])
    s1, s2 = f32(isx * isg), f32(isg * f32(1.0 / 4096.0))
    return ((acc.astype(f32) * s1).astype(f32) + (acv.astype(f32) * s2).astype(f32)).astype(f64)


class Attention(torch.autograd.Function):
    mode = None  # None: float64 throughout; else the keyword arguments of backward_h3

    @staticmethod
    def forward(ctx, q):
        if Attention.mode is None:
            s = (q @ q.transpose(-1, -2)) / math.sqrt(q.shape[-1])
            lse = torch.logsumexp(s, -1)
            A = torch.exp(s - lse[..., None]) @ q
        else:
            qn = q.numpy()
            A, lse = np.zeros(qn.shape), np.zeros(qn.shape[:-1])
            for b in range(qn.shape[0]):
                for h in range(qn.shape[1]):
                    A[b, h], lse[b, h] = forward_fp32(qn[b, h])
            A, lse = torch.from_numpy(A), torch.from_numpy(lse)
        ctx.save_for_backward(q, A, lse)
        return A

    @staticmethod
    def backward(ctx, dA):
        q, A, lse = ctx.saved_tensors
        if Attention.mode is None:
            p = torch.exp((q @ q.transpose(-1, -2)) / math.sqrt(q.shape[-1]) - lse[..., None])
            dS = p * (dA @ q.transpose(-1, -2) - (dA * A).sum(-1, keepdim=True)) / math.sqrt(q.shape[-1])
            return dS @ q + dS.transpose(-1, -2) @ q + p.transpose(-1, -2) @ dA
        out = np.zeros(tuple(q.shape))
        for b in range(q.shape[0]):
            for h in range(q.shape[1]):
                out[b, h] = backward_h3(q[b, h].numpy(), dA[b, h].numpy(), A[b, h].numpy(), lse[b, h].numpy(), **Attention.mode)
        return torch.from_numpy(out)


def step_gradient(p0, cfg, feats, ids, y, ipw):
    """tests/sr_attn_bwd_ref.train_step with Attention in the place of the softmax attention."""
    F, d, H, nl, dff = cfg
    p = torch.as_tensor(np.asarray(p0), dtype=torch.float64).clone().requires_grad_(True)
    W = {n: p[o:o + int(np.prod(sh))].reshape(sh) for n, sh, o in O.setrank_layout(F, d, nl, dff)}
    ln = torch.nn.functional.layer_norm
    e = "Encoder_layer."
    x = RB.gather(feats, ids)
    B, L = x.shape[0], x.shape[1]
    x = ln(x, (F,), W[e + "input_layer_norm.weight"], W[e + "input_layer_norm.bias"], 1e-6)
    x = torch.relu(x @ W[e + "input_embedding.0.weight"].T + W[e + "input_embedding.0.bias"])
    x = x @ W[e + "input_embedding.2.weight"].T + W[e + "input_embedding.2.bias"]
    for i in range(nl):
        l = e + "enc_layers.encoder%d." % i
        att = Attention.apply(x.reshape(B, L, H, d // H).permute(0, 2, 1, 3).contiguous())
        att = att.permute(0, 2, 1, 3).reshape(B, L, d)
        o = att @ W[l + "mha.dense.weight"].T + W[l + "mha.dense.bias"]
        out1 = ln(x + o, (d,), W[l + "layernorm1.weight"], W[l + "layernorm1.bias"], 1e-6)
        f = torch.relu(out1 @ W[l + "ffn.0.weight"].T + W[l + "ffn.0.bias"])
        f = f @ W[l + "ffn.2.weight"].T + W[l + "ffn.2.bias"]
        x = ln(out1 + f, (d,), W[l + "layernorm2.weight"], W[l + "layernorm2.bias"], 1e-6)
    o = torch.relu(x @ W[e + "output_layer.0.weight"].T + W[e + "output_layer.0.bias"])
    scores = (o @ W[e + "output_layer.2.weight"].T + W[e + "output_layer.2.bias"])[..., 0]
    labels = torch.from_numpy(np.ascontiguousarray(np.transpose(y))).double()
    loss = RB.softmax_loss(scores, labels, O.ipw_weights(y, ipw).double())
    (g,) = torch.autograd.grad(loss, p)
    return g.numpy()


def main():
    shape = tuple(int(v) for v in sys.argv[1].split(","))
    gain = float(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2] != "none" else None
    p0, feats, ids, y, ipw, r32, r64 = C.case(shape, gain)
    modes = [("float64 throughout", None),
             ("fp32 operands, exact sums (the fp32 matrix-core kernels)", dict(exact_operands=True)),
             ("hi + lo operands, exact sums", dict())]
    modes += [("hi + lo operands, adder keeps %d bits in %s only" % (b, k), dict(bits=b, only=k)) for k in PRODUCTS for b in (25, 26)]
    modes += [("hi + lo operands, adder keeps %d bits everywhere" % b, dict(bits=b)) for b in (25, 26)]
    for name, mode in modes:
        Attention.mode = mode
        g = step_gradient(p0, tuple(shape[2:]), feats, ids, y, ipw)
        print("%-60s largest distance to float64 %.3g = %.3g of hold_to_float64's bound" % (name, float(np.abs(g - r64["grads"]).max()),
                                                                                         C.in_bars(g, r32, r64)), flush=True)


if __name__ == "__main__":
    main()
