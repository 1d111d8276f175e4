"""Host restatement of the NSGD kernels (csrc/ultr_nsgd.hip): the null-space noise of nsgd_{dot,solve,project,finish}_kernel (Philox
normals through Box-Muller, the pivoted Cholesky that decides which memory rows are kept, the projection and the whole-tensor
normalization, in float64) and the memory update of nsgd_memory_kernel (both loser rules, exact).  The gradient, the loss and the
interleave are DBGD's (tests/dbgd_ref.py)."""
import numpy as np

from tests import dbgd_ref as D
from tests import philox_ref as P

NOISE_TAG = 0x0E56D001
PIVOT_TOL = 1e-12
EPS = 1e-12  # nsgd.py normalization's eps


def tensors(F, hidden):
    """The Linear tensors of the flat DNN vector: (offset, length, scalar) per weight and per bias, in layer order; scalar marks the
    bias of one entry (the reference's sum(shape) <= 1 branch)."""
    lay, _ = D.layout(F, hidden)
    out = []
    for (og, k, ow, m, ob) in lay:
        out.append((ow, m * k, False))
        out.append((ob, m, m == 1))
    return out


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


def kept_rows(mem):
    """The memory rows [R, n] the kernel's pivoted Cholesky of their Gram matrix keeps (largest remaining pivot first; a pivot at or
    below PIVOT_TOL x the largest squared row norm ends it).  Exactly-zero rows are never kept."""
    G = np.asarray(mem, np.float64) @ np.asarray(mem, np.float64).T
    R = G.shape[0]
    tol = G.diagonal().max(initial=0.0) * PIVOT_TOL
    W, kept = G.copy(), []
    for _ in range(R):
        free = [i for i in range(R) if i not in kept]
        q = max(free, key=lambda i: W[i, i]) if free else None
        if q is None or not W[q, q] > tol:
            break
        l = np.sqrt(W[q, q])
        col = np.where(np.isin(np.arange(R), kept + [q]), 0.0, W[:, q] / l)
        kept.append(q)
        W -= np.outer(col, col)
    return kept


def null_space_noise(z, memory, F, hidden):
    """u [R, P]: per Linear tensor and ranker, normalize(P z) with P the projection onto the complement of the kept memory rows;
    0 when the kept rows span the tensor; the one-entry bias: z / |z|; 0 on the LayerNorm entries."""
    z = np.asarray(z, np.float64)
    mem = np.asarray(memory, np.float64)
    u = np.zeros_like(z)
    for off, n, scalar in tensors(F, hidden):
        zt = z[:, off:off + n]
        if scalar:
            v = zt
        else:
            mt = mem[:, off:off + n]
            kept = kept_rows(mt)
            if len(kept) >= n:
                continue
            if kept:
                Q, _ = np.linalg.qr(mt[kept].T)  # [n, k] orthonormal basis of the kept rows
                v = zt - (zt @ Q) @ Q.T
            else:
                v = zt
        u[:, off:off + n] = v / np.sqrt(np.maximum((v ** 2).sum(1, keepdims=True), EPS))
    return u


def losers(R, winners_BR=None, ndcg=None):
    """[R] bools: ranker r + 1 lost.  With interleaving (winners [B, R + 1]): no list credits it.  Without (ndcg [R + 1]): the
    reference's batch-level winners w = ceil(ndcg_a - ndcg_0) / (sum + 1e-9) sum to 0, in the kernel's float32 order - every ranker
    or none."""
    if winners_BR is not None:
        return ~(np.asarray(winners_BR, np.float32)[:, 1:] != 0).any(0)
    nd = np.asarray(ndcg, np.float32)
    g = [np.float32(np.ceil(np.float32(x - nd[0]))) for x in nd]
    sg = np.float32(0)
    for x in g:
        sg = np.float32(sg + x)
    sw = np.float32(0)
    for x in g:
        sw = np.float32(sw + np.float32(x / np.float32(sg + np.float32(1e-9))))
    return np.full(R, bool(sw == 0))


def memory_update(noise, lost, F, hidden):
    """The memory after a step: row r = noise_r on the Linear entries if ranker r + 1 lost, else 0 (and 0 elsewhere)."""
    noise = np.asarray(noise, np.float32)
    mem = np.zeros_like(noise)
    for off, n, _ in tensors(F, hidden):
        for r, lo in enumerate(lost):
            if lo:
                mem[r, off:off + n] = noise[r, off:off + n]
    return mem
