"""plrank_kernel (csrc/ultr_plrank.hip) on the GPU against the float64 law of tests/plrank_ref.py.

The sampled orders are an input of the law: every comparison of values feeds the twin the kernel's OWN perm_out; the orders themselves
are compared with the host restatement of the race (Philox uniforms, float64 keys) wherever the draw is not within rounding of a tie.

Bars (tests/loss_ref.py): SCALAR_RTOL for each list's loss, TERMS_RTOL * (|ref| + sum |terms|) for dscores - plus float32's smallest
normal number, below which a float32 carries no relative precision (tests/plrank_ref.dscores_bar)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import loss_ref as R  # noqa: E402
from tests import plrank_ref as T  # noqa: E402

N_DOCS = 1000
SENTINEL = -12345.0


def lpw():
    from ultra_pytorch_amd import hip_ops
    return 4 // int(hip_ops.loss_part_count(4))


def make_lists(seed, B, L, scale=1.5, pads=0, click_rate=0.35):
    """scores [B, L], docids [L, B] with `pads` interior PADs per list (id = N_DOCS), labels [L, B]: clicks, a grade, a fraction."""
    rng = np.random.RandomState(seed)
    scores = (rng.normal(size=(B, L)) * scale).astype(np.float32)
    docids = rng.randint(0, N_DOCS, size=(L, B)).astype(np.int32)
    for b in range(B):
        if pads and L > pads:
            docids[rng.choice(L, size=pads, replace=False), b] = N_DOCS
    labels = (rng.uniform(size=(L, B)) < click_rate).astype(np.float32) * rng.choice(np.array([1.0, 1.0, 2.0, 0.5], np.float32), size=(L, B))
    return scores, docids, labels


def run_kernel(scores, docids, labels, N, cutoff=0, gain="linear", seed=11, step=3, pw=None, ipw=None, perm=True):
    """One launch: dscores [B, L], perm_out [B, N, L] (or None), the per-list tails [B, 4 + 2 L]."""
    from ultra_pytorch_amd import hip_ops
    dev = torch.device("cuda")
    B, L = scores.shape
    s, y, d = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scores, labels, docids))
    ds = torch.full((B, L), SENTINEL, dtype=torch.float32, device=dev)
    ws = torch.full((hip_ops.loss_workspace_bytes(B, L) // 4,), SENTINEL, dtype=torch.float32, device=dev)
    po = torch.full((B, N, L), -1, dtype=torch.int32, device=dev) if perm else None
    pw_d = torch.from_numpy(np.ascontiguousarray(pw)).to(dev) if pw is not None else None
    ipw_d = torch.from_numpy(np.ascontiguousarray(ipw)).to(dev) if ipw is not None else None
    hip_ops.plrank_loss(s, y, d, N_DOCS, B, L, ds, ws, n_samples=N, cutoff=cutoff, gain=gain, seed=seed, step=step, pw=pw_d,
                        ipw_table=ipw_d, perm_out=po)
    torch.cuda.synchronize()
    tail = 4 + 2 * L
    assert lpw() == 1  # one list per workgroup: one tail partial per list
    return ds.cpu().numpy(), (po.cpu().numpy().astype(np.int64) if perm else None), ws[:B * tail].view(B, tail).cpu().numpy()


def hold(tag, scores, docids, labels, N, cutoff, gain, pw=None, ipw=None, **kw):
    """The kernel against the twin put on the kernel's own orders; returns (dscores, perm, n_pos, valid)."""
    ds, perm, tails = run_kernel(scores, docids, labels, N, cutoff, gain, pw=pw, ipw=ipw, **kw)
    B, L = scores.shape
    valid = T.valid_of(docids, N_DOCS)
    n_pos, margin = T.n_pos_of(scores, valid)
    assert (margin > 1e-4).all(), (tag, "a log-probability within 1e-4 of the zero threshold: choose other inputs")
    assert (np.sort(perm, axis=2) == np.arange(L)).all(), (tag, "perm_out rows are permutations")
    for b in range(B):  # behind the drawn documents: the zero-probability ones and the PADs, in index order
        rest = perm[b, :, n_pos[b]:]
        assert (np.diff(rest, axis=1) > 0).all(), (tag, b)
    rho = T.rho_of(labels, valid, gain, pw=pw, ipw=ipw)
    ref = T.reference(scores, rho, valid, perm, cutoff, n_pos)
    err = np.abs(ds.astype(np.float64) - ref["dscores"])
    bar = T.dscores_bar(ref["dscores"], ref["terms"], R.TERMS_RTOL)
    e_loss = np.abs(tails[:, 0] - ref["loss_b"]) / np.maximum(1.0, np.abs(ref["loss_b"]))
    print("%s: dscores %.3g of the bar, loss %.3g (bar %.0e)" % (tag, float((err / bar).max()), float(e_loss.max()), R.SCALAR_RTOL))
    assert np.isfinite(ds).all() and (err <= bar).all(), (tag, float((err / bar).max()))
    assert (e_loss <= R.SCALAR_RTOL).all(), (tag, float(e_loss.max()))
    assert (tails[:, 1] == 1.0).all() and (tails[:, 2:] == 0.0).all()
    assert (ds[~valid] == 0.0).all()  # a PAD gets exactly 0
    return ds, perm, n_pos, valid


LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 129, 256)  # the lane boundaries, the slice boundaries and the 256 of the other list losses
SAMPLES = (1, 15, 16, 17, 100)                      # fewer samples than waves, one per wave, the wrap
TABLE = np.array([1.0, 1.3, 1.9, 2.6, 3.8], np.float32)  # shorter than most lists: the last entry serves the rest


@pytest.mark.parametrize("L", LENGTHS)
def test_kernel_against_the_twin(L):
    """Every N at every L; B, the cutoff, the gain and the weight source rotate so that each value meets each L-class."""
    batches = (1, 3, lpw() + 1)
    cutoffs = (1, 3, 0, L + 5)
    k = LENGTHS.index(L)
    for j, N in enumerate(SAMPLES):
        B, cutoff = batches[(j + k) % 3], cutoffs[(j + k) % 4]
        gain, weights = ("linear", "exp2")[(j + k) % 2], ("table", "pw", None)[(j + 2 * k) % 3]
        scores, docids, labels = make_lists(1000 * L + j, B, L, pads=1 if L > 2 and j % 2 else 0)
        rng = np.random.RandomState(j)
        pw = rng.uniform(0.5, 4.0, size=(B, L)).astype(np.float32) if weights == "pw" else None
        hold("L=%d B=%d N=%d K=%d %s %s" % (L, B, N, cutoff, gain, weights), scores, docids, labels, N, cutoff, gain, pw=pw,
             ipw=TABLE if weights == "table" else None)


def test_special_lists():
    """Interior PADs, fewer valid documents than K, no valid document, no click, tied scores - one list each, and a plain one."""
    B, L, N, K = 6, 17, 17, 5
    scores, docids, labels = make_lists(5, B, L)
    docids[[2, 5, 9], 0] = N_DOCS
    docids[:, 1] = N_DOCS
    docids[[3, 11], 1] = [4, 8]          # two valid documents, K = 5
    labels[[3, 11], 1] = 1.0
    docids[:, 2] = -1                    # none: ids below 0 are PADs too
    labels[:, 3] = 0.0                   # no click
    scores[4, :] = np.float32(0.75)      # ties
    scores[5, ::2] = scores[5, 1]
    labels[0, 4] = labels[7, 4] = 1.0
    ds, perm, n_pos, valid = hold("special", scores, docids, labels, N, K, "linear", ipw=TABLE)
    assert n_pos.tolist()[1:3] == [2, 0]
    assert (perm[2] == np.arange(L)).all()          # nothing to draw: index order
    assert (ds[2] == 0.0).all() and (ds[3] == 0.0).all()
    _, _, tails = run_kernel(scores, docids, labels, N, K, "linear", ipw=TABLE, perm=False)
    assert tails[2, 0] == 0.0 and tails[3, 0] == 0.0 and tails[0, 0] < 0.0  # loss 0 without a click or a document
    assert len({tuple(r) for r in perm[4]}) > 1      # tied scores are still drawn in different orders
    assert np.abs(ds[4]).max() > 0.0


@pytest.mark.parametrize("L,cutoff", [(10, 0), (65, 0), (65, 4), (130, 0)])
def test_scores_of_scale_40(L, cutoff):
    """Documents underflow to probability 0 (they follow the drawn ones in index order) and e spans the float32 range."""
    scores, docids, labels = make_lists(40 + L, 3, L, scale=40.0, pads=1, click_rate=0.5)
    ds, perm, n_pos, valid = hold("scale 40 L=%d K=%d" % (L, cutoff), scores, docids, labels, 33, cutoff, "linear", ipw=TABLE)
    assert (n_pos < valid.sum(axis=1)).any() and (n_pos >= 1).all()


def test_the_longest_list_and_one_past_it():
    from ultra_pytorch_amd import _lib
    L = T.MAX_L
    scores, docids, labels = make_lists(77, 1, L, scale=2.0, pads=3)
    hold("L=%d" % L, scores, docids, labels, 17, 10, "exp2", ipw=TABLE)
    scores, docids, labels = make_lists(78, 2, L + 1)
    with pytest.raises(_lib.UltrHipError):
        run_kernel(scores, docids, labels, 4)
    # ... with nothing written
    from ultra_pytorch_amd import hip_ops
    dev = torch.device("cuda")
    s, y, d = (torch.from_numpy(a).to(dev) for a in (scores, labels, docids))
    ds = torch.full((2, L + 1), SENTINEL, dtype=torch.float32, device=dev)
    ws = torch.full((hip_ops.loss_workspace_bytes(2, L + 1) // 4,), SENTINEL, dtype=torch.float32, device=dev)
    po = torch.full((2, 4, L + 1), -1, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.UltrHipError):
        hip_ops.plrank_loss(s, y, d, N_DOCS, 2, L + 1, ds, ws, n_samples=4, perm_out=po)
    torch.cuda.synchronize()
    assert (ds == SENTINEL).all() and (ws == SENTINEL).all() and (po == -1).all()


PERM_SHAPES = (10, 16, 65, 129, 256)


def perm_case(L):
    scale = max(1.5, 0.31 * L)
    scores, docids, labels = make_lists(300 + L, 8, L, scale=scale, pads=1)
    return scores, docids, labels


@pytest.mark.parametrize("L", PERM_SHAPES)
def test_permutations_against_the_host_restatement(L):
    """B 8, N 64, score scale max(1.5, 0.31 L): every (list, sample) whose float64 race keys are more than 1e-4 apart and whose
    log-probabilities are more than 1e-4 from the zero threshold must be drawn in exactly the host's order; at least 97 % are such."""
    scores, docids, labels = perm_case(L)
    N, seed, step = 64, 0x1234567890ABCDEF, 41
    _, perm, _ = run_kernel(scores, docids, labels, N, seed=seed, step=step)
    valid = T.valid_of(docids, N_DOCS)
    orders, sep = T.host_orders(scores, valid, seed, step, N)
    share = float(sep.mean())
    same = (perm == orders).all(axis=2)
    print("L=%d: %.1f %% of the pairs are separated; %d of the others differ" % (L, 100 * share, int((~same & ~sep).sum())))
    assert share >= 0.97
    assert same[sep].all(), (L, int((~same & sep).sum()))
    assert (np.sort(perm, axis=2) == np.arange(L)).all()
    n_pos, _ = T.n_pos_of(scores, valid)
    for b in range(8):
        assert (np.diff(perm[b, :, n_pos[b]:], axis=1) > 0).all()  # zero-probability documents and PADs: last, in index order
        assert valid[b][perm[b, :, :n_pos[b]]].all()


def test_unbiased_on_the_device():
    """4096 identical lists at (L, K) = (5, 3), 64 samples each: the mean of -dscores over the lists against the enumerated exact
    gradient, within 4.75 standard errors of the estimator (its exact sigma from the same enumeration) plus the terms bar."""
    B, N, L, K = 4096, 64, 5, 3
    s = np.array([0.4, -0.3, 1.1, 0.0, -1.2], np.float32)
    y = np.array([1.0, 0.0, 1.0, 0.0, 1.0], np.float32)
    table = np.array([1.0, 1.5, 2.0, 2.5, 3.0], np.float32)
    scores = np.tile(s, (B, 1))
    labels = np.tile(y[:, None], (1, B))
    docids = np.tile(np.arange(L, dtype=np.int32)[:, None], (1, B))
    ds, perm, tails = run_kernel(scores, docids, labels, N, cutoff=K, ipw=table, seed=2024, step=7)
    valid = np.ones((B, L), bool)
    rho = T.rho_of(labels, valid, "linear", ipw=table)
    ref = T.reference(scores, rho, valid, perm, K, np.full(B, L))
    bar = T.dscores_bar(ref["dscores"], ref["terms"], R.TERMS_RTOL)
    assert (np.abs(ds - ref["dscores"]) <= bar).all()  # more than one workgroup per CU: every list against the twin as well
    reward, mean, sd = T.enumerate_exact(s, rho[0], K)
    got = -ds.astype(np.float64).mean(axis=0)
    allowed = 4.75 * sd / np.sqrt(B * N) + R.TERMS_RTOL * (np.abs(mean) + ref["terms"].mean(axis=0))
    print("unbiasedness: |mean - exact| / allowed =", np.abs(got - mean) / allowed, "reward", -tails[:, 0].mean(), "exact", reward)
    assert (np.abs(got - mean) <= allowed).all()
    assert len({tuple(r) for r in perm[:, 0].tolist()}) > 50  # the lists draw different rankings


def test_determinism():
    scores, docids, labels = make_lists(9, 5, 70, scale=3.0, pads=2)
    a = run_kernel(scores, docids, labels, 40, cutoff=7, ipw=TABLE, seed=5, step=100)
    b = run_kernel(scores, docids, labels, 40, cutoff=7, ipw=TABLE, seed=5, step=100)
    for x, z in zip(a, b):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, z.view(np.uint32) if z.dtype == np.float32 else z)
    c = run_kernel(scores, docids, labels, 40, cutoff=7, ipw=TABLE, seed=5, step=101)
    assert not np.array_equal(a[1], c[1])
    d = run_kernel(scores, docids, labels, 40, cutoff=7, ipw=TABLE, seed=6, step=100)
    assert not np.array_equal(a[1], d[1])
    e = run_kernel(scores, docids, labels, 40, cutoff=7, ipw=TABLE, seed=5, step=100, perm=False)  # perm_out changes nothing
    assert np.array_equal(a[0].view(np.uint32), e[0].view(np.uint32)) and np.array_equal(a[2].view(np.uint32), e[2].view(np.uint32))
