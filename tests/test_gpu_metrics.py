"""Validation's NDCG kernel (ndcg_list_kernel, csrc/ultr_metrics.hip) behind ultr_ndcg, ultr_ndcg_report and ultr_dnn_forward_ndcg against
the float64 restatement of tests/ndcg_ref.py (itself pinned to the oracle by tests/test_metrics_cpu.py): per-list values, batch
means, the permutation and the masked scores - at list sizes across the 64-lane wavefront and up to the LDS cap, batches into the
hundred thousands, every cutoff form, ties between documents with different labels, invalid labels, PADs, infinities and NaN."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ndcg_ref as N

pytestmark = pytest.mark.gpu

PER_LIST_TOL, MEAN_TOL = 2e-6, 1e-6
TOPN_4, TOPN_16, TOPN_ODD = [1, 3, 5, 10], list(range(1, 17)), [10, 3, 1000, 3]


def make_inputs(seed, B, L, n_docs=1000):
    """scores on a 0.25 grid (ties between documents of different labels are common), graded / fractional / -1 labels, PAD ids;
    with B >= 8 the first rows are edge rows: every label invalid, all scores equal, +-1e30 and +-inf, all labels 0."""
    rng = np.random.RandomState(seed)
    s = (np.round(rng.normal(size=(B, L)) * 4) / 4).astype(np.float32)
    y = rng.randint(0, 5, size=(B, L)).astype(np.float32)
    y[rng.rand(B, L) < 0.15] += 0.5
    y[rng.rand(B, L) < 0.1] = -1.0
    ids = rng.randint(0, n_docs, size=(L, B)).astype(np.int32)
    ids[rng.rand(L, B) < 0.05] = n_docs
    if B >= 8:
        y[0] = -1.0
        s[1] = 0.75
        s[2, ::4], s[2, 1::4], s[2, 2::4] = 1e30, -1e30, np.inf
        s[2, 3::8] = -np.inf
        s[3] = np.float32(-1e30)
        s[3, ::3] = np.inf
        y[4] = 0.0
        y[5, ::2] = -1.0
        s[5] = -np.inf
    return s, np.ascontiguousarray(y.T), ids  # scores [B, L], labels and ids [L, B]


class Ndcg:
    def __init__(self, B, L, topn):
        dev = torch.device("cuda")
        self.B, self.L, self.topn = B, L, list(topn)
        self.arr = (ctypes.c_int32 * len(topn))(*[int(t) for t in topn])
        # sentinels: every element must be written; one guard row behind each output must not be
        self._out = torch.full((len(topn) + 1,), -7.0, device=dev)
        self._ws = torch.full((B + 1, len(topn)), -7.0, device=dev)
        self._order = torch.full((B + 1, L), -7, dtype=torch.int32, device=dev)
        self._masked = torch.full((B + 1, L), -7.0, device=dev)
        self.out, self.ws, self.order, self.masked = self._out[:-1], self._ws[:-1], self._order[:-1], self._masked[:-1]
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(self, s, y_LB, ids_LB, n_docs, report=False, topn_count=None):
        from ultra_pytorch_amd import _lib, hip_ops
        lib = _lib.load()
        n = len(self.topn) if topn_count is None else topn_count
        ptrs = (s.data_ptr(), y_LB.data_ptr(), ids_LB.data_ptr() if ids_LB is not None else None, n_docs, self.B, self.L, self.arr, n,
                self.out.data_ptr(), self.order.data_ptr(), self.masked.data_ptr(), self.ws.data_ptr())
        if report:
            rc = lib.ultr_ndcg_report(*ptrs, self.counter.data_ptr(), None, 1, hip_ops.raw_stream())
        else:
            rc = lib.ultr_ndcg(*ptrs, hip_ops.raw_stream())
        if rc != 0:
            return rc
        torch.cuda.synchronize()
        for guard in (self._out[-1:], self._ws[-1], self._order[-1], self._masked[-1]):
            assert (guard.cpu().numpy() == -7).all(), "a write behind the end of an output"
        return (self.out.cpu().numpy().copy(), self.ws.cpu().numpy().copy(), self.order.cpu().numpy().copy(),
                self.masked.cpu().numpy().copy())


def _dev(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def check(got, s, y_LB, ids_LB, n_docs, topn, what=""):
    out, ws, order, masked = got
    m = N.masked_scores(s, ids_LB, n_docs)
    per, ref_order, _ = N.ndcg_per_list(m, np.ascontiguousarray(y_LB.T), topn)
    np.testing.assert_array_equal(masked, m, err_msg="masked scores " + what)
    np.testing.assert_array_equal(order, ref_order, err_msg="order " + what)
    np.testing.assert_allclose(ws, per, rtol=0, atol=PER_LIST_TOL, err_msg="per-list NDCG " + what)
    np.testing.assert_allclose(out, per.mean(0), rtol=0, atol=MEAN_TOL, err_msg="batch mean " + what)
    return per


SHAPES = [(1, 1, TOPN_4), (3, 2, TOPN_ODD), (5, 63, TOPN_16), (1024, 1, TOPN_4), (1024, 2, TOPN_16), (1024, 63, TOPN_ODD),
          (1024, 64, TOPN_4), (1024, 65, TOPN_16), (1024, 100, TOPN_ODD), (100003, 64, TOPN_4), (100003, 100, TOPN_ODD),
          (3, 129, TOPN_4), (1024, 129, TOPN_ODD), (5, 256, TOPN_16), (1024, 256, TOPN_4), (1024, 1023, TOPN_ODD), (3, 1023, TOPN_16)]


@pytest.mark.parametrize("report", [False, True], ids=["two_launch", "report"])
@pytest.mark.parametrize("B,L,topn", SHAPES, ids=["B%d_L%d_k%d" % (b, l, len(t)) for b, l, t in SHAPES])
def test_ndcg_is_the_restatement(B, L, topn, report):
    s, y, ids = make_inputs(B * 7 + L, B, L)
    k = Ndcg(B, L, topn)
    got = k.run(*_dev(s, y, ids), 1000, report=report)
    check(got, s, y, ids, 1000, topn, "B=%d L=%d" % (B, L))
    assert (np.sort(got[2], axis=1) == np.arange(L)).all()


def test_ndcg_without_docids_masks_nothing():
    B, L = 37, 70
    s, y, _ = make_inputs(3, B, L)
    k = Ndcg(B, L, TOPN_4)
    st, yt = _dev(s, y)
    got = k.run(st, yt, None, 0)
    check(got, s, y, None, 0, TOPN_4)


def test_report_counter_is_reused_across_batch_sizes():
    """ultr_ndcg_report on ONE arrival counter: B = 1024, then 5, then 1024 - each launch must find the counter reset by the one before."""
    L = 65
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    for rep, B in enumerate((1024, 5, 1024)):
        s, y, ids = make_inputs(100 + rep, B, L)
        k = Ndcg(B, L, TOPN_16)
        k.counter = counter
        got = k.run(*_dev(s, y, ids), 1000, report=True)
        check(got, s, y, ids, 1000, TOPN_16, "launch %d" % rep)
        two = Ndcg(B, L, TOPN_16).run(*_dev(s, y, ids), 1000)
        for a, b in zip(got, two):
            np.testing.assert_array_equal(a, b)  # the one-launch form sums in the two-launch form's order: the same bits
        assert int(counter.item()) == 0


def test_ndcg_rejects_what_it_cannot_do():
    ULTR_E_BADARG, ULTR_E_UNSUPPORTED = -1, -2
    s, y, ids = make_inputs(1, 4, 1024)
    args = _dev(s, y, ids)
    for report in (False, True):
        assert Ndcg(4, 1024, TOPN_4).run(*args, 1000, report=report) == ULTR_E_UNSUPPORTED  # (16 L + 4) * 4 bytes > 64 KiB of LDS
        s2, y2, i2 = make_inputs(1, 4, 8)
        a2 = _dev(s2, y2, i2)
        assert Ndcg(4, 8, list(range(1, 18))).run(*a2, 1000, report=report) == ULTR_E_BADARG  # 17 cutoffs
        assert Ndcg(4, 8, [1, 0, 3]).run(*a2, 1000, report=report) == ULTR_E_BADARG


@pytest.mark.parametrize("invalid", [False, True], ids=["valid_labels", "invalid_labels"])
@pytest.mark.parametrize("B,L", [(8, 12), (1024, 65), (5, 130)])
def test_ndcg_with_nan_scores(B, L, invalid):
    """A diverging model scores NaN.  The oracle (torch) orders NaN above every number and carries it into the row minimum that invalid
    labels take; the kernel must report the same per-list NDCG, a permutation with the oracle's key sequence (every index once), and
    repeat itself bit for bit - not read LDS slots that no rank was written to."""
    rng = np.random.RandomState(B + L + invalid)
    s, y, ids = make_inputs(B * 3 + L, B, L)
    y = np.where(y < 0, 1.0, y).astype(np.float32)
    for b in range(B):
        if b % 4 == 3:
            continue  # rows without NaN in the same launch
        s[b, rng.choice(L, size=1 + b % 2, replace=False)] = np.nan
        if invalid:
            y[rng.choice(L, size=2, replace=False), b] = -1.0
    k = Ndcg(B, L, TOPN_4)
    args = _dev(s, y, ids)
    first = k.run(*args, 1000)
    check(first, s, y, ids, 1000, TOPN_4, "NaN rows")
    assert (np.sort(first[2], axis=1) == np.arange(L)).all()
    again = Ndcg(B, L, TOPN_4).run(*args, 1000, report=True)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)


def test_eval_engine_is_the_restatement():
    """EvalEngine.run (ultr_dnn_forward_ndcg: forward + metric in one call) at L = 100, B = 1024: its per-list values, permutation
    and masked scores against the restatement of its own scores."""
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model import init_flat_params
    B, L, F = 1024, 100, 24
    shape = hip_ops.DnnShape(F, [32, 16], "elu")
    p = init_flat_params(shape, 5).cuda()
    ev = engine.EvalEngine(shape, B, L, torch.device("cuda"))
    rng = np.random.RandomState(11)
    feats, ids, y = synthetic.make_batch(rng, B, L, F, clicks=False, n_pad=7)
    y = y.copy()
    y[rng.rand(*y.shape) < 0.1] = -1.0
    f, i_, y_ = _dev(feats, ids, y)
    ev.run(p, f, feats.shape[0], i_, y_)
    got = ev.read_ndcg()
    scores = ev.scores.cpu().numpy()
    per = check((got, ev.ndcg_ws.cpu().numpy().reshape(B, -1), ev.order.cpu().numpy(), ev.masked.cpu().numpy()), scores, y, ids,
                feats.shape[0], ev.topn)
    assert per[:, -1].mean() > 0
