"""The long-list metric kernel (metrics_long_kernel, csrc/ultr_metrics.hip: one workgroup of 16 waves per list, the list's arrays in up
to 160 KiB of LDS) through ultr_metrics_long and, beyond 813 documents, ultr_metrics_report: bit for bit the one-wave kernel wherever
both take a list; the float64 restatement of tests/metrics_ref.py at the lengths only it takes (the routing threshold, the NDCG
launch's old limit, a multiple of the workgroup size and one past it, the bound); NaN scores; one arrival counter across both kernels;
rejections; and the plugin - validation() and validation_set() at max_candidate_num 900 / 1251 without a host copy, and beyond the
bound on the host without raising.  Tolerances are tests/test_gpu_metrics_all.py's."""
import numpy as np
import pytest
import torch

from tests import metrics_ref as M
from tests.test_gpu_metrics_all import (TOPN_4, TOPN_16, TOPN_ODD, ULTR_E_BADARG, ULTR_E_UNSUPPORTED, Launch, _algo, _batch, _dev, _feeds,
                                        _host_metrics, check, make_inputs, moot_rows, nan_inputs)

pytestmark = pytest.mark.gpu


class _LongEntry:
    """The library with ultr_metrics_long under ultr_metrics_report's name (the two share one argument list)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, "ultr_metrics_long" if name == "ultr_metrics_report" else name)


class LongLaunch(Launch):
    """Launch with ultr_metrics_long as its entry: the same sentinels, guard rows, report and counter checks."""

    def run(self, *a, **k):
        from ultra_pytorch_amd import _lib
        real = _lib.load
        _lib.load = lambda: _LongEntry(real())
        try:
            return super().run(*a, **k)
        finally:
            _lib.load = real


def max_list():
    from ultra_pytorch_amd import _lib
    return int(_lib.load().ultr_metrics_max_list())


# ---- 1. bit equality with the one-wave kernel ----------------------------------------------------------------------------------------
SHORT = [(1, 1, TOPN_4), (3, 2, TOPN_ODD), (5, 63, TOPN_16), (261, 64, TOPN_4), (261, 65, TOPN_16), (9, 129, TOPN_ODD), (3, 256, TOPN_4),
         (2, 800, TOPN_16), (9, 813, TOPN_ODD)]


@pytest.mark.parametrize("B,L,topn", SHORT, ids=["B%d_L%d" % (b, l) for b, l, _ in SHORT])
def test_long_entry_is_the_short_launch_bit_for_bit(B, L, topn):
    s, y, ids = make_inputs(B * 7 + L, B, L)
    args = _dev(s, y, ids)
    short, long_, again = Launch(B, L, topn), LongLaunch(B, L, topn), LongLaunch(B, L, topn)
    want, got, twice = short.run(*args, 1000), long_.run(*args, 1000), again.run(*args, 1000)
    for what, a, b, c in zip(("means", "per-list block", "order", "masked scores"), want, got, twice):
        np.testing.assert_array_equal(b, a, err_msg=what)
        np.testing.assert_array_equal(c, b, err_msg=what + ", launched twice")
    np.testing.assert_array_equal(long_.host.numpy(), short.host.numpy(), err_msg="host report")
    np.testing.assert_array_equal(again.host.numpy(), long_.host.numpy(), err_msg="host report, launched twice")


# ---- 2. the restatement at lengths only the long kernel takes --------------------------------------------------------------------------
LONG = [(3, 814), (3, 1023), (5, 1024), (9, 1025), (3, 1251), (2, 4096), (1, None)]  # None: ultr_metrics_max_list()


@pytest.mark.parametrize("topn", [TOPN_ODD, TOPN_16], ids=["k_odd", "k16"])
@pytest.mark.parametrize("B,L", LONG, ids=["B%d_L%s" % (b, l or "max") for b, l in LONG])
def test_long_lists_are_the_restatement(B, L, topn):
    L = max_list() if L is None else L
    s, y, ids = make_inputs(B * 7 + L, B, L)
    args = _dev(s, y, ids)
    direct = LongLaunch(B, L, topn).run(*args, 1000)
    check(direct, M.NAMES, s, y, ids, 1000, topn, 5.0, what="ultr_metrics_long B=%d L=%d" % (B, L))
    routed = Launch(B, L, topn).run(*args, 1000)
    assert not isinstance(routed, int), "ultr_metrics_report returned %r at list_size %d" % (routed, L)
    for a, b in zip(direct, routed):  # the same kernel: the same bits
        np.testing.assert_array_equal(b, a)


# ---- 3. NaN scores -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invalid", [False, True], ids=["valid_labels", "invalid_labels"])
@pytest.mark.parametrize("B,L", [(8, 1100), (9, 1025), (5, 1300)])
def test_long_lists_with_nan_scores(B, L, invalid):
    s, y, ids = nan_inputs(B, L, invalid)
    rows = moot_rows(s, y, ids, 1000)
    assert 2 * int(rows.sum()) >= B and np.isnan(s[rows]).any()
    got = Launch(B, L, TOPN_4).run(*_dev(s, y, ids), 1000)
    assert not isinstance(got, int), got
    check(got, M.NAMES, s, y, ids, 1000, TOPN_4, 5.0, rows=rows, what="NaN rows")
    assert (np.sort(got[2], axis=1) == np.arange(L)).all()


# ---- 4. one arrival counter across kernels and batch sizes -----------------------------------------------------------------------------
def test_one_counter_serves_both_kernels():
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    for rep, (cls, B, L) in enumerate([(LongLaunch, 5, 900), (Launch, 261, 65), (LongLaunch, 261, 900), (LongLaunch, 3, 900)]):
        s, y, ids = make_inputs(200 + rep, B, L)
        got = cls(B, L, TOPN_4, counter=counter).run(*_dev(s, y, ids), 1000, seq=rep + 1)  # (run() asserts the counter is back at 0)
        assert not isinstance(got, int), (rep, got)
        check(got, M.NAMES, s, y, ids, 1000, TOPN_4, 5.0, what="launch %d" % rep)
        assert int(counter.item()) == 0


# ---- 5. rejections -------------------------------------------------------------------------------------------------------------------
def test_long_entry_rejects_what_it_cannot_do():
    B, L = 2, max_list() + 1
    s, y, ids = make_inputs(1, B, L)
    args = _dev(s, y, ids)
    assert LongLaunch(B, L, TOPN_4).run(*args, 1000) == ULTR_E_UNSUPPORTED
    assert Launch(B, L, TOPN_4).run(*args, 1000) == ULTR_E_UNSUPPORTED
    B, L = 4, 8
    s, y, ids = make_inputs(1, B, L)
    args = _dev(s, y, ids)
    for null in ("scores", "labels", "topn", "ids", "out", "ws", "counter"):
        assert LongLaunch(B, L, TOPN_4).run(*args, 1000, **{null: None}) == ULTR_E_BADARG, null
    assert LongLaunch(B, L, TOPN_4).run(*args, 1000, n_metrics=0) == ULTR_E_BADARG
    assert LongLaunch(B, L, TOPN_4).run(*args, 1000, n_metrics=9) == ULTR_E_BADARG
    assert LongLaunch(B, L, TOPN_4, names=["mrr", 8]).run(*args, 1000) == ULTR_E_BADARG
    assert LongLaunch(B, L, TOPN_4, names=["mrr", "ndcg", "mrr"]).run(*args, 1000) == ULTR_E_BADARG  # a repeated id
    assert LongLaunch(B, L, [1, 0, 3]).run(*args, 1000) == ULTR_E_BADARG
    assert LongLaunch(B, L, [1, -2]).run(*args, 1000) == ULTR_E_BADARG
    assert LongLaunch(B, L, TOPN_4, max_label=float("nan")).run(*args, 1000) == ULTR_E_BADARG


# ---- 6. the plugin: validation() at lists beyond 813 / 1023 documents ------------------------------------------------------------------
@pytest.mark.parametrize("device_feed", [False, True], ids=["host_feed", "device_feed"])
@pytest.mark.parametrize("names", [["mrr", "ndcg", "err"], ["ndcg"]], ids=["three_keys", "ndcg_alone"])
@pytest.mark.parametrize("L", [900, 1251])
def test_validation_at_long_lists_reads_the_report_without_a_host_copy(L, names, device_feed, monkeypatch):
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    B, F, topn = 4, 13, [1, 3, 5, 10]
    feats, ids, y = _batch(B, L, F)
    algo = _algo(F, L, names)
    calls, real = [], torch.Tensor.cpu

    def counted(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)

    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", counted)
        for _ in range(2):  # the call that builds the engine and one that finds it
            _, scores, summary = algo.validation(_feeds(algo, feats, ids, y, device_feed))
            summary = dict(summary)
    assert len(calls) == 0, "validation() copied a tensor to the host %d times" % len(calls)
    assert tuple(scores.shape) == (B, L) and sorted(summary) == sorted("%s_%d" % (m, n) for m in names for n in topn)
    for key, v in _host_metrics(algo, y, names, topn).items():
        assert abs(summary[key] - v) <= 1e-6, (key, summary[key], v)


# ---- 7. the resident set ---------------------------------------------------------------------------------------------------------------
class RaggedDS:
    """tests/test_gpu_eval_set.py's DS with lists of 1 .. M documents, the shortest and the longest among them."""

    def __init__(self, n_queries, M, F, seed):
        rng = np.random.RandomState(seed)
        lens = rng.randint(1, M + 1, size=n_queries)
        lens[0], lens[1] = 1, M
        self.feature_size, self.rank_list_size, self.initial_list, self.labels, did = F, M, [], [], 0
        for n in map(int, lens):
            self.initial_list.append(list(range(did, did + n)) + [-1] * (M - n))
            self.labels.append([int(v) for v in rng.randint(0, 5, size=n)])
            did += n
        self.features = rng.uniform(-1, 1, size=(did, F)).astype(np.float32).tolist() + [[0.0] * F]
        self.dids = ["d%d" % i for i in range(did)]
        self.qids = ["q%d" % q for q in range(n_queries)]


def test_resident_set_at_900_documents_is_the_per_batch_loop(monkeypatch):
    from tests import test_gpu_eval_set as E
    from ultra_pytorch_amd import engine, input_layer
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    L, B, F = 900, 8, 13
    ds = RaggedDS(21, L, F, seed=5)
    algo = E._algo(F, L, E.NAMES, "DNN", "hidden_layer_sizes=[32, 16]")
    dfeed = input_layer.DeviceDirectLabelFeed(algo, B, "")
    want, want_scores, want_ws, sizes = E.per_batch_loop(algo, dfeed, ds, keep_ws=True)
    assert sizes == [8, 8, 5]
    called, real = [], engine.EvalSetEngine.run

    def run(self, *a, **k):
        called.append(1)
        return real(self, *a, **k)

    monkeypatch.setattr(engine.EvalSetEngine, "run", run)
    summary, scores, pq = algo.validation_set(dfeed, ds, want_scores=True, per_query=True)
    assert called, "validation_set fell back to the per-batch loop"
    assert set(want) == set(summary)
    for k in summary:
        assert summary[k] == want[k], (k, summary[k], want[k])
    assert tuple(scores.shape) == (21, L) and torch.equal(scores, want_scores)
    assert pq is not None and tuple(pq.shape) == (21, len(E.NAMES), len(E.TOPN)) and torch.equal(pq, want_ws)


# ---- 8. beyond the bound: validation() computes on the host and does not raise -----------------------------------------------------------
@pytest.mark.parametrize("device_feed", [False, True], ids=["host_feed", "device_feed"])
def test_validation_beyond_the_bound_computes_on_the_host(device_feed, monkeypatch):
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    B, L, F, names, topn = 2, max_list() + 1, 13, ["mrr", "ndcg", "err"], [1, 3, 5, 10]
    feats, ids, y = _batch(B, L, F)
    algo = _algo(F, L, names)
    _, scores, summary = algo.validation(_feeds(algo, feats, ids, y, device_feed))
    assert tuple(scores.shape) == (B, L) and sorted(summary) == sorted("%s_%d" % (m, n) for m in names for n in topn)
    masked = torch.where(torch.from_numpy(ids.T == feats.shape[0]), torch.full((), float(algo.PADDING_SCORE)), scores.cpu())
    assert (ids == feats.shape[0]).any()
    lab = torch.from_numpy(np.ascontiguousarray(y.T))
    for name in names:
        for n, v in zip(topn, metrics.make_ranking_metric_fn(name, topn)(lab, masked, None)):
            assert abs(summary["%s_%d" % (name, n)] - float(v)) <= 1e-6, (name, n, summary["%s_%d" % (name, n)], float(v))
