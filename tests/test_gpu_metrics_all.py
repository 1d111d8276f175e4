"""ultr_metrics_report / ultr_dnn_forward_metrics (ndcg_list_kernel<ALL>, csrc/ultr_metrics.hip): the eight validation metrics of
utils/metrics.py out of the one metric launch, against the float64 restatement of tests/metrics_ref.py (itself pinned to the oracle and
to the reference's recorded values by tests/test_metrics_all_cpu.py) - per-list values, batch means, the permutation and the masked
scores, at list sizes across the 64-lane chunks of the rank scans and up to the largest list the entry point must take; the NDCG row
against ultr_ndcg_report bit for bit; and BaseAlgorithm.validation reading every metric without a copy to the host."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as M
from tests import ndcg_ref as N

pytestmark = pytest.mark.gpu

PER_LIST_TOL, MEAN_TOL = 2e-6, 1e-6  # tests/test_gpu_metrics.py's; times max(1, |reference|) for the unbounded dcg and arp
TOPN_4, TOPN_16, TOPN_ODD = [1, 3, 5, 10], list(range(1, 17)), [10, 3, 1000, 3]
ULTR_E_BADARG, ULTR_E_UNSUPPORTED = -1, -2
SEQ_WORD = 128
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def make_inputs(seed, B, L, n_docs=1000):
    """tests/test_gpu_metrics.py make_inputs: scores on a 0.25 grid (ties between documents of different labels are common), graded /
    fractional / -1 labels, PAD ids; with B >= 8 the first rows are edge rows: every label invalid, all scores equal, +-1e30 and
    +-inf, all labels 0."""
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


def _dev(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


class Launch:
    """One ultr_metrics_report with sentinels: every element must be written; one guard row behind each output must not be."""

    def __init__(self, B, L, topn, names=M.NAMES, max_label=5.0, counter=None, report=True):
        dev = torch.device("cuda")
        self.B, self.L, self.topn, self.names, self.max_label = B, L, list(topn), list(names), max_label
        nm, nt = len(self.names), len(self.topn)
        self.arr = (ctypes.c_int32 * nt)(*[int(t) for t in topn])
        self.ids = (ctypes.c_int32 * max(nm, 1))(*[M.IDS[n] if isinstance(n, str) else int(n) for n in self.names])
        self._out = torch.full((nm + 1, nt), -7.0, device=dev)
        self._ws = torch.full((B + 1, nm, nt), -7.0, device=dev)
        self._order = torch.full((B + 1, L), -7, dtype=torch.int32, device=dev)
        self._masked = torch.full((B + 1, L), -7.0, device=dev)
        self.out, self.ws, self.order, self.masked = self._out[:-1], self._ws[:-1], self._order[:-1], self._masked[:-1]
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev) if counter is None else counter
        self.host = torch.full((SEQ_WORD + 2,), -7.0).pin_memory() if report else None  # [.. means .., seq word, guard]

    def run(self, s, y_LB, ids_LB, n_docs, seq=5, n_metrics=None, **null):
        from ultra_pytorch_amd import _lib, hip_ops
        lib = _lib.load()
        p = dict(scores=s.data_ptr(), labels=y_LB.data_ptr(), topn=self.arr, ids=self.ids, out=self.out.data_ptr(), ws=self.ws.data_ptr(),
                 counter=self.counter.data_ptr())
        p.update(null)  # a pointer replaced by None
        rc = lib.ultr_metrics_report(p["scores"], p["labels"], ids_LB.data_ptr() if ids_LB is not None else None, n_docs, self.B, self.L,
                                     p["topn"], len(self.topn), p["ids"], len(self.names) if n_metrics is None else n_metrics,
                                     self.max_label, p["out"], self.order.data_ptr(), self.masked.data_ptr(), p["ws"], p["counter"],
                                     self.host.data_ptr() if self.host is not None else None, seq, hip_ops.raw_stream())
        if rc != 0:
            return rc
        torch.cuda.synchronize()
        for guard in (self._out[-1], self._ws[-1], self._order[-1], self._masked[-1]):
            assert (guard.cpu().numpy() == -7).all(), "a write behind the end of an output"
        out = self.out.cpu().numpy().copy()
        if self.host is not None:
            h = self.host.numpy()
            assert int(h.view(np.uint32)[SEQ_WORD]) == seq, "the sequence word"
            np.testing.assert_array_equal(h[:out.size], out.reshape(-1), err_msg="the host report carries the floats of out")
            assert (h[out.size:SEQ_WORD] == -7).all() and h[SEQ_WORD + 1] == -7, "a write outside the report"
        assert int(self.counter.item()) == 0, "the arrival counter resets itself"
        return out, self.ws.cpu().numpy().copy(), self.order.cpu().numpy().copy(), self.masked.cpu().numpy().copy()


def check(got, names, s, y_LB, ids_LB, n_docs, topn, max_label, rows=None, what=""):
    """The launch against the restatement; rows: the lists whose values are compared (None: all of them, and the batch means)."""
    out, ws, order, masked = got
    m = N.masked_scores(s, ids_LB, n_docs)
    per, ref_order = M.per_list(m, np.ascontiguousarray(y_LB.T), topn, max_label)
    np.testing.assert_array_equal(masked, m, err_msg="masked scores " + what)
    np.testing.assert_array_equal(order, ref_order, err_msg="order " + what)
    sel = slice(None) if rows is None else rows
    for k, name in enumerate(names):
        ref = per[name]
        scale = np.maximum(1.0, np.abs(ref)) if name in M.UNBOUNDED else np.ones_like(ref)
        err = np.abs(ws[:, k, :] - ref) / scale
        assert err[sel].max() <= PER_LIST_TOL, "per-list %s %s: %g" % (name, what, err[sel].max())
        if rows is None:
            mean = ref.mean(0)
            mscale = np.maximum(1.0, np.abs(mean)) if name in M.UNBOUNDED else 1.0
            merr = np.abs(out[k] - mean) / mscale
            assert merr.max() <= MEAN_TOL, "batch mean %s %s: %g" % (name, what, merr.max())
    return per


def ndcg_report(s, y_LB, ids_LB, n_docs, B, L, topn):
    """ultr_ndcg_report on the same device inputs: (means, per-list, order, masked)."""
    from ultra_pytorch_amd import _lib, hip_ops
    arr = (ctypes.c_int32 * len(topn))(*[int(t) for t in topn])
    out, ws = torch.empty(len(topn), device="cuda"), torch.empty(B, len(topn), device="cuda")
    order, masked = torch.empty(B, L, dtype=torch.int32, device="cuda"), torch.empty(B, L, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _lib.load().ultr_ndcg_report(s.data_ptr(), y_LB.data_ptr(), ids_LB.data_ptr() if ids_LB is not None else None, n_docs, B, L, arr,
                                      len(topn), out.data_ptr(), order.data_ptr(), masked.data_ptr(), ws.data_ptr(), counter.data_ptr(), None,
                                      1, hip_ops.raw_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), ws.cpu().numpy(), order.cpu().numpy(), masked.cpu().numpy()


# a partial last workgroup, one workgroup against many at the counter, the 64-lane chunk boundaries of the scans, the largest list asked
SHAPES = [(1, 1, TOPN_4), (3, 2, TOPN_ODD), (5, 63, TOPN_16), (261, 64, TOPN_4), (261, 65, TOPN_16), (7, 129, TOPN_ODD), (3, 256, TOPN_4),
          (2, 800, TOPN_16)]


@pytest.mark.parametrize("B,L,topn", SHAPES, ids=["B%d_L%d_k%d" % (b, l, len(t)) for b, l, t in SHAPES])
def test_all_metrics_are_the_restatement(B, L, topn):
    s, y, ids = make_inputs(B * 7 + L, B, L)
    args = _dev(s, y, ids)
    got = Launch(B, L, topn).run(*args, 1000)
    check(got, M.NAMES, s, y, ids, 1000, topn, 5.0, what="B=%d L=%d" % (B, L))
    # the NDCG row, the permutation and the masked scores are ultr_ndcg_report's, bit for bit
    r_out, r_ws, r_order, r_masked = ndcg_report(*args, 1000, B, L, topn)
    k = M.IDS["ndcg"]
    np.testing.assert_array_equal(got[0][k], r_out)
    np.testing.assert_array_equal(got[1][:, k, :], r_ws)
    np.testing.assert_array_equal(got[2], r_order)
    np.testing.assert_array_equal(got[3], r_masked)


def test_integer_labels_at_max_label_4():
    B, L = 37, 70
    s, y, ids = make_inputs(3, B, L)
    y = np.floor(y)  # 0 .. 4 and -1: rel <= 15 / 16
    got = Launch(B, L, TOPN_4, max_label=4.0).run(*_dev(s, y, ids), 1000)
    check(got, M.NAMES, s, y, ids, 1000, TOPN_4, 4.0)


def test_subsets_come_back_in_the_order_asked():
    """[MRR, NDCG], [ERR] alone and a permutation of all eight; two batch sizes on ONE arrival counter."""
    L = 65
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    for rep, (B, names) in enumerate([(261, ["mrr", "ndcg"]), (5, ["err"]), (261, list(reversed(M.NAMES))), (3, ["precision", "dcg", "map"])]):
        s, y, ids = make_inputs(100 + rep, B, L)
        args = _dev(s, y, ids)
        got = Launch(B, L, TOPN_ODD, names=names, counter=counter).run(*args, 1000, seq=rep + 1)
        check(got, names, s, y, ids, 1000, TOPN_ODD, 5.0, what="launch %d" % rep)
        full = Launch(B, L, TOPN_ODD).run(*args, 1000)
        for k, name in enumerate(names):  # a row does not depend on which others were asked for
            np.testing.assert_array_equal(got[0][k], full[0][M.IDS[name]])
            np.testing.assert_array_equal(got[1][:, k], full[1][:, M.IDS[name]])


def test_without_a_host_report():
    B, L = 9, 12
    s, y, ids = make_inputs(8, B, L)
    got = Launch(B, L, TOPN_4, report=False).run(*_dev(s, y, ids), 1000)
    check(got, M.NAMES, s, y, ids, 1000, TOPN_4, 5.0)


def test_the_reference_s_recorded_cases():
    """Both cases of tests/golden/metrics_host.npz (the reference's own outputs) through the launch; docids = NULL: the scores are
    masked already."""
    d = np.load(os.path.join(GOLDEN, "metrics_host.npz"))
    meta = json.loads(str(d["meta"]))
    for tag in ("a", "b"):
        s, y = d[tag + "_scores"], d[tag + "_labels"]
        B, L = s.shape
        st, yt = _dev(s, np.ascontiguousarray(y.T))
        out = Launch(B, L, meta["topn"], names=meta["keys"], max_label=meta["max_label"]).run(st, yt, None, 0)[0]
        for k, key in enumerate(meta["keys"]):
            ref = d["%s_%s" % (tag, key)]
            np.testing.assert_allclose(out[k], np.broadcast_to(ref, out[k].shape), rtol=0, atol=1e-6, err_msg=tag + " " + key)


def test_rejects_what_it_cannot_do():
    B, L = 4, 8
    s, y, ids = make_inputs(1, B, L)
    args = _dev(s, y, ids)
    for null in ("scores", "labels", "topn", "ids", "out", "ws", "counter"):
        assert Launch(B, L, TOPN_4).run(*args, 1000, **{null: None}) == ULTR_E_BADARG, null
    assert Launch(B, L, TOPN_4).run(*args, 1000, n_metrics=0) == ULTR_E_BADARG
    assert Launch(B, L, TOPN_4).run(*args, 1000, n_metrics=9) == ULTR_E_BADARG
    assert Launch(B, L, TOPN_4, names=["mrr", 8]).run(*args, 1000) == ULTR_E_BADARG  # an unknown id
    assert Launch(B, L, TOPN_4, names=["mrr", -1]).run(*args, 1000) == ULTR_E_BADARG
    assert Launch(B, L, TOPN_4, names=["mrr", "ndcg", "mrr"]).run(*args, 1000) == ULTR_E_BADARG  # a repeated id
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert Launch(B, L, TOPN_4, max_label=bad).run(*args, 1000) == ULTR_E_BADARG
    assert Launch(B, L, [1, 0, 3]).run(*args, 1000) == ULTR_E_BADARG
    assert Launch(B, L, [1, -2]).run(*args, 1000) == ULTR_E_BADARG
    # five [lists][L] arrays: 1023 documents are beyond 64 KiB of LDS (or, should the launch ever reach that far, right)
    B, L = 3, 1023
    s, y, ids = make_inputs(2, B, L)
    got = Launch(B, L, TOPN_4).run(*_dev(s, y, ids), 1000)
    if not isinstance(got, int):
        check(got, M.NAMES, s, y, ids, 1000, TOPN_4, 5.0)
    else:
        assert got == ULTR_E_UNSUPPORTED


def nan_inputs(B, L, invalid):
    """tests/test_gpu_metrics.py test_ndcg_with_nan_scores' rows; in the rows b % 4 == 0 the NaN documents carry label 0 (with the
    invalid ones, which take the NaN row minimum): there the order among NaNs cannot change a value."""
    rng = np.random.RandomState(B + L + invalid)
    s, y, ids = make_inputs(B * 3 + L, B, L)
    y = np.where(y < 0, 1.0, y).astype(np.float32)
    for b in range(B):
        if b % 4 == 3:
            continue  # rows without NaN in the same launch
        at = rng.choice(L, size=1 + b % 2, replace=False)
        s[b, at] = np.nan
        if b % 4 == 0:
            y[at, b] = 0.0
        if invalid:
            y[rng.choice(L, size=2, replace=False), b] = -1.0
    return s, y, ids


def moot_rows(s, y_LB, ids_LB, n_docs):
    """The lists in which every document whose order key is NaN has the same validated label."""
    prep, lab = N.prepare(N.masked_scores(s, ids_LB, n_docs), np.ascontiguousarray(y_LB.T))
    return np.array([len(set(lab[b][np.isnan(prep[b])].tolist())) <= 1 for b in range(prep.shape[0])])


@pytest.mark.parametrize("invalid", [False, True], ids=["valid_labels", "invalid_labels"])
@pytest.mark.parametrize("B,L", [(8, 12), (261, 65), (5, 130)])
def test_all_metrics_with_nan_scores(B, L, invalid):
    s, y, ids = nan_inputs(B, L, invalid)
    rows = moot_rows(s, y, ids, 1000)
    assert 2 * int(rows.sum()) >= B and np.isnan(s[rows]).any()
    got = Launch(B, L, TOPN_4).run(*_dev(s, y, ids), 1000)
    check(got, M.NAMES, s, y, ids, 1000, TOPN_4, 5.0, rows=rows, what="NaN rows")
    assert (np.sort(got[2], axis=1) == np.arange(L)).all()
    # the batch means are the means of the launch's own per-list values (which lists the restatement vouches for: rows)
    mean = got[1].astype(np.float64).mean(0)
    assert (np.abs(got[0] - mean) / np.maximum(1.0, np.abs(mean)) <= MEAN_TOL).all()


# ---- the plugin: validation() reads every metric from the launch's report -----------------------------------------------------------
class DataSet:
    def __init__(self, feature_size):
        self.feature_size = feature_size


def _algo(F, L, metrics, model="ultra_pytorch_amd.ranking_model.DNN", model_hparams="hidden_layer_sizes=[32, 16]"):
    from ultra_pytorch_amd.utils import find_class
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.IPWrank", "learning_algorithm_hparams": "",
           "ranking_model": model, "ranking_model_hparams": model_hparams, "max_candidate_num": L, "selection_bias_cutoff": min(10, L),
           "metrics": list(metrics), "metrics_topn": [1, 3, 5, 10]}
    return find_class(exp["learning_algorithm"])(DataSet(F), exp)


def _feeds(algo, feats, ids, y, device_feed):
    if device_feed:
        f, i_, y_ = _dev(feats, ids, y)
        return {"device_feed": True, "features": f, "n_docs": feats.shape[0], "docids": i_, "labels": y_, "batch_size": ids.shape[1]}
    feed = {algo.letor_features_name: feats.astype(np.float64)}
    for l in range(ids.shape[0]):
        feed[algo.docid_inputs_name[l]] = ids[l].astype(np.float32)
        feed[algo.labels_name[l]] = y[l].astype(np.float32)
    return feed


def _host_metrics(algo, y, names, topn):
    """utils.metrics on the masked scores of the engine validation() used last."""
    from ultra_pytorch_amd.utils import metrics
    ev = next(reversed(algo._eval_engines.values()))
    masked, lab = ev.masked.cpu(), torch.from_numpy(np.ascontiguousarray(y.T))
    return {"%s_%d" % (name, n): float(v) for name in names
            for n, v in zip(topn, metrics.make_ranking_metric_fn(name, topn)(lab, masked, None))}


def _batch(B, L, F, seed=11):
    from ultra_pytorch_amd import synthetic
    rng = np.random.RandomState(seed)
    feats, ids, y = synthetic.make_batch(rng, B, L, F, clicks=False, n_pad=3)
    y = y.copy()
    y[rng.rand(*y.shape) < 0.1] = -1.0
    return feats, ids, y


@pytest.mark.parametrize("device_feed", [False, True], ids=["host_feed", "device_feed"])
def test_validation_reads_every_metric_without_a_host_copy(device_feed, monkeypatch):
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    B, L, F, names, topn = 64, 20, 24, ["mrr", "ndcg", "err"], [1, 3, 5, 10]
    feats, ids, y = _batch(B, L, F)
    algo = _algo(F, L, names)
    only = _algo(F, L, ["ndcg"])
    only.model.flat_params.copy_(algo.model.flat_params)
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
    ref = _host_metrics(algo, y, names, topn)
    for key, v in ref.items():
        assert abs(summary[key] - v) <= 1e-6, (key, summary[key], v)
    _, scores1, summary1 = only.validation(_feeds(only, feats, ids, y, device_feed))
    assert torch.equal(scores, scores1)
    for n in topn:
        assert summary["ndcg_%d" % n] == summary1["ndcg_%d" % n]


def test_validation_takes_max_label_at_each_call(monkeypatch):
    """The loader sets RankingMetricKey.MAX_LABEL after an engine may exist: ERR follows it from one call to the next."""
    from ultra_pytorch_amd.utils import metrics
    B, L, F, names, topn = 16, 12, 24, ["err", "ordered_pair_accuracy", "map", "arp", "precision", "dcg"], [1, 3, 5, 10]
    feats, ids, y = _batch(B, L, F, seed=3)
    algo = _algo(F, L, names)
    for max_label in (4.0, 6.0):
        monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", max_label)
        summary = dict(algo.validation(_feeds(algo, feats, ids, y, False))[2])
        for key, v in _host_metrics(algo, y, names, topn).items():
            assert abs(summary[key] - v) <= 1e-6 * max(1.0, abs(v)), (key, max_label, summary[key], v)
    assert len(algo._eval_engines) == 1


def test_setrank_validation_reads_every_metric(monkeypatch):
    from tests.hipref import load_golden
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    d, m = load_golden("setrank_tiny")
    names, topn = ["mrr", "ndcg", "err"], [1, 3, 5, 10]
    algo = _algo(m["F"], m["L"], names, model="ultra_pytorch_amd.ranking_model.SetRank.SetRank",
                 model_hparams="d_model=32,num_heads=4,num_layers=2,diff=16")
    y = d["s0_labels"].astype(np.float32)
    _, scores, summary = algo.validation(_feeds(algo, d["s0_features"], d["s0_docids"], y, False))
    assert tuple(scores.shape) == (m["B"], m["L"])
    for key, v in _host_metrics(algo, y, names, topn).items():
        assert abs(summary[key] - v) <= 1e-6, (key, summary[key], v)
