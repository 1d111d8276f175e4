"""Evaluation of a resident dataset on the GPU (csrc/ultr_eval.hip, engine.EvalSetEngine, BaseAlgorithm.validation_set,
input_layer.DeviceDirectLabelFeed): the sequential pick against a numpy restatement (exact), the accumulate against
utils.merge_Summary (`==` on float64), a whole set against the per-batch loop it replaces (bit for bit) and against the host
DirectLabelFeed loop (1e-6, the bar of tests/test_gpu_metrics_all.py), the random batches of the feed, and the driver with the
device feed as its valid / test feed against the same run with the host feed."""
import copy
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATA = os.path.join(GOLDEN, "ultra_toy_data") + "/"


class DS:
    """A padded Raw_data look-alike: ragged lists of 2 .. M documents with PAD tails (-1), the all-zero PAD feature row that
    Raw_data.pad appends, labels 0 .. 4 (ragged, as the loader leaves them)."""

    def __init__(self, n_queries, M, F, seed, zero_lists=()):
        rng = np.random.RandomState(seed)
        self.feature_size, self.features, self.initial_list, self.labels, self.dids, self.qids = F, [], [], [], [], []
        did = 0
        for q in range(n_queries):
            n = int(rng.randint(2, M + 1))
            self.features += rng.uniform(-1, 1, size=(n, F)).astype(np.float32).tolist()
            self.initial_list.append(list(range(did, did + n)) + [-1] * (M - n))
            lab = rng.randint(0, 5, size=n)
            if q in zero_lists:
                lab[:] = 0
            self.labels.append([int(v) for v in lab])
            self.dids += ["d%d" % i for i in range(did, did + n)]
            self.qids.append("q%d" % q)
            did += n
        self.features.append([0.0] * F)
        self.rank_list_size = M


class Lists:
    """Just enough of a dataset for ResidentDataset: explicit lists and labels over n_docs one-float documents."""

    def __init__(self, lists, labels, n_docs):
        self.features = [[float(i)] for i in range(n_docs)]
        self.dids = ["d%d" % i for i in range(n_docs)]
        self.initial_list, self.labels = [list(map(int, r)) for r in lists], [list(map(float, r)) for r in labels]


# ---- the sequential pick -------------------------------------------------------------------------------------------------------------
def pick_ref(lists, labels, n_docs, start, B, L):
    """DirectLabelFeed.prepare_true_labels_with_index with global ids: the entry, or n_docs (label 0) at a PAD or past the row."""
    lmax = lists.shape[1]
    ids, y = np.full((L, B), n_docs, np.int32), np.zeros((L, B), np.float32)
    for b in range(B):
        for l in range(min(L, lmax)):
            if lists[start + b, l] >= 0:
                ids[l, b], y[l, b] = lists[start + b, l], labels[start + b, l]
    return ids, y


def _resident(lmax, n_docs=500, seed=3):
    from ultra_pytorch_amd.input_layer import ResidentDataset
    rng = np.random.RandomState(seed + lmax)
    lists = rng.randint(0, n_docs, size=(11, lmax))
    lens = rng.randint(1, lmax + 1, size=11)
    lens[0] = lmax
    lists[np.arange(lmax)[None, :] >= lens[:, None]] = -1
    lists[1, 0] = -1                 # a leading PAD
    lists[2, min(1, lmax - 1)] = -1  # an interior PAD
    lists[3, 0] = n_docs + 5         # an id beyond the documents: -1 after the upload
    lists[10, lmax - 1] = n_docs     # ... and the first such id, in the last row's last entry
    labels = rng.randint(1, 5, size=(11, lmax)).astype(np.float32)  # non-zero everywhere: a PAD's label must come back as 0
    rd = ResidentDataset(Lists(lists, labels, n_docs), torch.device("cuda"))
    up = rd.lists.cpu().numpy()
    assert rd.n_docs == n_docs and rd.lmax == lmax and up[3, 0] == -1 and up[10, lmax - 1] == -1 and up[0, 0] == lists[0, 0]
    return rd, up, labels


def run_pick(rd, start, B, L, with_idx):
    from ultra_pytorch_amd import _lib
    ids = torch.full((L, B), -7, dtype=torch.int32, device="cuda")  # sentinels: every element must be written
    y = torch.full((L, B), -7.0, device="cuda")
    q = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.load().ultr_eval_pick(rd.lists.data_ptr(), rd.labels.data_ptr(), rd.n_queries, rd.lmax, rd.n_docs, start, B, L,
                                    ids.data_ptr(), y.data_ptr(), q.data_ptr() if with_idx else None, None)
    torch.cuda.synchronize()
    assert rc == 0
    return ids.cpu().numpy(), y.cpu().numpy(), q.cpu().numpy()


@pytest.mark.parametrize("lmax,start,B,L", [(7, 0, 4, 7), (7, 8, 3, 7), (7, 10, 1, 7), (7, 0, 5, 5), (7, 2, 6, 9), (7, 0, 11, 1),
                                            (130, 0, 5, 130), (130, 6, 5, 130)])
def test_pick_is_the_restatement(lmax, start, B, L):
    rd, lists, labels = _resident(lmax)
    want_ids, want_y = pick_ref(lists, labels, rd.n_docs, start, B, L)
    assert (want_ids == rd.n_docs).any() and (want_ids != rd.n_docs).any()
    for with_idx in (True, False):
        ids, y, q = run_pick(rd, start, B, L, with_idx)
        np.testing.assert_array_equal(ids, want_ids)
        np.testing.assert_array_equal(y, want_y)
        np.testing.assert_array_equal(q, np.arange(start, start + B) if with_idx else np.full(B, -7))


# ---- the accumulate ------------------------------------------------------------------------------------------------------------------
def _means(rng, n):
    m = rng.uniform(0, 1, size=n).astype(np.float32)
    special = np.array([0.0, 1.0, 1e-45, 1.1e-38, 5e-39, np.float32(1) - np.float32(2) ** -24], np.float32)  # 0, 1, denormals, 1 - ulp
    k = rng.randint(0, n, size=min(n, len(special)))
    m[k] = special[:len(k)]
    return m


@pytest.mark.parametrize("chunks", [(5, 5, 2), (1,), (256, 256, 256, 7)])
@pytest.mark.parametrize("n", [1, 6, 128])
def test_accumulate_is_merge_summary(chunks, n):
    from ultra_pytorch_amd import _lib
    from ultra_pytorch_amd.utils import merge_Summary
    lib = _lib.load()
    rng = np.random.RandomState(1000 * n + len(chunks))
    acc = torch.full((n + 1,), 12345.0, dtype=torch.float64, device="cuda")  # garbage: ULTR_EVAL_RESET must not read it
    hs = torch.zeros(_lib.EVAL_SEQ_BYTE // 8 + 1, dtype=torch.float64).pin_memory()
    hs_d = hs.numpy()
    hs_u = hs_d.view(np.uint32)
    for run in (1, 2):  # the second run reuses the accumulator: the reset
        means = [_means(rng, n) for _ in chunks]
        dev = [torch.from_numpy(m).cuda() for m in means]
        for j, (m, b) in enumerate(zip(dev, chunks)):
            flags = (_lib.EVAL_RESET if j == 0 else 0) | (_lib.EVAL_FINISH if j == len(chunks) - 1 else 0)
            assert lib.ultr_eval_accumulate(m.data_ptr(), n, b, acc.data_ptr(), flags, hs.data_ptr(), run, None) == 0
            if j < len(chunks) - 1:
                assert int(hs_u[_lib.EVAL_SEQ_BYTE // 4]) == run - 1  # the report is written by the finishing launch only
        torch.cuda.synchronize()
        assert int(hs_u[_lib.EVAL_SEQ_BYTE // 4]) == run
        want = merge_Summary([{i: float(m[i]) for i in range(n)} for m in means], list(chunks))
        got = hs_d[:n].copy()
        for i in range(n):
            assert got[i] == want[i], (i, got[i], want[i])
        assert hs_d[128] == float(sum(chunks))
        a = acc.cpu().numpy()
        assert a[n] == float(sum(chunks))
        total = np.zeros(n)
        for m, b in zip(means, chunks):
            total = total + m.astype(np.float64) * b
        np.testing.assert_array_equal(a[:n], total)


# ---- a whole set ---------------------------------------------------------------------------------------------------------------------
TOPN = [1, 3, 10]
NAMES = ["mrr", "ndcg", "err"]


def _algo(F, L, metrics, model, model_hparams):
    from ultra_pytorch_amd.utils import find_class
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.IPWrank", "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model." + model, "ranking_model_hparams": model_hparams, "max_candidate_num": L,
           "selection_bias_cutoff": min(10, L), "metrics": list(metrics), "metrics_topn": list(TOPN)}
    return find_class(exp["learning_algorithm"])(DS(1, L, F, 0), exp)


def per_batch_loop(algo, feed, ds, keep_ws=False):
    """What main.validate_model / main.test do: get_next_batch + validation() per batch, utils.merge_Summary at the end."""
    from ultra_pytorch_amd.utils import merge_Summary
    it, summaries, sizes, rows, ws = 0, [], [], [], []
    while it < len(ds.initial_list):
        input_feed, info_map = feed.get_next_batch(it, ds, check_validation=False)
        _, out, summary = algo.validation(input_feed)
        summaries.append(copy.deepcopy(summary))
        sizes.append(len(info_map["input_list"]))
        rows.append(out[:sizes[-1]].clone())
        if keep_ws:
            ev = next(reversed(algo._eval_engines.values()))
            ws.append(ev.metric_ws.clone())
        it += sizes[-1]
    return merge_Summary(summaries, sizes), torch.cat(rows), (torch.cat(ws) if keep_ws else None), sizes


@pytest.mark.parametrize("model,hp,F", [("DNN", "hidden_layer_sizes=[32, 16]", 136), ("DNN", "hidden_layer_sizes=[32, 16]", 13),
                                        ("Linear", "", 136), ("Linear", "", 13)])
def test_whole_set_is_the_per_batch_loop(model, hp, F, monkeypatch):
    from ultra_pytorch_amd import input_layer
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    L, B = 12, 8
    ds = DS(37, L, F, seed=5)
    algo = _algo(F, L, NAMES, model, hp)
    dfeed = input_layer.DeviceDirectLabelFeed(algo, B, "")
    want, want_scores, want_ws, sizes = per_batch_loop(algo, dfeed, ds, keep_ws=True)
    assert sizes == [8, 8, 8, 8, 5]
    summary, scores, pq = algo.validation_set(dfeed, ds, want_scores=True, per_query=True)
    assert list(summary) == ["%s_%d" % (m, n) for m in NAMES for n in TOPN] and set(want) == set(summary)
    for k in summary:
        assert summary[k] == want[k], (k, summary[k], want[k])            # (a)
    assert tuple(scores.shape) == (37, L) and torch.equal(scores, want_scores)  # (b) bitwise
    assert tuple(pq.shape) == (37, len(NAMES), len(TOPN)) and torch.equal(pq, want_ws)  # (c) bitwise
    again = algo.validation_set(dfeed, ds)  # without the optional outputs: the per-chunk workspaces
    assert again[0] == summary and again[1] is None and again[2] is None
    # (d) the host feed's loop (batch-local feature copies, staged per batch)
    host, host_scores, _, hsizes = per_batch_loop(algo, input_layer.DirectLabelFeed(algo, B, ""), ds)
    assert hsizes == sizes
    worst = max(abs(summary[k] - host[k]) for k in host)
    print("device set vs host DirectLabelFeed loop: largest metric difference %.3g, largest score difference %.3g"
          % (worst, float((scores - host_scores).abs().max())))
    for k in host:
        assert abs(summary[k] - host[k]) <= 1e-6, (k, summary[k], host[k])


def test_whole_set_setrank(monkeypatch):
    from ultra_pytorch_amd import input_layer
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    L, B, F = 12, 8, 24
    ds = DS(37, L, F, seed=6)
    algo = _algo(F, L, NAMES, "SetRank.SetRank", "d_model=32,num_heads=2,num_layers=1,diff=16")
    dfeed = input_layer.DeviceDirectLabelFeed(algo, B, "")
    want, want_scores, _, sizes = per_batch_loop(algo, dfeed, ds)
    summary, scores, pq = algo.validation_set(dfeed, ds, want_scores=True, per_query=True)
    assert set(want) == set(summary)
    for k in summary:
        assert summary[k] == want[k], (k, summary[k], want[k])  # (a)
    assert torch.equal(scores, want_scores)                     # (b)
    assert tuple(pq.shape) == (37, len(NAMES), len(TOPN))


def test_ndcg_only_is_the_per_batch_loop(monkeypatch):
    """["ndcg"] alone: validation() takes the NDCG launch, the set takes the metric launch - the same arithmetic, the same bits."""
    from ultra_pytorch_amd import input_layer
    L, B, F = 12, 8, 136
    ds = DS(37, L, F, seed=7)
    algo = _algo(F, L, ["ndcg"], "DNN", "hidden_layer_sizes=[32, 16]")
    dfeed = input_layer.DeviceDirectLabelFeed(algo, B, "")
    want, want_scores, _, _ = per_batch_loop(algo, dfeed, ds)
    summary, scores, _ = algo.validation_set(dfeed, ds, want_scores=True)
    assert summary == want and torch.equal(scores, want_scores)


def test_fallback_keeps_the_per_batch_loop(monkeypatch):
    """A metric key outside the launch's table: validation_set walks the batches as the driver does, with the same figures."""
    from ultra_pytorch_amd import engine, input_layer
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    monkeypatch.delitem(engine.METRIC_IDS, "err")  # "err" is outside the table now: utils.metrics computes it on the host
    L, B, F = 12, 8, 13
    ds = DS(21, L, F, seed=8)
    algo = _algo(F, L, ["ndcg", "err"], "DNN", "hidden_layer_sizes=[32, 16]")
    called = []
    monkeypatch.setattr(engine.EvalSetEngine, "run", lambda *a, **k: called.append(1))
    for feed in (input_layer.DeviceDirectLabelFeed(algo, B, ""), input_layer.DirectLabelFeed(algo, B, "")):
        want, want_scores, _, _ = per_batch_loop(algo, feed, ds)
        summary, scores, pq = algo.validation_set(feed, ds, want_scores=True, per_query=True)
        assert summary == want and torch.equal(scores, want_scores) and pq is None
    assert not called


# ---- the feed's random batches -------------------------------------------------------------------------------------------------------
def test_get_batch_draws_labelled_queries_reproducibly():
    from ultra_pytorch_amd import input_layer
    L, B, F = 12, 16, 13
    zero = (0, 3, 4, 9, 17)
    ds = DS(23, L, F, seed=9, zero_lists=zero)
    algo = _algo(F, L, ["ndcg"], "DNN", "hidden_layer_sizes=[32, 16]")
    feed = input_layer.DeviceDirectLabelFeed(algo, B, "", seed=11)
    rd = feed.resident(ds)
    lists, labels = rd.lists.cpu().numpy(), rd.labels.cpu().numpy()
    seen, batches = set(), []
    for t in range(6):
        input_feed, info = feed.get_batch(ds, check_validation=True)
        torch.cuda.synchronize()
        ids, y, q = input_feed["docids"].cpu().numpy(), input_feed["labels"].cpu().numpy(), info["rank_list_idxs"].cpu().numpy()
        assert ids.shape == (L, B) and y.shape == (L, B) and q.shape == (B,) and input_feed["batch_size"] == B
        assert len(info["input_list"]) == B and input_feed["device_feed"] and input_feed["features"] is rd.features
        assert not set(q.tolist()) & set(zero) and (y.sum(0) != 0).all()
        for b in range(B):  # the resident labels and documents of rank_list_idxs
            want_ids, want_y = pick_ref(lists, labels, rd.n_docs, int(q[b]), 1, L)
            np.testing.assert_array_equal(ids[:, b], want_ids[:, 0])
            np.testing.assert_array_equal(y[:, b], want_y[:, 0])
        seen |= set(q.tolist())
        batches.append((ids, y, q))
    assert len(seen) > B // 2  # not one query over and over
    assert any(not np.array_equal(batches[0][2], b[2]) for b in batches[1:])  # the counter moves the draw
    twin = input_layer.DeviceDirectLabelFeed(algo, B, "", seed=11)
    for t in range(2):
        input_feed, info = twin.get_batch(ds, check_validation=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(input_feed["docids"].cpu().numpy(), batches[t][0])
        np.testing.assert_array_equal(info["rank_list_idxs"].cpu().numpy(), batches[t][2])
    other = input_layer.DeviceDirectLabelFeed(algo, B, "", seed=12).get_batch(ds, check_validation=True)[1]["rank_list_idxs"]
    assert not np.array_equal(other.cpu().numpy(), batches[0][2])
    q_all = feed.get_batch(ds, check_validation=False)[1]["rank_list_idxs"].cpu().numpy()  # unfiltered: any query
    assert ((q_all >= 0) & (q_all < 23)).all()
    # training takes the batch as it is
    loss, _, _ = algo.train(feed.get_batch(ds, check_validation=True)[0])
    assert np.isfinite(loss)


def test_get_batch_refuses_lists_the_online_pick_does_not_take():
    from ultra_pytorch_amd import input_layer
    L, F = 300, 13
    algo = _algo(F, L, ["ndcg"], "Linear", "")
    ds = DS(3, L, F, seed=10)
    feed = input_layer.DeviceDirectLabelFeed(algo, 2, "")
    with pytest.raises(NotImplementedError):
        feed.get_batch(ds)
    input_feed, info = feed.get_next_batch(2, ds)  # the sequential pick has no such limit
    torch.cuda.synchronize()
    assert tuple(input_feed["docids"].shape) == (L, 1) and len(info["input_list"]) == 1
    rd = feed.resident(ds)
    want_ids, want_y = pick_ref(rd.lists.cpu().numpy(), rd.labels.cpu().numpy(), rd.n_docs, 2, 1, L)
    np.testing.assert_array_equal(input_feed["docids"].cpu().numpy(), want_ids)
    np.testing.assert_array_equal(input_feed["labels"].cpu().numpy(), want_y)
    one, _ = feed.get_data_by_index(ds, 0)
    assert tuple(one["labels"].shape) == (L, 1)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def _drive(tmp_path, tag, eval_feed, seed):
    from ultra_pytorch_amd import main as driver
    d = os.path.join(str(tmp_path), tag)
    os.makedirs(d)
    s = {"train_input_feed": "ultra_pytorch_amd.input_layer.DirectLabelFeed", "train_input_hparams": "",
         "valid_input_feed": "ultra_pytorch_amd.input_layer." + eval_feed, "valid_input_hparams": "",
         "test_input_feed": "ultra_pytorch_amd.input_layer." + eval_feed, "test_input_hparams": "",
         "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=[32,16]",
         "learning_algorithm": "ultra_pytorch_amd.learning_algorithm.NavieAlgorithm", "learning_algorithm_hparams": "",
         "metrics": ["err", "ndcg"], "metrics_topn": [1, 3, 5, 10], "objective_metric": "ndcg_10"}
    sf = os.path.join(d, "settings.json")
    json.dump(s, open(sf, "w"))
    argv = ["--data_dir", DATA, "--setting_file", sf, "--model_dir", d + "/model/", "--output_dir", d + "/out/", "--batch_size", "4",
            "--max_train_iteration", "20", "--steps_per_checkpoint", "10", "--test_while_train", "True"]
    random.seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    _, history = driver.main(argv)
    summary = driver.main(argv + ["--test_only", "True"])
    runs = {}
    for line in open(os.path.join(d, "out", "test.ranklist")):
        qid, _, did, rank, score, _ = line.split()
        runs.setdefault(qid, []).append((did, float(score)))
    return history, summary, runs


def test_driver_with_the_device_feed_is_the_driver_with_the_host_feed(tmp_path):
    seed = 0
    h_host, s_host, r_host = _drive(tmp_path, "host", "DirectLabelFeed", seed)
    # precondition: the host run orders no two documents of a list on a gap that the 1e-6 score bar could flip
    gap = min(a[1] - b[1] for rows in r_host.values() for a, b in zip(rows, rows[1:]))
    print("smallest within-list score gap of the host-feed run: %.3g" % gap)
    assert gap > 1e-4, gap
    h_dev, s_dev, r_dev = _drive(tmp_path, "device", "DeviceDirectLabelFeed", seed)
    assert [h[0] for h in h_dev] == [h[0] for h in h_host] == [10, 20, 30]
    for (_, loss_h, m_h), (_, loss_d, m_d) in zip(h_host, h_dev):
        assert abs(loss_d - loss_h) <= 1e-6 and list(m_d) == list(m_h)  # evaluation does not touch the training trajectory
        for k in m_h:
            assert abs(m_d[k] - m_h[k]) <= 1e-6, (k, m_d[k], m_h[k])
    assert set(s_dev) == set(s_host)
    for k in s_host:
        assert abs(s_dev[k] - s_host[k]) <= 1e-6, (k, s_dev[k], s_host[k])
    assert list(r_dev) == list(r_host)
    for qid in r_host:
        assert [d for d, _ in r_dev[qid]] == [d for d, _ in r_host[qid]], qid
        for (_, a), (_, b) in zip(r_dev[qid], r_host[qid]):
            assert abs(a - b) <= 1e-6, (qid, a, b)
