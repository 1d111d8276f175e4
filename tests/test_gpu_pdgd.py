"""PDGD on the GPU: pdgd_loss_kernel through the C ABI (ultr_pdgd_loss, ultr_train_step with ULTR_ALGO_PDGD) against the
reference's own steps (tests/golden/pdgd_*.npz) and the restatement (tests/pdgd_ref.py) - the (B, L) grid, no pairs, the
clipped weight, the NaN overflow regime, the size limit, determinism - then the plugin on every feed, the 20-step online run,
IPWrank on an online batch, and the data-parallel step."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import pdgd_ref as R  # noqa: E402
from tests.hipref import dev, load_golden  # noqa: E402
from tests.test_gpu_parity import gtol  # noqa: E402
from tests.test_gpu_plugins import load_flat  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "ultra_toy_data") + "/"
CASES = ["pdgd_tiny", "pdgd_sgd_tau2", "pdgd_linear", "pdgd_cutoff"]


def _engine(F, hidden, B, L, **kw):
    from ultra_pytorch_amd import engine, hip_ops
    shape = hip_ops.DnnShape(F, hidden or [], "elu")
    return shape, engine.StepEngine(shape, B, L, torch.device("cuda"), algo="pdgd", **kw)


def _loss(scores, labels_MB, docids_MB, n_docs, tau, cutoff):
    """ultr_pdgd_loss alone: (dscores [B, L], loss)."""
    from ultra_pytorch_amd import hip_ops
    B, L = scores.shape
    ws = torch.zeros(hip_ops.loss_workspace_bytes(B, L) // 4 + 1, device="cuda")
    ds = torch.full((B, L), 7.0, device="cuda")
    hip_ops.pdgd_loss(dev(scores, torch.float32), dev(labels_MB, torch.float32), dev(docids_MB, torch.int32), n_docs, tau, cutoff,
                      B, L, ds, ws)
    torch.cuda.synchronize()
    tail = hip_ops.tail_floats(L)
    parts = ws[: hip_ops.loss_part_count(B) * tail].view(-1, tail).cpu().numpy()
    assert not parts[:, 1:].any()
    return ds.cpu().numpy(), float(parts[:, 0].astype(np.float64).sum())


# ---- golden steps ---------------------------------------------------------------------------------------------------------
def _golden(name):
    d, m = load_golden(name)
    kw = dict(learning_rate=m["lr"], max_gradient_norm=m["max_gradient_norm"], sigma=m["tau"], cutoff=m["cutoff"],
              l2_loss=m["l2_loss"], optimizer="sgd" if m["grad_strategy"] == "sgd" else "ada")
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        ids = d[p + "docids"]
        B = ids.shape[1]
        shape, eng = _engine(m["F"], m["hidden"], B, m["M"], **kw)
        feats = d[p + "features"]
        params, state = dev(d[p + "pre_params"]), dev(d[p + "pre_adagrad"])
        f, i, y = dev(feats), dev(ids, torch.int32), dev(d[p + "labels"])
        sc = eng.train_step(params, state, f, feats.shape[0], i, y)
        torch.cuda.synchronize()
        sc = sc.cpu().numpy()
        np.testing.assert_allclose(eng.scores.cpu().numpy(), d[p + "scores"], atol=1e-5, rtol=0, err_msg="scores")
        ref_loss = float(d[p + "loss"])
        assert abs(sc[0] - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (sc[0], ref_loss)
        assert sc[3] == 1.0
        # the reference's pre-clip gradient includes the L2 term: l2_loss * p
        g = eng.grads[: shape.n_params].cpu().numpy() + m["l2_loss"] * d[p + "pre_params"]
        gref = d[p + "grads"]
        np.testing.assert_allclose(g, gref, err_msg="grads", **gtol(gref, name))
        assert abs(sc[1] - float(d[p + "norm"])) <= 1e-5 * max(1.0, float(d[p + "norm"]))
        sel = np.abs(gref) > 1e-6 * max(1.0, float(np.abs(gref).max()))
        # (a warm Adagrad state divides by sqrt(state): relative gradient rounding of small elements reaches ~1e-5 absolute)
        np.testing.assert_allclose(params.cpu().numpy()[sel], d[p + "post_params"][sel], atol=2e-5, rtol=1e-5, err_msg="params")
        if m["grad_strategy"] != "sgd":
            ref_state = d[p + "post_adagrad"]
            np.testing.assert_allclose(state.cpu().numpy(), ref_state, rtol=2e-5, atol=2e-6 * float(ref_state.max()))
        eng.close()


@pytest.mark.parametrize("name", CASES)
def test_golden_train_step(name):
    _golden(name)


def test_golden_train_step_under_both_mfma_plans(mfma_mode):
    _golden("pdgd_tiny")


# ---- the kernel against the restatement -----------------------------------------------------------------------------------
def _rand_case(rng, B, L, scale=2.0, p_pad=0.1):
    n_docs = B * L
    s = (rng.standard_normal((B, L)) * scale).astype(np.float32)
    s[rng.uniform(size=s.shape) < 0.2] = np.float32(0.5)  # ties
    y = (rng.randint(0, 4, size=(L, B)) * (rng.uniform(size=(L, B)) < 0.5)).astype(np.float32)  # graded
    ids = np.arange(n_docs, dtype=np.int32).reshape(L, B)
    ids[rng.uniform(size=ids.shape) < p_pad] = n_docs
    return s, y, ids, n_docs


@pytest.mark.parametrize("B,L", [(3, 1), (5, 2), (7, 10), (4, 63), (3, 64), (3, 65), (2, 130), (2, 256)])
def test_kernel_matches_restatement(B, L):
    rng = np.random.RandomState(B * 1000 + L)
    for tau in (1, 2, 3):
        s, y, ids, n_docs = _rand_case(rng, B, L)
        cutoff = max(1, L - int(rng.randint(0, max(1, L // 3))))
        ds, loss = _loss(s, y, ids, n_docs, tau, cutoff)
        ref_loss, ref_g, pairs = R.pdgd_score_grad(s, y, ids, n_docs, cutoff, tau)
        assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (loss, ref_loss)
        np.testing.assert_allclose(ds, ref_g, rtol=1e-4, atol=1e-6 * max(1.0, np.abs(ref_g).max()))
        assert L < 4 or pairs


def test_no_pairs_gives_zero():
    rng = np.random.RandomState(1)
    s, y, ids, n = _rand_case(rng, 4, 12)
    y[:] = 0
    ds, loss = _loss(s, y, ids, n, 1, 12)
    assert loss == 0.0 and not ds.any()
    y[:] = 2  # every label equal: no pair either
    ds, loss = _loss(s, y, ids, n, 1, 12)
    assert loss == 0.0 and not ds.any()


def test_clipped_weight_and_pad_past_cutoff():
    """One pair whose delta is far above 20 (the weight stops at 1 / (1 + e^20)), and a PAD past the cutoff whose exp-score
    still counts in the suffix sums; relative tolerance only, so a dropped clip or a zeroed PAD is caught."""
    s = np.array([[0.0, -40.0, -45.0, -50.0]], dtype=np.float32)  # swapping positions 0 and 1: delta ~ 40
    y = np.array([[0.0], [1.0], [0.0], [0.0]], dtype=np.float32)
    ids = np.arange(4, dtype=np.int32).reshape(4, 1)
    ds, loss = _loss(s, y, ids, 4, 1, 2)
    ref_loss, ref_g, pairs = R.pdgd_score_grad(s, y, ids, 4, 2, 1)
    assert [(l, k) for _, l, k, _ in pairs] == [(1, 0)] and pairs[0][3] == pytest.approx(1.0 / (1.0 + np.exp(20.0)))
    np.testing.assert_allclose(ds, ref_g, rtol=1e-4, atol=0)
    assert loss == pytest.approx(ref_loss, rel=1e-5)
    ids = np.array([[0], [1], [2], [4]], dtype=np.int32)  # position 3 is a PAD (n_docs = 4), past the cutoff 3
    # a non-trivial weight that depends on the PAD past the cutoff
    s = np.array([[0.0, -0.5, 0.2, 1.5]], dtype=np.float32)
    ds, loss = _loss(s, y, ids, 4, 1, 3)
    ref_loss, ref_g, _ = R.pdgd_score_grad(s, y, ids, 4, 3, 1)
    np.testing.assert_allclose(ds, ref_g, rtol=1e-5, atol=0)


def test_overflow_gives_nan():
    s = np.array([[100.0, 0.0, 1.0]], dtype=np.float32)  # exp(100) overflows in fp32
    y = np.array([[1.0], [0.0], [0.0]], dtype=np.float32)
    ids = np.arange(3, dtype=np.int32).reshape(3, 1)
    ds, loss = _loss(s, y, ids, 3, 1, 3)
    assert np.isnan(ds[0, 0]) and np.isnan(loss)


def test_refuses_lists_beyond_256():
    from ultra_pytorch_amd import _lib
    with pytest.raises(_lib.UltrHipError):
        _loss(np.zeros((1, 257), np.float32), np.zeros((257, 1), np.float32), np.zeros((257, 1), np.int32), 1, 1, 257)


def test_step_is_bitwise_deterministic():
    rng = np.random.RandomState(5)
    F, hidden, B, L = 24, [32, 16], 32, 40
    from oracle import ultr_oracle as O
    p0 = O.init_params(F, hidden, seed=3)
    s, y, ids, n = _rand_case(rng, B, L)
    feats = dev(rng.uniform(-1, 1, size=(n, F)).astype(np.float32))
    outs = []
    for _ in range(2):
        shape, eng = _engine(F, hidden, B, L, cutoff=30, l2_loss=0.005, max_gradient_norm=1.0)
        p, st = dev(p0), torch.full((p0.size,), 0.1, device="cuda")
        for _ in range(3):
            sc = eng.train_step(p, st, feats, n, dev(ids, torch.int32), dev(y))
        torch.cuda.synchronize()
        outs.append((sc.cpu().numpy().copy(), p.cpu().numpy(), st.cpu().numpy(), eng.dscores.cpu().numpy()))
        eng.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ---- the plugin ----------------------------------------------------------------------------------------------------------
class DS:
    def __init__(self, n_queries, M, F, seed, pads=True):
        rng = np.random.RandomState(seed)
        self.feature_size, self.features, self.initial_list, self.labels, self.dids, self.qids = F, [], [], [], [], []
        did = 0
        for q in range(n_queries):
            n = int(rng.randint(2, M + 1)) if pads else M
            self.features += rng.uniform(-1, 1, size=(n, F)).astype(np.float32).tolist()
            self.initial_list.append(list(range(did, did + n)) + [-1] * (M - n))
            lab = rng.randint(0, 5, size=M)
            lab[0] = max(lab[0], 1)
            self.labels.append([int(v) for v in lab])
            self.dids += ["d%d" % i for i in range(did, did + n)]
            self.qids.append("q%d" % q)
            did += n
        self.rank_list_size = M


def make_algo(F, M, cutoff, hidden, hp="", model="DNN", algo="PDGD"):
    from ultra_pytorch_amd.utils import find_class
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm." + algo, "learning_algorithm_hparams": hp,
           "ranking_model": "ultra_pytorch_amd.ranking_model." + model,
           "ranking_model_hparams": "hidden_layer_sizes=%s" % json.dumps(hidden) if hidden else "",
           "max_candidate_num": M, "selection_bias_cutoff": cutoff, "metrics": ["ndcg"], "metrics_topn": [1, 3]}
    return find_class(exp["learning_algorithm"])(DS(1, M, F, 0), exp)


def _arrays(algo, feed, M):
    if feed.get("device_feed", False):
        return (feed["features"].cpu().numpy().copy(), feed["docids"].cpu().numpy().astype(np.int64),
                feed["labels"].cpu().numpy().copy())
    feats = np.asarray(feed["letor_features"], np.float32)
    ids = np.stack([np.asarray(feed[algo.docid_inputs_name[l]]) for l in range(M)]).astype(np.int64)
    y = np.stack([np.asarray(feed[algo.labels_name[l]]) for l in range(M)]).astype(np.float32)
    return feats, ids, y


@pytest.mark.parametrize("feed_name", ["ClickSimulationFeed", "DeviceClickFeed", "StochasticOnlineSimulationFeed",
                                       "DeterministicOnlineSimulationFeed"])
def test_plugin_on_every_feed(feed_name, capsys):
    from ultra_pytorch_amd import input_layer
    F, M, hidden = 24, 10, [16, 8]
    online = "Online" in feed_name
    cutoff = 7 if online else M
    algo = make_algo(F, M, cutoff, hidden)
    ds = DS(64, M, F, seed=4, pads=online)
    feed = input_layer.DeviceClickFeed(algo, 16, "", seed=3) if feed_name == "DeviceClickFeed" else \
        getattr(input_layer, feed_name)(algo, 16, "")
    random.seed(1)
    np.random.seed(1)
    algo.state_sum.fill_(0.1)  # warm Adagrad state: the first update is lr * sign(g) from zero
    for step in range(2):
        input_feed, _ = feed.get_batch(ds, check_validation=True)
        feats, ids, y = _arrays(algo, input_feed, ids_len(input_feed, M))
        p0, s0 = algo.model.flat_params.cpu().numpy().copy(), algo.state_sum.cpu().numpy().copy()
        capsys.readouterr()
        loss, out, summary = algo.train(input_feed)
        assert out is None and isinstance(summary, dict)
        assert " Loss %f at Global Step %d: " % (loss, step + 1) in capsys.readouterr().out  # after the increment, as there
        ref = R.pdgd_step(p0, s0, F, hidden, feats, ids, y, cutoff, 1, 0.05, 1.0, 0.005, "ada")
        assert abs(loss - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"]))
        np.testing.assert_allclose(algo.model.flat_params.cpu().numpy(), ref["params"], atol=5e-6, rtol=1e-5)
    assert algo.global_step == 2


def ids_len(feed, M):
    return int(feed["docids"].shape[0]) if feed.get("device_feed", False) else M


def test_plugin_refuses_setrank():
    from ultra_pytorch_amd.utils import find_class
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.PDGD", "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.SetRank.SetRank",
           "ranking_model_hparams": "d_model=32,num_heads=4,num_layers=1,diff=16", "max_candidate_num": 10,
           "selection_bias_cutoff": 10, "metrics": ["ndcg"], "metrics_topn": [1]}
    with pytest.raises(NotImplementedError, match="two-document"):
        find_class(exp["learning_algorithm"])(DS(1, 10, 24, 0), exp)


# ---- online runs ----------------------------------------------------------------------------------------------------------
def _toy_algo(m, algo="PDGD"):
    from ultra_pytorch_amd import utils
    ds = utils.read_data(DATA, "train")
    ds.pad(m["M"])
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm." + algo, "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=%s" % json.dumps(m["hidden"]),
           "max_candidate_num": m["M"], "selection_bias_cutoff": m["cutoff"], "metrics": ["ndcg"], "metrics_topn": [1, 3, 5]}
    from ultra_pytorch_amd.utils import find_class
    return find_class(exp["learning_algorithm"])(ds, exp), ds


def test_online_run_matches_reference():
    """20 steps of PDGD + StochasticOnlineSimulationFeed: the same re-rankings and clicks at every step (the Plackett-Luce draw
    reads the GPU's scores), losses within 1e-5 relative, final parameters at the golden tolerance."""
    from ultra_pytorch_amd.input_layer import StochasticOnlineSimulationFeed
    d, m = load_golden("pdgd_online")
    algo, ds = _toy_algo(m)
    load_flat(algo.model, d["init_params"])
    random.seed(m["seed"])
    np.random.seed(m["seed"])
    feed = StochasticOnlineSimulationFeed(algo, m["B"], "")
    for t in range(m["n_steps"]):
        f, info = feed.get_batch(ds, check_validation=True)
        np.testing.assert_array_equal(info["rank_list_idxs"], d["s%d_idxs" % t])
        _, ids, y = _arrays(algo, f, m["M"])
        np.testing.assert_array_equal(ids, d["s%d_docids" % t], err_msg="step %d" % t)
        np.testing.assert_array_equal(y, d["s%d_labels" % t], err_msg="step %d" % t)
        loss, _, _ = algo.train(f)
        assert abs(loss - d["losses"][t]) <= 1e-5 * max(1.0, abs(d["losses"][t])), (t, loss, d["losses"][t])
    # Adagrad turns the rounding of near-zero gradient elements into O(lr) moves: a handful of weights drift, the rest agree
    got, want = algo.model.flat_params.cpu().numpy(), d["final_params"]
    off = ~np.isclose(got, want, atol=5e-5, rtol=1e-4)
    assert off.mean() <= 0.01 and np.abs(got - want).max() <= 0.05, (off.sum(), np.abs(got - want).max())


def test_ipw_step_on_an_online_batch():
    from ultra_pytorch_amd.input_layer import StochasticOnlineSimulationFeed
    d, m = load_golden("pdgd_ipw_online")
    algo, ds = _toy_algo(m, algo="IPWrank")
    load_flat(algo.model, d["pre_params"])
    random.seed(m["seed"])
    np.random.seed(m["seed"])
    f, _ = StochasticOnlineSimulationFeed(algo, m["B"], "").get_batch(ds, check_validation=True)
    _, ids, y = _arrays(algo, f, m["M"])
    np.testing.assert_array_equal(ids, d["docids"])
    np.testing.assert_array_equal(y, d["labels"])
    loss, _, _ = algo.train(f)
    assert abs(loss - float(d["loss"])) <= 1e-5 * max(1.0, abs(float(d["loss"])))
    got = algo.model.flat_params.cpu().numpy()
    # Adagrad's first step moves every weight by +-lr: where the gradient is rounding noise its sign may differ
    off = ~np.isclose(got, d["post_params"], atol=5e-6, rtol=1e-5)
    lr = algo.learning_rate
    # (|g| near Adagrad's eps moves a weight by less than lr: the output bias, whose softmax gradient is exactly zero in theory)
    flips = (np.abs(got - d["pre_params"]) <= lr * 1.001) & (np.abs(d["post_params"] - d["pre_params"]) <= lr * 1.001)
    assert off.mean() <= 0.01 and (flips | ~off).all()


# ---- data parallel --------------------------------------------------------------------------------------------------------
DP_F, DP_HIDDEN, DP_B, DP_L = 24, [32, 16], 7, 9  # 7 lists -> shards of 4 and 3


def _dp_global():
    rng = np.random.RandomState(3)
    s, y, ids, n = _rand_case(rng, DP_B, DP_L)
    feats = rng.uniform(-1, 1, size=(n, DP_F)).astype(np.float32)
    return feats, ids, y


def _dp_run(feats, ids, y, pg):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine, hip_ops
    d = torch.device("cuda", torch.cuda.current_device())
    params = O.init_params(DP_F, DP_HIDDEN, seed=5)
    shape = hip_ops.DnnShape(DP_F, DP_HIDDEN, "elu")
    eng = engine.StepEngine(shape, ids.shape[1], DP_L, d, algo="pdgd", process_group=pg, cutoff=7, l2_loss=0.005,
                            max_gradient_norm=1.0)
    p, st = torch.tensor(params, device=d), torch.full((params.shape[0],), 0.01, device=d)
    f, i, yy = torch.tensor(feats, device=d), torch.tensor(ids, device=d), torch.tensor(y, device=d)
    losses = []
    for _ in range(2):
        sc = eng.train_step(p, st, f, feats.shape[0], i, yy)
        torch.cuda.synchronize()
        losses.append(float(sc[0]))
    out = dict(params=p.cpu().numpy(), state=st.cpu().numpy(), losses=losses)
    eng.close()
    return out


def _dp_worker(rank, world, port, mode, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      ULTR_DP_COMM=mode, HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from ultra_pytorch_amd import parallel
    torch.cuda.set_device(0)
    _, _, _, pg = parallel.init_process_group_from_env(backend="gloo")
    feats, ids, y = _dp_global()
    lo, hi = parallel.shard_bounds(DP_B, rank, world)
    q.put((rank, _dp_run(feats, ids[:, lo:hi].copy(), y[:, lo:hi].copy(), pg)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["peer", "pg"])
def test_two_rank_step_equals_single_process(mode):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29890 + (0 if mode == "peer" else 1)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, mode, q)) for r in range(2)]  # 2 rank processes (<= 5)
    [p.start() for p in procs]
    got = dict(q.get(timeout=300) for _ in range(2))
    [p.join(120) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    one = _dp_run(*_dp_global(), None)
    for rank in (0, 1):
        res = got[rank]
        assert np.array_equal(res["params"], got[0]["params"])
        np.testing.assert_allclose(res["losses"], one["losses"], rtol=1e-6)
        np.testing.assert_allclose(res["params"], one["params"], rtol=1e-6, atol=1e-6 * np.abs(one["params"]).max())
        np.testing.assert_allclose(res["state"], one["state"], rtol=2e-5, atol=1e-12)
