"""PRSrank on the GPU: prs_loss_kernel through the C ABI (ultr_prs_loss, ultr_train_step with ULTR_ALGO_PRS) against the
reference's own steps (tests/golden/prs_*.npz) and against the restatement (tests/prs_ref.py) - ordinary lists, ties, lists
without clicks, zero and short IPW tables, the saturated regime and its NaN edge, the LDS limit - then a full-size step, the
plugin class, and the data-parallel step."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import prs_ref  # noqa: E402
from tests.hipref import HipRun, dev, load_golden  # noqa: E402
from tests.test_gpu_parity import gtol  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DNN_CASES = ["prs_tiny", "prs_odd", "prs_sgd", "prs_l50"]


# ---- golden steps ---------------------------------------------------------------------------------------------------------
def _check_update(d, m, p, name, gs, tail, sc, params, state2):
    ref_loss = float(d[p + "loss"])
    assert abs(sc[0] - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (sc[0], ref_loss)
    assert abs(sc[3] - tail[1]) <= 1e-6 * abs(tail[1])
    assert abs(sc[1] - float(d[p + "norm"])) <= 1e-5 * max(1.0, float(d[p + "norm"]))
    gref = d[p + "grads"]
    sel = np.abs(gref) > 1e-6 * max(1.0, float(np.abs(gref).max()))
    np.testing.assert_allclose(params[sel], d[p + "post_params"][sel], atol=5e-6, rtol=1e-5, err_msg="params")
    if m["grad_strategy"] != "sgd":
        ref_state = d[p + "post_adagrad"]
        np.testing.assert_allclose(state2, ref_state, rtol=4e-5 if name.endswith("_odd") else 2e-5,
                                   atol=2e-6 * float(ref_state.max()))


def _golden_dnn_step(name):
    d, m = load_golden(name)
    kw = dict(learning_rate=m["lr"], max_gradient_norm=m["max_gradient_norm"], sigma=m["sigma"])
    if m["grad_strategy"] == "sgd":
        kw["optimizer"] = "sgd"
    run = HipRun(m["F"], m["hidden"], m["B"], m["L"], algo="prs", **kw)
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        run.set_inputs(d[p + "features"], d[p + "docids"], d[p + "labels"])
        scores = run.forward(d[p + "pre_params"])
        np.testing.assert_allclose(scores, d[p + "scores"], atol=1e-5, rtol=0, err_msg="scores")
        ds, tail = run.loss(ipw_table=d["ipw_list"])
        gs, ref_loss = 1.0 / float(tail[1]), float(d[p + "loss"])
        assert abs(tail[0] * gs - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (tail[0] * gs, ref_loss)
        assert not tail[2:].any()
        g, tail2 = run.backward()
        np.testing.assert_allclose(tail2, tail, rtol=1e-6, atol=1e-6)
        gref = d[p + "grads"]
        np.testing.assert_allclose(g * gs, gref, err_msg="grads", **gtol(gref, name))
        params, state2, _, sc = run.update(d[p + "pre_adagrad"])
        _check_update(d, m, p, name, gs, tail, sc, params, state2)


@pytest.mark.parametrize("name", DNN_CASES)
def test_golden_train_step(name):
    _golden_dnn_step(name)


def test_golden_train_step_under_both_mfma_plans(mfma_mode):
    _golden_dnn_step("prs_tiny")


def test_golden_setrank_step():
    from ultra_pytorch_amd import engine, hip_ops
    d, m = load_golden("prs_setrank_tiny")
    F, dm, H, nl, dff = prs_ref.setrank_cfg(m)
    shape = hip_ops.SetRankShape(F, dm, H, nl, dff)
    assert [n for n, _, _ in shape.layout()] == m["param_keys"]
    B, L = m["B"], m["L"]
    eng = engine.SetRankStepEngine(shape, B, L, torch.device("cuda"), algo="prs", learning_rate=m["lr"],
                                   max_gradient_norm=m["max_gradient_norm"], sigma=m["sigma"])
    ipw = dev(np.asarray(d["ipw_list"], np.float32))
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        prm, st = dev(d[p + "pre_params"].copy()), dev(d[p + "pre_adagrad"].copy())
        f = dev(np.asarray(d[p + "features"], np.float32))
        i, y = dev(d[p + "docids"], torch.int32), dev(d[p + "labels"], torch.float32)
        sc = eng.train_step(prm, st, f, f.shape[0], i, y, ipw_table=ipw)
        torch.cuda.synchronize()
        np.testing.assert_allclose(eng.scores.cpu().numpy(), d[p + "scores"], atol=1e-5, rtol=0, err_msg="scores")
        sc = sc.cpu().numpy()
        g = eng.grads[: shape.n_params].cpu().numpy() / float(sc[3])
        gref = d[p + "grads"]
        np.testing.assert_allclose(g, gref, rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(gref).max())), err_msg="grads")
        tail = eng.grads[shape.n_params:].cpu().numpy()
        _check_update(d, m, p, "prs_setrank_tiny", 1.0 / float(sc[3]), tail, sc, prm.cpu().numpy(), st.cpu().numpy())


# ---- the loss kernel against the restatement ------------------------------------------------------------------------------
PRS_JW, LDS_LIMIT = 16, 160 * 1024  # csrc/ultr_listloss.h: LOSS_JW


def _lds_bytes(L):  # csrc/ultr_listloss.h: PrsLds (one list per workgroup)
    return ((4 + 2 * L) + 8 * L + L + PRS_JW * L * 2) * 4


L_MAX = max(L for L in range(1, 2048) if _lds_bytes(L) <= LDS_LIMIT)


def kernel_loss(scores_BL, labels_LB, ipw, sigma=1.0):
    """(loss, d loss / d scores) of ultr_prs_loss: the x D convention undone with the tail's D."""
    from ultra_pytorch_amd import hip_ops
    B, L = scores_BL.shape
    s = dev(scores_BL.astype(np.float32))
    y = dev(labels_LB.astype(np.float32))
    tab = dev(np.asarray(ipw, np.float32))
    ds = torch.full((B, L), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.full((hip_ops.loss_workspace_bytes(B, L) // 4,), 3.0, dtype=torch.float32, device="cuda")
    hip_ops.prs_loss(s, y, tab, sigma, B, L, ds, ws)
    torch.cuda.synchronize()
    tail = hip_ops.tail_floats(L)
    parts = ws[: hip_ops.loss_part_count(B) * tail].view(-1, tail).double().cpu().numpy()
    assert not parts[:, 2:].any()
    t = parts.sum(0)
    return t[0] / t[1], ds.double().cpu().numpy() / t[1], t[1]


def ref_loss(scores_BL, labels_LB, ipw, sigma=1.0, dtype=torch.float64):
    return prs_ref.prs_score_grad(scores_BL.astype(np.float32), labels_LB.T, ipw, sigma, dtype)


def _batch(rng, B, L, p_click=0.3):
    s = rng.normal(scale=1.5, size=(B, L)).astype(np.float32)
    y = (rng.uniform(size=(L, B)) < p_click).astype(np.float32)
    return s, y


@pytest.mark.parametrize("B,L", [(37, 10), (18, 50), (3, 70), (2, L_MAX)])
def test_loss_kernel_matches_restatement(B, L):
    rng = np.random.RandomState(B * 1000 + L)
    s, y = _batch(rng, B, L)
    s[0, : L // 2] = s[0, L // 2: 2 * (L // 2)]  # exact ties (broken by presentation order)
    s[1 % B, 3:7] = 0.25
    y[:, 2 % B] = 0.0  # a list without a click
    y[:, 0] = np.where(np.arange(L) % 3 == 0, 1.0, 0.0)
    ipw = np.linspace(1.0, 9.0, 40)
    ipw[4] = 0.0  # pw = 0 there (_safe_div), prs = 0 for pairs whose first element sits there
    for sigma, table in ((1.0, ipw), (0.7, ipw[:7])):  # and a table shorter than L: positions past it take the last entry
        loss, ds, D = kernel_loss(s, y, table, sigma)
        rl, rg = ref_loss(s, y, table, sigma)
        assert abs(loss - rl) <= 1e-5 * abs(rl), (loss, rl)
        np.testing.assert_allclose(ds, rg, rtol=1e-4, atol=1e-5 * np.abs(rg).max())


def test_loss_kernel_without_clicks_is_zero_over_zero():
    """No click anywhere in the batch: IDCG = 0, every delta is 0 - as in the reference, the loss is 0 / 0 (NaN) and the kernel's
    own sums are exact zeros."""
    from ultra_pytorch_amd import hip_ops
    B, L = 5, 10
    s, _ = _batch(np.random.RandomState(3), B, L)
    y = np.zeros((L, B), np.float32)
    ds = torch.zeros(B, L, device="cuda")
    ws = torch.zeros(hip_ops.loss_workspace_bytes(B, L) // 4, device="cuda")
    hip_ops.prs_loss(dev(s), dev(y), dev(np.ones(4, np.float32)), 1.0, B, L, ds, ws)
    torch.cuda.synchronize()
    assert not ds.cpu().numpy().any() and not ws.cpu().numpy().any()
    rl, _ = ref_loss(s, y, np.ones(4))
    assert np.isnan(rl)


def _clustered(rng, B, L):
    """Scores in clusters at 0, 21, 42, 63 (+-1.5): every gap is below 3 or between 18 and 66 - beyond the x == 1 cliff
    (~16.6) and away from exp's overflow (~88.7)."""
    c = rng.randint(0, 4, size=(B, L)) * 21.0
    return (c + rng.uniform(-1.5, 1.5, size=(B, L))).astype(np.float32)


def test_loss_kernel_saturated_regime():
    B, L = 12, 20
    rng = np.random.RandomState(21)
    s = _clustered(rng, B, L)
    y = (rng.uniform(size=(L, B)) < 0.4).astype(np.float32)
    ipw = np.linspace(1.0, 6.0, 40)
    loss, ds, D = kernel_loss(s, y, ipw)
    rl, rg = ref_loss(s, y, ipw, dtype=torch.float32)
    assert np.isfinite(ds).all()
    # the exploding gradient (x rounded to 1, the 1e-12 floor) is present: float64 arithmetic would give a 100x smaller one
    assert np.abs(rg).max() > 100.0 * np.abs(ref_loss(s, y, ipw)[1]).max()
    assert abs(loss - rl) <= 1e-3 * abs(rl), (loss, rl)
    np.testing.assert_allclose(ds, rg, rtol=1e-3, atol=1e-6 * np.abs(rg).max())


def test_loss_kernel_nan_where_exp_overflows():
    """A gap above ~88.7: exp overflows in the lower triangle and both scores of that pair get NaN - exactly where torch puts it."""
    B, L = 6, 10
    rng = np.random.RandomState(5)
    s, y = _batch(rng, B, L, p_click=0.4)
    s[2] = [92.0, 8.0, 5.0, 4.5, 7.0, 6.0, 1.0, -2.0, 0.0, 2.5]  # gaps to 92: 84 .. 87.5 (finite) and 89.5 .. 94 (overflow)
    y[:, 2] = [0, 1, 0, 1, 0, 0, 1, 0, 1, 0]
    ipw = np.linspace(1.0, 6.0, 40)
    loss, ds, D = kernel_loss(s, y, ipw)
    rl, rg = ref_loss(s, y, ipw, dtype=torch.float32)
    nan = np.isnan(rg)
    assert nan[2].any() and not nan[2].all() and not np.delete(nan, 2, axis=0).any()
    np.testing.assert_array_equal(np.isnan(ds), nan)
    assert np.isfinite(loss) and abs(loss - rl) <= 1e-3 * abs(rl)
    np.testing.assert_allclose(ds[~nan], rg[~nan], rtol=1e-3, atol=1e-6 * np.abs(rg[~nan]).max())


def test_loss_kernel_refuses_lists_beyond_the_lds_budget():
    from ultra_pytorch_amd import _lib, hip_ops
    L = L_MAX + 1
    s = torch.zeros(1, L, device="cuda")
    ds = torch.zeros(1, L, device="cuda")
    ws = torch.zeros(hip_ops.loss_workspace_bytes(1, L) // 4, device="cuda")
    tab = torch.ones(4, device="cuda")
    rc = _lib.load().ultr_prs_loss(s.data_ptr(), s.data_ptr(), tab.data_ptr(), 4, 1.0, 1, L, ds.data_ptr(), ws.data_ptr(),
                                   hip_ops.raw_stream())
    assert rc == -2  # ULTR_E_UNSUPPORTED
    rc = _lib.load().ultr_prs_loss(s.data_ptr(), s.data_ptr(), None, 0, 1.0, 1, 8, ds.data_ptr(), ws.data_ptr(), hip_ops.raw_stream())
    assert rc == -1  # ULTR_E_BADARG: PRS needs its table


# ---- full size ------------------------------------------------------------------------------------------------------------
def test_full_size_step_matches_oracle_and_restatement():
    """Config 4's shape (700-d, DNN[512,256,128], B 256, L 50) through ONE ultr_train_step, against the oracle's forward + the
    restatement; gradients at test_gpu_full_size's per-entry bar (1e-5 of |g_ref| + the entry's float64 sum of |terms|)."""
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    F, hidden, B, L = 700, [512, 256, 128], 256, 50
    rng = np.random.RandomState(7)
    feats, ids, y = synthetic.make_batch(rng, B, L, F)
    ipw = synthetic.load_ipw()
    params = O.init_params(F, hidden, seed=2)
    state = np.zeros_like(params)
    fwd = prs_ref.dnn_forward(F, hidden, feats, ids.astype(np.int64))
    ref = prs_ref.prs_step(params, state, fwd, y, ipw)
    shape = hip_ops.DnnShape(F, hidden, "elu")
    eng = engine.StepEngine(shape, B, L, torch.device("cuda"), algo="prs")
    p, st = dev(params.copy()), dev(state.copy())
    sc = eng.train_step(p, st, dev(feats), feats.shape[0], dev(ids, torch.int32), dev(y), ipw_table=dev(ipw.astype(np.float32)))
    torch.cuda.synchronize()
    sc = sc.cpu().numpy()
    np.testing.assert_allclose(eng.scores.cpu().numpy(), ref["scores"], atol=1e-5)
    assert abs(sc[0] - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"]))
    assert abs(sc[1] - ref["norm"]) <= 1e-5 * ref["norm"]
    gs = 1.0 / float(sc[3])
    g = eng.grads[: shape.n_params].cpu().numpy() * gs
    ds = eng.dscores.cpu().numpy() * gs
    terms = O.dnn_backward_manual(params, F, hidden, O.gather_rows(feats, ids).numpy(), ds.T.reshape(-1), abs_terms=True)
    assert (np.abs(g - ref["grads"]) <= 1e-5 * (np.abs(ref["grads"]) + terms)).all()
    sel = np.abs(ref["grads"]) > 1e-6 * np.abs(ref["grads"]).max()
    np.testing.assert_allclose(p.cpu().numpy()[sel], ref["params"][sel], atol=5e-6, rtol=1e-5)


# ---- the plugin -----------------------------------------------------------------------------------------------------------
class DS:
    def __init__(self, n_queries, L, F, seed):
        rng = np.random.RandomState(seed)
        self.feature_size, self.features, self.initial_list, self.labels, self.dids, self.qids = F, [], [], [], [], []
        for q in range(n_queries):
            self.features += rng.uniform(-1, 1, size=(L, F)).astype(np.float32).tolist()
            self.initial_list.append(list(range(q * L, (q + 1) * L)))
            lab = rng.randint(0, 5, size=L)
            lab[0] = max(lab[0], 1)
            self.labels.append([int(v) for v in lab])
            self.dids += ["d%d" % i for i in range(q * L, (q + 1) * L)]
            self.qids.append("q%d" % q)
        self.rank_list_size = L
        self.features.append([0.0] * F)  # pad row


def make_algo(F, L, hidden, hp=""):
    from ultra_pytorch_amd.utils import find_class
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.PRSrank", "learning_algorithm_hparams": hp,
           "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=%s" % json.dumps(hidden),
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3]}
    return find_class(exp["learning_algorithm"])(DS(1, L, F, 0), exp)


def _feed_arrays(algo, feed, L):
    if feed.get("device_feed", False):
        return (feed["features"].cpu().numpy().copy(), feed["docids"][:L].cpu().numpy().astype(np.int64),
                feed["labels"][:L].cpu().numpy().copy())
    feats = np.asarray(feed["letor_features"], np.float32)
    ids = np.stack([np.asarray(feed[algo.docid_inputs_name[l]]) for l in range(L)]).astype(np.int64)
    y = np.stack([np.asarray(feed[algo.labels_name[l]]) for l in range(L)]).astype(np.float32)
    return feats, ids, y


@pytest.mark.parametrize("device_feed", [False, True])
def test_plugin_train_on_a_feed_batch(device_feed, capsys):
    from ultra_pytorch_amd.input_layer import ClickSimulationFeed, DeviceClickFeed
    F, L, B, hidden = 24, 10, 16, [16, 8]
    ds = DS(64, L, F, seed=4)
    algo = make_algo(F, L, hidden)
    feed = DeviceClickFeed(algo, B, "", seed=3) if device_feed else ClickSimulationFeed(algo, B, "")
    for step in range(2):
        input_feed, _ = feed.get_batch(ds, check_validation=True)
        feats, ids, y = _feed_arrays(algo, input_feed, L)
        p0, s0 = algo.model.flat_params.cpu().numpy().copy(), algo.state_sum.cpu().numpy().copy()
        capsys.readouterr()
        loss, out, summary = algo.train(input_feed)
        assert out is None and isinstance(summary, dict)
        assert " Loss %f at Global Step %d: " % (loss, step) in capsys.readouterr().out  # 0-based, as the reference prints it
        ref = prs_ref.prs_step(p0, s0, prs_ref.dnn_forward(F, hidden, feats, ids), y, algo.IPW_list)
        assert abs(loss - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"]))
        g = ref["grads"]
        sel = np.abs(g) > 1e-6 * np.abs(g).max()
        np.testing.assert_allclose(algo.model.flat_params.cpu().numpy()[sel], ref["params"][sel], atol=5e-6, rtol=1e-5)
        if not device_feed:
            n = len(algo.IPW_list)
            assert input_feed["propensity_weights%d" % (L - 1)] == [algo.IPW_list[min(L - 1, n - 1)]] * B
    assert algo.global_step == 2


def test_plugin_trajectory_and_determinism():
    """20 steps at prs_tiny's shape against the CPU restatement (params within 1e-4), then one step run twice is bitwise equal."""
    d, m = load_golden("prs_tiny")
    F, L, B, hidden = m["F"], m["L"], m["B"], m["hidden"]
    from tests.test_gpu_plugins import load_flat, make_feed
    rng = np.random.RandomState(13)
    algo = make_algo(F, L, hidden)
    load_flat(algo.model, d["s0_pre_params"])
    # a warm Adagrad accumulator: from zero the first update is lr * sign(g), which flips on rounding noise where g ~ 0
    params, state = d["s0_pre_params"].copy(), np.full_like(d["s0_pre_params"], 0.1)
    algo.state_sum.fill_(0.1)
    for _ in range(20):
        feats, ids, y = _rand_batch(rng, B, L, F)
        algo.train(make_feed(algo, feats, ids, y))
        r = prs_ref.prs_step(params, state, prs_ref.dnn_forward(F, hidden, feats, ids.astype(np.int64)), y, algo.IPW_list)
        params, state = r["params"], r["state"]
    np.testing.assert_allclose(algo.model.flat_params.cpu().numpy(), params, atol=1e-4)
    feats, ids, y = _rand_batch(rng, B, L, F)
    p0, s0 = algo.model.flat_params.clone(), algo.state_sum.clone()
    outs = []
    for _ in range(2):
        algo.model.flat_params.copy_(p0)
        algo.state_sum.copy_(s0)
        loss, _, _ = algo.train(make_feed(algo, feats, ids, y))
        outs.append((loss, algo.model.flat_params.cpu().numpy().copy(), algo.state_sum.cpu().numpy().copy()))
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


def _rand_batch(rng, B, L, F):
    feats = rng.uniform(-1, 1, size=(B * L, F)).astype(np.float32)
    ids = rng.permutation(B * L).reshape(L, B).astype(np.int32)
    y = (rng.uniform(size=(L, B)) < 0.3).astype(np.float32)
    y[0] = 1.0
    return feats, ids, y


# ---- data parallel --------------------------------------------------------------------------------------------------------
DP_F, DP_HIDDEN, DP_B, DP_L = 24, [32, 16], 7, 6  # 7 lists -> shards of 4 and 3


def _dp_global():
    rng = np.random.RandomState(3)
    feats = rng.uniform(-1, 1, size=(DP_B * DP_L, DP_F)).astype(np.float32)
    ids = rng.permutation(DP_B * DP_L).reshape(DP_L, DP_B).astype(np.int32)
    y = (rng.uniform(size=(DP_L, DP_B)) < 0.4).astype(np.float32)
    y[0, :] = np.arange(DP_B) % 2
    return feats, ids, y


def _dp_run(feats, ids, y, pg):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine, hip_ops
    d = torch.device("cuda", torch.cuda.current_device())
    params = O.init_params(DP_F, DP_HIDDEN, seed=5)
    shape = hip_ops.DnnShape(DP_F, DP_HIDDEN, "elu")
    eng = engine.StepEngine(shape, ids.shape[1], DP_L, d, algo="prs", process_group=pg)
    p, st = torch.tensor(params, device=d), torch.full((params.shape[0],), 0.01, device=d)  # warm Adagrad state
    ipw = torch.linspace(1.0, 3.0, 4, device=d)  # shorter than L: clamps
    f, i, yy = torch.tensor(feats, device=d), torch.tensor(ids, device=d), torch.tensor(y, device=d)
    losses = []
    for _ in range(2):
        sc = eng.train_step(p, st, f, feats.shape[0], i, yy, ipw_table=ipw)
        torch.cuda.synchronize()
        losses.append(float(sc[0]))
    out = dict(params=p.cpu().numpy(), state=st.cpu().numpy(), losses=losses, peer=eng.comm is not None,
               status=0 if eng.comm is None else eng.comm.status())
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
    # every rank keeps the whole feature matrix: the shard is a slice of the lists
    q.put((rank, _dp_run(feats, ids[:, lo:hi].copy(), y[:, lo:hi].copy(), pg)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["peer", "pg"])
def test_two_rank_step_equals_single_process(mode):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29880 + (0 if mode == "peer" else 1)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, mode, q)) for r in range(2)]  # 2 rank processes (<= 5)
    [p.start() for p in procs]
    got = dict(q.get(timeout=300) for _ in range(2))
    [p.join(120) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    one = _dp_run(*_dp_global(), None)
    for rank in (0, 1):
        res = got[rank]
        assert res["status"] == 0 and res["peer"] == (mode == "peer")
        assert np.array_equal(res["params"], got[0]["params"])
        np.testing.assert_allclose(res["losses"], one["losses"], rtol=1e-6)
        np.testing.assert_allclose(res["params"], one["params"], rtol=1e-6, atol=1e-6 * np.abs(one["params"]).max())
        np.testing.assert_allclose(res["state"], one["state"], rtol=2e-5, atol=1e-12)
