"""PLRank behind the plugin seams, driven the way main.py drives a learning algorithm: the class from find_class and a settings dict,
numpy feed dicts, train() / validation() triples - on the DNN (F = 24, [32, 16], B = 7, L = 10), Linear and the small SetRank, DLCM and
GSF shapes of tests/test_gpu_twotower_plugins.py, with Adagrad, SGD and Adam, l2_loss 0 and > 0, the Oracle estimator on a
user-browsing model (the pw path) and DeviceClickFeed batches.

Every train() is held to the float64 law (tests/plrank_ref.py) fed what the GPU itself used: the engine's scores; the ORDERS the step
drew - the loss launch is repeated on those scores under the step's (seed, step) with perm_out, and must give the step's dscores bit
for bit; its `grads` buffer (raw gradient and folded step tail); the parameters and optimizer state before the step.  Bars: those of
tests/test_gpu_plrank.py for the loss stage, SCALAR_RTOL for the step scalars, PARAM_ATOL / STATE_RTOL after the update,
tests/adam_ref.py's for Adam."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import adam_ref as A  # noqa: E402
from tests import loss_ref as R  # noqa: E402
from tests import plrank_ref as T  # noqa: E402
from tests.test_gpu_plugins import DataSet, make_feed  # noqa: E402
from tests.test_gpu_twotower_plugins import MODELS, make_batch  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = os.path.join(GOLDEN, "ultra_toy_data") + "/"
DATA = os.path.join(os.path.dirname(GOLDEN), os.pardir, "ultra_pytorch_amd", "data")
CLS = "ultra_pytorch_amd.learning_algorithm.PLRank"


def settings(model, hp, L):
    cls, model_hp = MODELS[model][:2]
    return {"learning_algorithm": CLS, "learning_algorithm_hparams": hp, "ranking_model": "ultra_pytorch_amd.ranking_model." + cls,
            "ranking_model_hparams": model_hp, "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"],
            "metrics_topn": [1, 3]}


def build(model, hp=""):
    from ultra_pytorch_amd.utils import find_class
    F, L = MODELS[model][2], MODELS[model][4]
    torch.manual_seed(3)
    return find_class(CLS)(DataSet(F), settings(model, hp, L))


def host_state(algo):
    return algo.model.flat_params.detach().cpu().numpy().copy(), algo.state_sum.cpu().numpy().copy()


def hold_train(tag, algo, eng, before, after, loss, ids, y, n_docs, t, dnn=None):
    """One train() against the law put at `before`: the loss stage on the engine's scores and the orders it drew, then the update on
    the engine's gradients."""
    from ultra_pytorch_amd import hip_ops
    hp = algo.hparams
    opt = hp.grad_strategy if hp.grad_strategy in ("sgd", "adam") else "ada"
    L, B = ids.shape
    P = algo.model.shape.n_params
    (p0, st0), (p1, st1) = before, after
    g = eng.grads.cpu().numpy()
    g_raw, tail, sc = g[:P], g[P:].astype(np.float64), eng.scalars.cpu().numpy()
    scores, ds = eng.scores.cpu().numpy(), eng.dscores.cpu().numpy()
    assert eng.rng_seed == algo.rng_seed and eng.rng_step == t - 1 == algo.draw_steps - 1
    # the orders of the step: the same launch on the same scores under the same key, with perm_out
    N = int(hp.num_samples)
    pw = eng.oracle_pw if algo.propensity.oracle and getattr(eng, "oracle_pw", None) is not None else None
    ipw = None if pw is not None else (algo.ipw_table if algo.ipw_table is not None else algo.propensity.step_weights(eng, None, L)[0])
    ds2 = torch.empty_like(eng.dscores)
    ws2 = torch.empty_like(eng.loss_ws)
    perm = torch.empty(B, N, L, dtype=torch.int32, device=ds2.device)
    hip_ops.plrank_loss(eng.scores, algo.labels_LB, algo.docid_inputs, n_docs, B, L, ds2, ws2, n_samples=N, cutoff=int(hp.cutoff),
                        gain=hp.gain, seed=eng.rng_seed, step=eng.rng_step, pw=pw, ipw_table=ipw, perm_out=perm)
    torch.cuda.synchronize()
    assert np.array_equal(ds2.cpu().numpy().view(np.uint32), ds.view(np.uint32)), (tag, "the repeated launch gives other bits")
    perm = perm.cpu().numpy().astype(np.int64)
    valid = T.valid_of(ids, n_docs)
    n_pos, margin = T.n_pos_of(scores, valid)
    assert (margin > 1e-4).all()
    rho = T.rho_of(y, valid, hp.gain, pw=None if pw is None else pw.cpu().numpy(), ipw=None if ipw is None else ipw.cpu().numpy())
    ref = T.reference(scores, rho, valid, perm, int(hp.cutoff), n_pos)
    err = np.abs(ds.astype(np.float64) - ref["dscores"])
    bar = T.dscores_bar(ref["dscores"], ref["terms"], R.TERMS_RTOL)
    e_tail = abs(tail[0] - ref["tail"][0]) / max(1.0, abs(ref["tail"][0]))
    print("%s t=%d: dscores %.3g of the bar, tail %.3e (bar %.0e)" % (tag, t, float((err / bar).max()), e_tail, R.SCALAR_RTOL))
    assert (err <= bar).all() and e_tail <= R.SCALAR_RTOL and tail[1] == B and (tail[2:] == 0.0).all()
    assert (ds[~valid] == 0.0).all()
    if dnn is not None:  # the ranker against autograd through the oracle's DNN, at smoke()'s bar (rtol 1e-4, atol 1e-6)
        from oracle import ultr_oracle as O
        feats, F, hidden = dnn
        x = O.gather_rows(np.asarray(feats, np.float32), ids).double()
        p = torch.tensor(p0.astype(np.float64), requires_grad=True)
        s = O.dnn_forward(p, F, hidden, x, "elu").view(L, B).t()
        np.testing.assert_allclose(scores, s.detach().numpy(), atol=1e-5)
        (s * torch.tensor(ref["dscores"] / B)).sum().backward()
        np.testing.assert_allclose(g_raw.astype(np.float64) / B, p.grad.numpy(), rtol=1e-4, atol=1e-6)
    # the update launch
    n_state = {"sgd": 0, "ada": P, "adam": 2 * P}[opt]
    assert algo.state_sum.numel() == (n_state or P)
    u = T.update_ref(p0, g_raw, st0[:n_state], tail, opt, float(hp.learning_rate), float(hp.max_gradient_norm), float(hp.l2_loss), adam_t=t)
    ss = float((g_raw.astype(np.float64) ** 2).sum())
    want = (u["loss"], u["norm"], u["coef"], float(B), 0.0, 0.0, 0.0, ss)
    for k, w in enumerate(want):
        assert abs(float(sc[k]) - w) <= R.SCALAR_RTOL * max(1.0, abs(w)), (tag, k, float(sc[k]), w)
    assert loss == float(sc[0])  # train() returns scalars[0]
    if opt == "adam":
        terms = np.concatenate([(1 - A.B1) * u["g_terms"], (1 - A.B2) * u["g_terms"] ** 2])
        e_p, e_s = A.excess(p1, u["p"], float(hp.learning_rate)), A.moment_excess(st1, u["state"], st0, terms)
        print("%s t=%d: parameters %.3e (bar %.3e), moments %.3e (bar %.3e)" % (tag, t, e_p, A.BAR, e_s, A.MOMENT_RTOL))
        assert e_p <= A.BAR and e_s <= A.MOMENT_RTOL
    else:
        e_p = float(np.abs(p1 - u["p"]).max())
        print("%s t=%d: parameters %.3e (bar %.3e)" % (tag, t, e_p, R.PARAM_ATOL))
        assert np.isfinite(p1).all() and e_p <= R.PARAM_ATOL, (tag, "params", e_p)
        if opt == "ada":
            rel = np.abs(st1 - u["state"]) / np.maximum(u["state"], 1e-30)
            print("%s t=%d: accumulators %.3e (bar %.3e)" % (tag, t, float(rel.max()), R.STATE_RTOL))
            assert (rel <= R.STATE_RTOL).all(), (tag, "state", float(rel.max()))
        else:
            assert np.array_equal(st1, st0)
    assert not np.array_equal(p1, p0)


def run_three_steps(model, hp):
    cls, model_hp, F, B, L = MODELS[model]
    algo = build(model, hp)
    assert type(algo).__name__ == "PLRank" and algo.opt_steps == 0 and algo.draw_steps == 0 and not algo.state_sum.any()
    assert algo.rng_seed == 3
    dnn_hidden = {"DNN": [32, 16], "Linear": []}.get(model)
    for t in (1, 2, 3):
        feats, ids, y = make_batch(10 * t, F, B, L)
        before = host_state(algo)
        loss, out, summary = algo.train(make_feed(algo, feats, ids, y))
        torch.cuda.synchronize()
        assert out is None and isinstance(summary, dict) and np.isfinite(loss) and algo.global_step == t and algo.opt_steps == t
        eng = algo._train_engines[(B, L)]
        hold_train("%s [%s]" % (model, hp), algo, eng, before, host_state(algo), loss, ids, y, feats.shape[0], t,
                   dnn=None if dnn_hidden is None else (feats, F, dnn_hidden))
    feats, ids, y = make_batch(99, F, B, L)
    _, scores, summary = algo.validation(make_feed(algo, feats, ids, y))
    assert tuple(scores.shape) == (B, L) and torch.isfinite(scores).all() and 0.0 <= summary["ndcg_3"] <= 1.0
    return algo


@pytest.mark.parametrize("model", list(MODELS))
def test_three_train_steps_per_ranking_model(model):
    run_three_steps(model, "num_samples=32")


@pytest.mark.parametrize("hp", ["grad_strategy=sgd,learning_rate=0.1,num_samples=17,cutoff=3",
                                "grad_strategy=adam,gain=exp2,num_samples=16",
                                "grad_strategy=ada,l2_loss=0.01,max_gradient_norm=0.01,num_samples=100,cutoff=5"])
def test_each_grad_strategy_on_the_dnn(hp):
    algo = run_three_steps("DNN", hp)
    if "max_gradient_norm=0.01" in hp:
        assert float(algo._train_engines[(7, 10)].scalars[2]) < 1.0  # l2_loss > 0 and the clip still applies


def test_the_draw_counter_survives_an_evicted_engine():
    """The step of the draw's key is the algorithm object's: a new engine (another batch size) goes on where the last one stopped."""
    algo = build("DNN", "num_samples=8")
    F, L = 24, 10
    for t, B in enumerate((7, 5, 7), start=1):
        feats, ids, y = make_batch(t, F, B, L)
        algo.train(make_feed(algo, feats, ids, y))
        assert algo._train_engines[(B, L)].rng_step == t - 1
    assert algo.draw_steps == 3 and len(algo._train_engines) == 2


def test_refusals():
    with pytest.raises(ValueError, match="gain"):
        build("DNN", "gain=log")
    with pytest.raises(ValueError, match="num_samples"):
        build("DNN", "num_samples=0")
    from ultra_pytorch_amd.utils import find_class
    exp = dict(settings("DNN", "", 10), process_group=object())
    with pytest.raises(NotImplementedError):
        find_class(CLS)(DataSet(24), exp)


def test_oracle_estimator_on_a_user_browsing_model(tmp_path):
    """The pw path: hip_ops.history_pw fills the step's per-click weights [B, L] from the Oracle estimator's table."""
    from ultra_pytorch_amd.utils import find_class
    path = tmp_path / "oracle_ubm.json"
    path.write_text(json.dumps({"click_model": json.load(open(os.path.join(DATA, "ubm_0.1_1_4_1.0.json")))}))
    F, B, L = 24, 7, 10
    hp = ("propensity_estimator_type=ultra.utils.propensity_estimator.OraclePropensityEstimator,propensity_estimator_json=%s,"
          "num_samples=32" % path)
    torch.manual_seed(3)
    algo = find_class(CLS)(DataSet(F), settings("DNN", hp, L))
    assert algo.propensity.oracle and algo.ipw_table is None
    for t in (1, 2, 3):
        feats, ids, y = make_batch(20 * t, F, B, L)
        y = (y > 0).astype(np.float32)  # clicks
        before = host_state(algo)
        loss, _, _ = algo.train(make_feed(algo, feats, ids, y))
        torch.cuda.synchronize()
        eng = algo._train_engines[(B, L)]
        assert eng.oracle_pw is not None and float(eng.oracle_pw.max()) > 1.0
        hold_train("oracle ubm", algo, eng, before, host_state(algo), loss, ids, y, feats.shape[0], t, dnn=(feats, F, [32, 16]))


def test_three_steps_from_device_click_feed_batches():
    from tests.test_gpu_feed import DS
    from ultra_pytorch_amd.input_layer import DeviceClickFeed
    from ultra_pytorch_amd.utils import find_class
    F, L, B = 16, 10, 64
    ds = DS(200, (6, 10), F, seed=2)
    ds.pad(L)
    torch.manual_seed(5)
    algo = find_class(CLS)(ds, settings("DNN", "num_samples=16", L))
    feed = DeviceClickFeed(algo, B, "", seed=1)
    for t in (1, 2, 3):
        input_feed, _ = feed.get_batch(ds, check_validation=True)
        ids, y = input_feed["docids"].cpu().numpy().copy(), input_feed["labels"].cpu().numpy().copy()
        feats, n_docs = input_feed["features"].cpu().numpy().copy(), int(input_feed["n_docs"])
        assert (ids == n_docs).any()  # the batch has PADs
        before = host_state(algo)
        loss, _, _ = algo.train(input_feed)
        torch.cuda.synchronize()
        assert np.isfinite(loss) and algo.global_step == t
        eng = algo._train_engines[(B, L)]
        if t > 1:
            assert eng.next_click_source is feed  # the engine drew this batch behind the step before
        hold_train("device feed", algo, eng, before, host_state(algo), loss, ids, y, n_docs, t, dnn=(feats[:n_docs], F, [32, 16]))


def test_training_on_true_labels_lowers_the_loss(tmp_path):
    """DirectLabelFeed labels, gain=exp2, a table of ones: over 200 steps on the toy training set the mean reported loss (minus the
    sampled DCG) of the last 20 steps lies below that of the first 20."""
    from ultra_pytorch_amd import utils
    from ultra_pytorch_amd.input_layer import DirectLabelFeed
    table = tmp_path / "ones.json"
    table.write_text(json.dumps({"IPW_list": [1.0] * 10}))
    train_set = utils.read_data(TOY, "train", None, None)
    L = int(train_set.rank_list_size)
    exp = {"learning_algorithm": CLS,
           "learning_algorithm_hparams": "gain=exp2,num_samples=32,propensity_estimator_json=%s" % table,
           "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=[32,16]",
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3]}
    DirectLabelFeed.preprocess_data(train_set, "", exp)
    train_set.pad(L)
    torch.manual_seed(1)
    algo = utils.find_class(CLS)(train_set, exp)
    feed = DirectLabelFeed(algo, 16, "")
    import random
    random.seed(1)
    losses = []
    for _ in range(200):
        input_feed, _ = feed.get_batch(train_set, check_validation=True)
        losses.append(algo.train(input_feed)[0])
    first, last = float(np.mean(losses[:20])), float(np.mean(losses[-20:]))
    print("mean loss of the first 20 steps %.4f, of the last 20 %.4f" % (first, last))
    assert np.isfinite(losses).all() and last < first
