"""AffineRank behind the plugin seams, driven the way main.py drives a learning algorithm: the class from find_class and a settings
dict, numpy feed dicts and DeviceClickFeed batches, train() / validation() triples - on the DNN (F = 24, [32, 16], B = 7, L = 10),
Linear and the small SetRank, DLCM and GSF shapes of tests/test_gpu_twotower_plugins.py, with Adagrad, SGD and Adam, l2_loss 0 and > 0,
mask_padding on and off.

Every train() is held to the float64 step twin (tests/trust_ref.step_ref) fed what the GPU itself used: the engine's scores, its
`grads` buffer (raw gradient and folded step tail), the parameters and optimizer state before the step.  Checked: the scores and the
gradient of the DNN (against autograd through the oracle's DNN, at smoke()'s bar, its absolute part scaled by the largest
|dscores|), dscores and the loss sum (TERMS_RTOL), the loss, the
gradient norm, the clip coefficient and D (SCALAR_RTOL), the parameters and the optimizer state after the update (PARAM_ATOL /
STATE_RTOL; tests/adam_ref.py's for Adam) - in the manner of tests/test_gpu_plrank_plugins.py's hold_train."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import adam_ref as A  # noqa: E402
from tests import loss_ref as R  # noqa: E402
from tests import trust_ref as T  # noqa: E402
from tests.test_gpu_plugins import DataSet, make_feed  # noqa: E402
from tests.test_gpu_twotower_plugins import MODELS, make_batch  # noqa: E402

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ultra_pytorch_amd", "data")
SHIPPED = os.path.join(DATA, "trust_0.1_1.0_4_1.0.json")
CLS = "ultra_pytorch_amd.learning_algorithm.AffineRank"


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
    """One train() against the step twin put at `before`."""
    hp = algo.hparams
    opt = hp.grad_strategy if hp.grad_strategy in ("sgd", "adam") else "ada"
    L, B = ids.shape
    P = algo.model.shape.n_params
    (p0, st0), (p1, st1) = before, after
    g = eng.grads.cpu().numpy()
    g_raw, tail, sc = g[:P], g[P:].astype(np.float64), eng.scalars.cpu().numpy()
    scores, ds = eng.scores.cpu().numpy(), eng.dscores.cpu().numpy()
    n_state = {"sgd": 0, "ada": P, "adam": 2 * P}[opt]
    assert algo.state_sum.numel() == (n_state or P)
    masked = bool(hp.mask_padding)
    ref = T.step_ref(p0, st0[:n_state], scores, y, algo.alpha, algo.beta, ids, n_docs, masked, g_raw, opt, float(hp.learning_rate),
                     float(hp.max_gradient_norm), float(hp.l2_loss), t, dnn=dnn, tail=tail)
    # the loss stage, on the engine's own scores
    lp = ref["loss"]
    e_ds = T.excess(ds, lp["ds"], lp["ds_abs"])
    e_tail = T.excess(tail[:1], lp["tail"][:1], lp["tail_abs"][:1])
    print("%s t=%d: dscores %.3e, loss sum %.3e of (|ref| + terms) (bar %.0e)" % (tag, t, e_ds, e_tail, R.TERMS_RTOL))
    assert e_ds <= R.TERMS_RTOL and e_tail <= R.TERMS_RTOL and tail[1] == B and not tail[2:].any()
    assert (lp["W"] != 0).any() and (lp["w"] < 0).any()  # negative weights are the rule
    if masked:
        assert (lp["w"][~lp["live"]] == 0.0).all() and not lp["live"].all()
    if dnn is not None:
        # the ranker against autograd through the oracle's DNN, at smoke()'s bar (rtol 1e-4, atol 1e-6).  That bar is stated for
        # dscores of order 1 and the backward is linear in dscores: here the weights reach 1 / alpha ~ 20, so the absolute part scales
        # with the largest |dscores| of the twin (the output bias gradient is the sum of all dscores, exactly 0 list by list)
        scale = max(1.0, float(np.abs(lp["ds"]).max()))
        np.testing.assert_allclose(scores, ref["dnn_scores"], atol=1e-5)
        np.testing.assert_allclose(g_raw.astype(np.float64) / B, ref["dnn_grad"], rtol=1e-4, atol=1e-6 * scale)
    # the update launch
    u = ref["update"]
    ss = float((g_raw.astype(np.float64) ** 2).sum())
    want = (u["loss"], u["norm"], u["coef"], float(B), 0.0, 0.0, 0.0, ss)
    for k, w in enumerate(want):
        assert abs(float(sc[k]) - w) <= R.SCALAR_RTOL * max(1.0, abs(w)), (tag, k, float(sc[k]), w)
    assert loss == float(sc[0])  # train() returns scalars[0]
    assert abs(u["loss"] - float(hp.l2_loss) * 0.5 * float((p0.astype(np.float64) ** 2).sum()) - lp["loss"]) <= R.SCALAR_RTOL * max(1.0, abs(lp["loss"]))
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
    return u


def run_two_steps(model, hp):
    cls, model_hp, F, B, L = MODELS[model]
    algo = build(model, hp)
    assert type(algo).__name__ == "AffineRank" and algo.opt_steps == 0 and not algo.state_sum.any()
    assert algo.alpha.shape == algo.beta.shape == (L,) and tuple(algo.affine_table.shape) == (2 * L,)
    dnn_hidden = {"DNN": [32, 16], "Linear": []}.get(model)
    last = None
    for t in (1, 2):
        feats, ids, y = make_batch(10 * t, F, B, L)
        before = host_state(algo)
        loss, out, summary = algo.train(make_feed(algo, feats, ids, y))
        torch.cuda.synchronize()
        assert out is None and isinstance(summary, dict) and np.isfinite(loss) and algo.global_step == t and algo.opt_steps == t
        eng = algo._train_engines[(B, L)]
        last = hold_train("%s [%s]" % (model, hp), algo, eng, before, host_state(algo), loss, ids, y, feats.shape[0], t,
                          dnn=None if dnn_hidden is None else (feats, F, dnn_hidden))
    feats, ids, y = make_batch(99, F, B, L)
    _, scores, summary = algo.validation(make_feed(algo, feats, ids, y))
    assert tuple(scores.shape) == (B, L) and torch.isfinite(scores).all() and 0.0 <= summary["ndcg_3"] <= 1.0
    return algo, last


@pytest.mark.parametrize("model", list(MODELS))
def test_two_train_steps_per_ranking_model(model):
    run_two_steps(model, "")


@pytest.mark.parametrize("hp", ["grad_strategy=sgd,learning_rate=0.1,l2_loss=0.01,max_gradient_norm=0.01",
                                "grad_strategy=adam",
                                "mask_padding=false",
                                "affine_clip=0.2,grad_strategy=ada,l2_loss=0.001"])
def test_each_grad_strategy_and_setting_on_the_dnn(hp):
    algo, last = run_two_steps("DNN", hp)
    if "max_gradient_norm=0.01" in hp:
        assert last["coef"] < 1.0 and float(algo._train_engines[(7, 10)].scalars[2]) < 1.0  # l2_loss > 0 and the clip still applies
    if "affine_clip" in hp:
        assert algo.alpha.min() == np.float32(0.2) and (algo.alpha > np.float32(0.2)).any()


def test_two_steps_from_device_click_feed_batches_with_the_trust_model():
    from tests.test_gpu_feed import DS
    from ultra_pytorch_amd.input_layer import DeviceClickFeed
    from ultra_pytorch_amd.utils import find_class
    F, L, B = 16, 10, 64
    ds = DS(200, (6, 10), F, seed=2)
    ds.pad(L)
    torch.manual_seed(5)
    algo = find_class(CLS)(ds, settings("DNN", "affine_estimator_json=%s" % SHIPPED, L))
    feed = DeviceClickFeed(algo, B, "click_model_json=%s" % SHIPPED, seed=1)
    assert feed.model_id == 3
    # the learner's table is the image the feed simulates with
    assert np.array_equal(np.concatenate([algo.alpha, algo.beta]), feed.exam.cpu().numpy().reshape(-1))
    for t in (1, 2):
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


def test_refusals(tmp_path):
    from ultra_pytorch_amd.utils import find_class
    exp = dict(settings("DNN", "", 10), process_group=object())
    with pytest.raises(NotImplementedError):
        find_class(CLS)(DataSet(24), exp)
    table = tmp_path / "bad.json"
    table.write_text(json.dumps({"alpha": [0.5, 0.0, 0.2], "beta": [0.1, 0.1, 0.1]}))
    with pytest.raises(ValueError, match="alpha"):
        build("DNN", "affine_estimator_json=%s" % table)
    with pytest.raises(ValueError, match="affine_clip"):
        build("DNN", "affine_clip=-0.5")
    # a written table loads into the same learner
    algo = build("DNN", "affine_clip=0.1")
    out = tmp_path / "table.json"
    algo.write_affine_table(str(out))
    again = build("DNN", "affine_estimator_json=%s" % out)
    assert np.array_equal(again.alpha, algo.alpha) and np.array_equal(again.beta, algo.beta)


def test_a_step_without_its_table_is_refused_with_nothing_launched():
    """ultr_train_step checks AffineRank's table beside the loss route: ULTR_E_BADARG before the forward is queued."""
    from ultra_pytorch_amd import _lib
    cls, model_hp, F, B, L = MODELS["DNN"]
    algo = build("DNN")
    feats, ids, y = make_batch(10, F, B, L)
    algo.train(make_feed(algo, feats, ids, y))
    torch.cuda.synchronize()
    eng = algo._train_engines[(B, L)]
    before = host_state(algo)
    eng.scores.fill_(7.0)
    eng.dscores.fill_(7.0)
    eng.set_opt_step(2)
    with pytest.raises(_lib.UltrHipError):
        eng.train_step(algo.model.flat_params, algo.state_sum, algo.letor_features, algo.n_docs, algo.docid_inputs, algo.labels_LB,
                       ipw_table=None)
    torch.cuda.synchronize()
    assert (eng.scores == 7.0).all() and (eng.dscores == 7.0).all()
    after = host_state(algo)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
