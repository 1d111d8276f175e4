"""IPWrank / PRSrank trained with the Oracle propensity estimator on the GPU, against the reference's own steps
(tests/golden/oracle_pw/*.npz, recorded by make_golden_oracle_pw.py): through the step engines stage by stage and through the plugin
classes, the weight buffer bitwise; the settings-file route that used to die with KeyError; the device click feed; one full-size step.
Tolerances are the ones of the table-path golden tests (test_gpu_parity.py, test_gpu_plugins.py, test_gpu_prs.py,
test_gpu_setrank.py), restated."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import history_pw_ref as R  # noqa: E402
from tests.hipref import HipRun, dev, load_golden  # noqa: E402
from tests.test_gpu_parity import gtol  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "ultra_pytorch_amd", "data")
DNN_FIXTURES = ["ipw_oracle_ubm_tiny", "ipw_oracle_ubm_odd", "ipw_oracle_pbm_tiny", "prs_oracle_ubm_tiny", "prs_oracle_ubm_l50"]
SETRANK_FIXTURE = "ipw_oracle_ubm_setrank_tiny"
SETRANK_HPARAMS = "d_model=32,num_heads=4,num_layers=2,diff=16"
CLS = {"ipw": "IPWrank", "prs": "PRSrank"}
ORACLE = "ultra.utils.propensity_estimator.OraclePropensityEstimator"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_of(model_file):
    from ultra_pytorch_amd.utils import click_models as CM
    from ultra_pytorch_amd.utils.propensity_estimator import OraclePropensityEstimator
    return OraclePropensityEstimator(CM.loadModelFromJson(json.load(open(os.path.join(DATA, model_file)))))


def device_weights(m, labels_dev, want):
    """(ipw_table numpy or None, pw numpy [B, L] or None) the way the learners form them; the history buffer is bitwise `want`."""
    from ultra_pytorch_amd import hip_ops
    kind, w = oracle_of(m["oracle_model"]).weight_table(m["L"])
    if kind == "position":
        return w, None
    buf = torch.full((m["B"], m["L"]), -7.0, dtype=torch.float32, device="cuda")
    hip_ops.history_pw(labels_dev, dev(w), buf, m["algo"] == "prs")
    torch.cuda.synchronize()
    pw = buf.cpu().numpy()
    assert np.array_equal(bits(pw), bits(want))
    return None, pw


def check_update(d, m, p, name, sc, params, state2):
    ref_loss, gref = float(d[p + "loss"]), d[p + "grads"]
    assert abs(sc[0] - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (sc[0], ref_loss)
    assert abs(sc[1] - float(d[p + "norm"])) <= 1e-5 * max(1.0, float(d[p + "norm"]))
    sel = np.abs(gref) > 1e-6 * max(1.0, float(np.abs(gref).max()))
    np.testing.assert_allclose(params[sel], d[p + "post_params"][sel], atol=5e-6, rtol=1e-5, err_msg="params")
    ref_state = d[p + "post_adagrad"]
    np.testing.assert_allclose(state2, ref_state, rtol=4e-5 if name.endswith("_odd") else 2e-5, atol=2e-6 * float(ref_state.max()))


# ---- the step engine, stage by stage ----------------------------------------------------------------------------------------
def _engine_step(name):
    d, m = load_golden("oracle_pw/" + name)
    kw = dict(learning_rate=m["lr"], max_gradient_norm=m["max_gradient_norm"])
    if m["algo"] == "prs":
        kw["sigma"] = m["sigma"]
    run = HipRun(m["F"], m["hidden"], m["B"], m["L"], algo="prs" if m["algo"] == "prs" else "softmax", **kw)
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        run.set_inputs(d[p + "features"], d[p + "docids"], d[p + "labels"])
        scores = run.forward(d[p + "pre_params"])
        np.testing.assert_allclose(scores, d[p + "scores"], atol=1e-5, rtol=0, err_msg="scores")
        ipw, pw = device_weights(m, run.labels, d[p + "pw"])
        ds, tail = run.loss(ipw_table=ipw, pw=pw)
        gs, ref_loss = 1.0 / float(tail[1]), float(d[p + "loss"])
        assert abs(tail[0] * gs - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (tail[0] * gs, ref_loss)
        g, tail2 = run.backward()
        np.testing.assert_allclose(tail2, tail, rtol=1e-6, atol=1e-6)
        gref = d[p + "grads"]
        np.testing.assert_allclose(g * gs, gref, err_msg="grads", **gtol(gref, name))
        params, state2, _, sc = run.update(d[p + "pre_adagrad"])
        check_update(d, m, p, name, sc, params, state2)


@pytest.mark.parametrize("name", DNN_FIXTURES)
def test_engine_matches_golden_under_both_mfma_plans(name, mfma_mode):
    _engine_step(name)


def test_engine_train_step_takes_pw_for_both_algorithms():
    """ONE ultr_train_step with pw set: the softmax path reads it as its weights, the PRS path as its per-entry ipw."""
    from ultra_pytorch_amd import engine, hip_ops
    for name in ("ipw_oracle_ubm_tiny", "prs_oracle_ubm_l50"):
        d, m = load_golden("oracle_pw/" + name)
        kw = dict(sigma=m["sigma"]) if m["algo"] == "prs" else {}
        eng = engine.StepEngine(hip_ops.DnnShape(m["F"], m["hidden"], "elu"), m["B"], m["L"], torch.device("cuda"),
                                algo="prs" if m["algo"] == "prs" else "softmax", learning_rate=m["lr"],
                                max_gradient_norm=m["max_gradient_norm"], **kw)
        table = dev(oracle_of(m["oracle_model"]).weight_table(m["L"])[1])
        buf = torch.zeros(m["B"], m["L"], device="cuda")
        for t in range(m["n_steps"]):
            p = "s%d_" % t
            prm, st = dev(d[p + "pre_params"].copy()), dev(d[p + "pre_adagrad"].copy())
            f, i, y = dev(d[p + "features"]), dev(d[p + "docids"], torch.int32), dev(d[p + "labels"])
            hip_ops.history_pw(y, table, buf, m["algo"] == "prs")
            sc = eng.train_step(prm, st, f, f.shape[0], i, y, pw=buf)
            torch.cuda.synchronize()
            assert np.array_equal(bits(buf.cpu().numpy()), bits(d[p + "pw"]))
            check_update(d, m, p, name, sc.cpu().numpy(), prm.cpu().numpy(), st.cpu().numpy())


def test_setrank_engine_matches_golden():
    from ultra_pytorch_amd import engine, hip_ops
    from tests import prs_ref
    d, m = load_golden("oracle_pw/" + SETRANK_FIXTURE)
    F, dm, H, nl, dff = prs_ref.setrank_cfg(m)
    shape = hip_ops.SetRankShape(F, dm, H, nl, dff)
    assert [n for n, _, _ in shape.layout()] == m["param_keys"]
    B, L = m["B"], m["L"]
    eng = engine.SetRankStepEngine(shape, B, L, torch.device("cuda"), algo="softmax", learning_rate=m["lr"],
                                   max_gradient_norm=m["max_gradient_norm"])
    table = dev(oracle_of(m["oracle_model"]).weight_table(L)[1])
    buf = torch.zeros(B, L, device="cuda")
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        prm, st = dev(d[p + "pre_params"].copy()), dev(d[p + "pre_adagrad"].copy())
        f, i, y = dev(np.asarray(d[p + "features"], np.float32)), dev(d[p + "docids"], torch.int32), dev(d[p + "labels"])
        hip_ops.history_pw(y, table, buf, False)
        sc = eng.train_step(prm, st, f, f.shape[0], i, y, pw=buf)
        torch.cuda.synchronize()
        assert np.array_equal(bits(buf.cpu().numpy()), bits(d[p + "pw"]))
        np.testing.assert_allclose(eng.scores.cpu().numpy(), d[p + "scores"], atol=1e-5, rtol=0, err_msg="scores")
        sc = sc.cpu().numpy()
        ref_loss, gref = float(d[p + "loss"]), d[p + "grads"]
        assert abs(sc[0] - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (sc[0], ref_loss)
        g = eng.grads[: shape.n_params].cpu().numpy() / float(sc[3])
        np.testing.assert_allclose(g, gref, rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(gref).max())), err_msg="grads")
        assert abs(sc[1] - float(d[p + "norm"])) <= 1e-5 * max(1.0, float(d[p + "norm"]))
        sel = np.abs(gref) > 1e-6 * max(1.0, float(np.abs(gref).max()))
        np.testing.assert_allclose(prm.cpu().numpy()[sel], d[p + "post_params"][sel], atol=5e-6, rtol=1e-5, err_msg="params")


# ---- the plugin classes -----------------------------------------------------------------------------------------------------
def oracle_json(tmp_path, model_file):
    """A settings-file estimator JSON that holds only "click_model" (what OraclePropensityEstimator.outputEstimatorToFile writes)."""
    path = tmp_path / ("oracle_" + model_file)
    path.write_text(json.dumps({"click_model": json.load(open(os.path.join(DATA, model_file)))}))
    assert "IPW_list" not in json.load(open(str(path)))
    return str(path)


def build_algo(algo, F, L, hidden, est_type, est_json, model="DNN", model_hparams=None, prefix="ultra_pytorch_amd"):
    from ultra_pytorch_amd.utils import find_class
    from tests.test_gpu_plugins import DataSet
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm." + CLS[algo],
           "learning_algorithm_hparams": "propensity_estimator_type=%s,propensity_estimator_json=%s" % (est_type, est_json),
           "ranking_model": "ultra_pytorch_amd.ranking_model." + model,
           "ranking_model_hparams": model_hparams if model_hparams is not None else "hidden_layer_sizes=%s" % json.dumps(hidden),
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3, 5, 10]}
    return find_class(exp["learning_algorithm"])(DataSet(F), exp)


@pytest.mark.parametrize("name", DNN_FIXTURES + [SETRANK_FIXTURE])
def test_plugin_matches_golden(name, tmp_path):
    from tests.test_gpu_plugins import load_flat, make_feed
    d, m = load_golden("oracle_pw/" + name)
    L, B = m["L"], m["B"]
    setrank = name == SETRANK_FIXTURE
    # (the `ultra.` and the `ultra_pytorch_amd.` module path name the same class)
    est_type = ORACLE if not name.endswith("_odd") else "ultra_pytorch_amd.utils.propensity_estimator.OraclePropensityEstimator"
    algo = build_algo(m["algo"], m["F"], L, m["hidden"], est_type, oracle_json(tmp_path, m["oracle_model"]),
                      model="SetRank.SetRank" if setrank else "DNN", model_hparams=SETRANK_HPARAMS if setrank else None)
    assert list(algo.model.state_dict().keys()) == m["param_keys"]
    assert algo.IPW_list is None and type(algo.propensity_estimator).__name__ == "OraclePropensityEstimator"
    buffers = set()
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        load_flat(algo.model, d[p + "pre_params"])
        algo.state_sum.copy_(torch.from_numpy(d[p + "pre_adagrad"]))
        feed = make_feed(algo, d[p + "features"], d[p + "docids"], d[p + "labels"])
        loss, out, summary = algo.train(feed)
        ref = float(d[p + "loss"])
        assert out is None and isinstance(summary, dict)
        assert abs(loss - ref) <= 1e-5 * max(1.0, abs(ref))
        g = d[p + "grads"]
        sel = np.abs(g) > 1e-6 * max(1.0, float(np.abs(g).max()))
        torch.cuda.synchronize()
        np.testing.assert_allclose(algo.model.flat_params.cpu().numpy()[sel], d[p + "post_params"][sel], atol=5e-6, rtol=1e-5)
        eng = algo._train_engines[(B, L)]
        if "pbm" in name:  # the table path: no weight launch, no buffer
            assert getattr(eng, "oracle_pw", None) is None
        else:
            assert np.array_equal(bits(eng.oracle_pw.cpu().numpy()), bits(d[p + "pw"]))
            buffers.add(id(eng.oracle_pw))
        # the host feed's entries, as the reference leaves them: Python floats of the estimator's own getPropensityForOneList
        cols = np.asarray([list(feed["propensity_weights%d" % l]) for l in range(L)], np.float64).T
        assert len(feed["propensity_weights0"]) == B and np.array_equal(bits(cols.astype(np.float32)), bits(d[p + "pw"]))
        if m["algo"] == "ipw":
            assert np.array_equal(bits(np.asarray(algo.propensity_weights, np.float64).astype(np.float32)), bits(d[p + "pw"]))
    assert algo.global_step == m["n_steps"]
    assert len(buffers) <= 1  # ONE buffer per engine, the same tensor object every step


@pytest.mark.parametrize("algo", ["ipw", "prs"])
def test_settings_file_with_only_a_click_model_constructs_and_trains(algo, tmp_path):
    """propensity_estimator_type = ...OraclePropensityEstimator with the JSON outputEstimatorToFile writes: KeyError: 'IPW_list' before
    the learners were wired to the estimator."""
    from ultra_pytorch_amd.input_layer import ClickSimulationFeed
    from tests.test_gpu_prs import DS
    F, L, B, hidden = 24, 10, 16, [16, 8]
    a = build_algo(algo, F, L, hidden, ORACLE, oracle_json(tmp_path, "ubm_0.1_1_4_1.0.json"))
    feed = ClickSimulationFeed(a, B, "click_model_json=./example/ClickModel/ubm_0.1_1_4_1.0.json")
    ds = DS(64, L, F, seed=4)
    for _ in range(2):
        loss, _, _ = a.train(feed.get_batch(ds, check_validation=True)[0])
        assert np.isfinite(loss)
    # a randomized_*.json carries its click model too: the Oracle answers from that, not from the file's IPW_list
    b = build_algo(algo, F, L, hidden, ORACLE, "./example/PropensityEstimator/randomized_pbm_0.1_1.0_4_1.0.json")
    assert b.propensity.oracle and b.propensity_estimator.click_model.model_name == "position_biased_model"
    assert b.propensity.step_weights(None, None, L)[1] is None


@pytest.mark.parametrize("algo", ["ipw", "prs"])
def test_unknown_estimator_raises(algo, tmp_path):
    with pytest.raises(NotImplementedError, match="RandomizedPropensityEstimator.*BasicPropensityEstimator.*OraclePropensityEstimator"):
        build_algo(algo, 24, 10, [16, 8], "ultra.utils.propensity_estimator.DualLearningEstimator",
                   oracle_json(tmp_path, "ubm_0.1_1_4_1.0.json"))


@pytest.mark.parametrize("est", ["RandomizedPropensityEstimator", "BasicPropensityEstimator"])
def test_table_estimators_keep_their_path(est):
    a = build_algo("ipw", 24, 10, [16, 8], "ultra.utils.propensity_estimator." + est,
                   "./example/PropensityEstimator/randomized_pbm_0.1_1.0_4_1.0.json")
    table = json.load(open(os.path.join(DATA, "randomized_pbm_0.1_1.0_4_1.0.json")))["IPW_list"]
    assert not a.propensity.oracle and a.IPW_list == [float(x) for x in table]
    assert np.array_equal(a.ipw_table.cpu().numpy(), np.asarray(table, np.float32))


# ---- the device click feed --------------------------------------------------------------------------------------------------
def _device_feed_run(tmp_path, steps=3):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd.input_layer import DeviceClickFeed
    from tests.test_gpu_plugins import load_flat
    from tests.test_gpu_prs import DS
    F, L, B, hidden = 24, 10, 16, [16, 8]
    algo = build_algo("ipw", F, L, hidden, ORACLE, oracle_json(tmp_path, "ubm_0.1_1_4_1.0.json"))
    load_flat(algo.model, O.init_params(F, hidden, seed=6))
    feed = DeviceClickFeed(algo, B, "click_model_json=./example/ClickModel/ubm_0.1_1_4_1.0.json", seed=11)
    ds = DS(64, L, F, seed=4)
    table = algo.propensity_estimator.weight_table(L)[1]
    seen = []
    for _ in range(steps):
        input_feed, _ = feed.get_batch(ds, check_validation=True)
        algo.train(input_feed)  # (queues the draw of the NEXT batch behind the step: into the feed's other buffer)
        torch.cuda.synchronize()
        labels = input_feed["labels"].cpu().numpy().copy()  # the buffer this step read
        pw = algo._train_engines[(B, L)].oracle_pw.cpu().numpy().copy()
        assert np.array_equal(bits(pw), bits(R.history_pw(labels, table, False)))
        seen.append(labels)
    assert any(((y > 0).sum(0) >= 2).any() for y in seen)  # lists with several clicks
    assert not np.array_equal(seen[0], seen[1])
    return algo.model.flat_params.cpu().numpy().copy(), algo.state_sum.cpu().numpy().copy()


def test_device_click_feed_weights_follow_the_drawn_clicks(tmp_path):
    p1, s1 = _device_feed_run(tmp_path)
    p2, s2 = _device_feed_run(tmp_path)
    assert np.array_equal(bits(p1), bits(p2)) and np.array_equal(bits(s1), bits(s2))


# ---- full size --------------------------------------------------------------------------------------------------------------
def test_config2_fused_step_with_history_weights():
    """Config 2's shape (136-d, DNN [256, 256], B 256, L 10): ONE ultr_train_step on the fused kernel with pw from ultr_history_pw.
    Loss within test_gpu_full_size's 1e-5 * max(1, |loss|) of the oracle's closed form on the step's own scores; dscores within 1e-5 of
    the largest entry (fp32 exp / log / sums over 10 positions: a few ulp of softmax x S_b, the largest term of an entry)."""
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model import init_flat_params
    F, hidden, B, L = 136, [256, 256], 256, 10
    shape = hip_ops.DnnShape(F, hidden, "elu")
    feats, ids, y = synthetic.make_batch(np.random.RandomState(17), B, L, F)
    y = (np.random.RandomState(18).uniform(size=(L, B)) < 0.35).astype(np.float32)
    y[0, ::3] = 1.0
    table = oracle_of("ubm_0.1_1_4_1.0.json").weight_table(L)[1]
    eng = engine.StepEngine(shape, B, L, torch.device("cuda"), algo="softmax", learning_rate=0.05, max_gradient_norm=5.0)
    p0 = init_flat_params(shape, seed=3).numpy()
    params, state, yd = dev(p0.copy()), dev(np.zeros_like(p0)), dev(y)
    buf = torch.zeros(B, L, device="cuda")
    hip_ops.history_pw(yd, dev(table), buf, False)
    sc = eng.train_step(params, state, dev(feats), feats.shape[0], dev(ids, torch.int32), yd, pw=buf)
    torch.cuda.synchronize()
    pw = buf.cpu().numpy()
    assert np.array_equal(bits(pw), bits(R.history_pw(y, table, False)))
    sc = sc.cpu().numpy()
    loss, ds, D = O.softmax_loss_closed_form(eng.scores.cpu().numpy(), y.T, pw)
    print("loss %.8f closed form %.8f; D %.6f closed form %.6f" % (sc[0], loss, sc[3], D))
    assert abs(sc[0] - loss) <= 1e-5 * max(1.0, abs(loss)), (sc[0], loss)
    got = eng.dscores.cpu().numpy() / float(sc[3])
    print("dscores max abs diff %.3e of max %.3e" % (np.abs(got - ds).max(), np.abs(ds).max()))
    np.testing.assert_allclose(got, ds, rtol=0, atol=1e-5 * float(np.abs(ds).max()))
