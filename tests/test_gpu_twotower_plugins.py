"""TwoTower behind the plugin seams, driven the way main.py drives a learning algorithm: the class from find_class and a settings
dict, numpy feed dicts, train() / validation() triples - on the DNN (F = 24, [32, 16], B = 7, L = 10), Linear and the small SetRank,
DLCM and GSF shapes of tests/test_gpu_adam_plugins.py, one case per grad_strategy, and from DeviceClickFeed batches.

Every train() is held to the float64 twin (tests/twotower_ref.py) fed what the GPU itself used - the engine's scores, its `grads`
buffer (raw gradient and folded step tail), the parameters, theta and optimizer state before the step - at the bars of
tests/test_gpu_twotower.py.  Once per ranking model the step is also compared end to end with the model's existing twin (the oracle for
DNN / Linear / SetRank, tests/dlcm_ref.py, tests/gsf_ref.py): its scores, and the raw gradient its backward makes of TwoTower's
dscores against the twin's gradient of the float64 loss - sign and scale included - at the bars those models' own tests hold.

Adagrad accumulators are held at STATE_RTOL relative to the accumulator.  One exemption, confined by measurement: with l2_loss > 0 the
gradient is the float32 sum g_raw / D + l2_loss p, and an entry where the two cancel by kappa = (|a| + |b|) / |a + b| > 2 is held at
STATE_RTOL x kappa.  Measured (l2_loss=0.01, max_gradient_norm=0.01, step 1, zero accumulator so s' = g^2): one entry of 1489 beyond
the plain bar, 2.15e-6 against 1.12e-6, at a LayerNorm weight p = 1: g_raw / D = -1.0520e-2, l2_loss p = +1.0000e-2, sum = -5.20e-4,
kappa = 39.5 - half an ulp of 1e-2 (4.7e-10) is 9e-7 of that sum and twice that of its square.  Every other entry of every case holds
the plain bar; tests/test_gpu_twotower.py holds it without exemption."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import adam_ref as A  # noqa: E402
from tests import loss_ref as R  # noqa: E402
from tests import twotower_ref as T  # noqa: E402
from tests.test_gpu_plugins import DataSet, make_feed  # noqa: E402

F0 = R.TAIL_FIXED
MODELS = {
    "DNN": ("DNN", "hidden_layer_sizes=[32,16]", 24, 7, 10),
    "Linear": ("Linear", "", 24, 7, 10),
    "SetRank": ("SetRank.SetRank", "d_model=32,num_heads=2,num_layers=1,diff=16", 24, 4, 5),
    "DLCM": ("DLCM", "hidden_size=20,num_heads=3", 12, 4, 5),
    "GSF": ("GSF", "hidden_layer_sizes=[20,8],group_size=2,train_shuffle=false", 12, 4, 5),
}


def make_batch(seed, F, B, L):
    """features [n_docs, F], docids [L, B] with three PADs, labels [L, B]: clicks, a grade and a fraction."""
    rng = np.random.RandomState(seed)
    n_docs = B * L - 3
    feats = rng.uniform(-1, 1, size=(n_docs, F)).astype(np.float32)
    ids = rng.permutation(B * L)
    ids = np.where(ids >= n_docs, n_docs, ids).astype(np.int32).reshape(L, B)
    y = rng.choice(np.array([0.0, 0.0, 1.0, 1.0, 0.5, 2.0], np.float32), size=(L, B))
    return feats, ids, y


def build(model, hp=""):
    from ultra_pytorch_amd.utils import find_class
    cls, model_hp, F, B, L = MODELS[model]
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.TwoTower", "learning_algorithm_hparams": hp,
           "ranking_model": "ultra_pytorch_amd.ranking_model." + cls, "ranking_model_hparams": model_hp, "max_candidate_num": L,
           "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3]}
    torch.manual_seed(3)
    return find_class(exp["learning_algorithm"])(DataSet(F), exp)


def hyper_of(algo):
    hp = algo.hparams
    gs = hp.grad_strategy if hp.grad_strategy in ("sgd", "adam") else "ada"
    return T.hyper_of(optimizer=gs, learning_rate=float(hp.learning_rate), max_gradient_norm=float(hp.max_gradient_norm),
                      l2_loss=float(hp.l2_loss), propensity_learning_rate=float(hp.propensity_learning_rate),
                      tower_combination=hp.tower_combination, mask_padding=bool(hp.mask_padding))


def host_state(algo):
    return (algo.model.flat_params.detach().cpu().numpy().copy(), algo.state_sum.cpu().numpy().copy(), algo.bias_logits.cpu().numpy().copy())


def hold_model_twin(tag, algo, sd0, p0, th0, scores, g_raw, feats, ids, y, n_docs):
    """SetRank / DLCM / GSF end to end against the model's existing twin at the parameters before the step: the scores, then the
    twin's gradient of sum(scores * dscores / B) with dscores from the float64 loss on the twin's OWN scores, against the engine's
    raw gradient / B.  Bars: the ones the models' own tests use (test_gpu_setrank.py; dlcm_ref.BAR / gsf_ref.BAR per tensor)."""
    h, sh = hyper_of(algo), algo.model.shape
    L, B = ids.shape
    name = type(algo.model).__name__

    def ds_of(s):
        return T.loss_parts(s, y, th0, h["tower_combination"], ids if h["mask_padding"] else None, n_docs)["ds"] / B

    if name == "SetRank":
        from oracle import ultr_oracle as O
        p = torch.tensor(p0, requires_grad=True)
        s = O.setrank_forward(p, sh.feature_size, sh.d_model, sh.num_heads, sh.num_layers, sh.dff, feats, ids)
        (s * torch.tensor(ds_of(s.detach().numpy()), dtype=s.dtype)).sum().backward()
        gref = p.grad.numpy()
        np.testing.assert_allclose(scores, s.detach().numpy(), atol=1e-5)
        np.testing.assert_allclose(g_raw / B, gref, rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(gref).max())))
        return
    if name == "DLCM":
        from tests import dlcm_ref as M
        ref = lambda d: M.reference(sd0, sh.feature_size, sh.hidden_size, sh.num_heads, feats, ids, d)  # noqa: E731
    else:
        from tests import gsf_ref as M
        ref = lambda d: M.reference(sd0, sh.feature_size, sh.hidden, sh.group_size, feats, ids, d, activation=sh.activation)  # noqa: E731
    s_ref, _ = ref(torch.zeros(B, L))
    s_ref, grads = ref(torch.tensor(ds_of(s_ref.numpy())))
    e = M.rel_err(torch.tensor(scores), s_ref)
    assert e <= M.BAR, (tag, "scores", e)
    worst = 0.0
    for k, shape, off in sh.layout():
        got = torch.tensor(g_raw[off:off + int(np.prod(shape))].astype(np.float64) / B).view(*shape)
        e = M.rel_err(got, grads[k])
        worst = max(worst, e)
        assert e <= M.BAR, (tag, "gradient", k, e)
    print("%s against the model's twin: largest gradient error %.3g of max|ref| (bar %.0e)" % (tag, worst, M.BAR))


def hold_train(tag, algo, eng, before, after, loss, ids, y, n_docs, t, dnn=None, pads=3, model_twin=None):
    """One train() against the twin put at `before`: the loss kernel on the engine's scores, then the update on its gradients."""
    h = hyper_of(algo)
    L, B = ids.shape
    P = algo.model.shape.n_params
    p0, st0, th0 = before
    p1, st1, th1 = after
    g = eng.grads.cpu().numpy()
    g_raw, tail, sc = g[:P], g[P:].astype(np.float64), eng.scalars.cpu().numpy()
    scores, ds = eng.scores.cpu().numpy(), eng.dscores.cpu().numpy()
    ref = T.loss_parts(scores, y, th0, h["tower_combination"], ids if h["mask_padding"] else None, n_docs)
    e_ds, e_tail = T.excess(ds, ref["ds"], ref["ds_abs"]), T.excess(tail, ref["tail"], ref["tail_abs"])
    print("%s t=%d: dscores %.3e, tail %.3e (bar %.0e)" % (tag, t, e_ds, e_tail, R.TERMS_RTOL))
    assert e_ds <= R.TERMS_RTOL and e_tail <= R.TERMS_RTOL and tail[1] == B
    if h["mask_padding"]:
        assert (ds[~ref["live"]] == 0.0).all() and (pads is None or (~ref["live"]).sum() == pads)
    if model_twin is not None:
        hold_model_twin(tag, algo, model_twin[0], p0, th0, scores, g_raw, model_twin[1], ids, y, n_docs)
    n_state = T.state_floats(h["optimizer"], P, L)
    assert algo.state_sum.numel() == max(n_state, P if n_state == 0 else n_state)
    tw = T.Twin([torch.tensor(p0.astype(np.float64))], th0, h)
    tw.load(p0, th0, st0[:n_state], t - 1)
    r = tw.step(y, ids, n_docs, scores=scores, force_grad=g_raw.astype(np.float64) / B, force_theta_grad=tail[F0:F0 + L] / B)
    if dnn is not None:  # the ranker against autograd through the oracle's DNN, at smoke()'s bar (rtol 1e-4, atol 1e-6)
        feats, F, hidden = dnn
        tw2 = T.dnn_twin(p0, th0, h, F, hidden, feats, ids)
        r2 = tw2.step(y, ids, n_docs)
        np.testing.assert_allclose(scores, r2["scores"], atol=1e-5)
        np.testing.assert_allclose(g_raw.astype(np.float64) / B, r2["grad"], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(tail[F0:F0 + L] / B, r2["theta_grad"], rtol=1e-4, atol=1e-6)
        assert abs(loss - r2["loss"]) <= 1e-5 * max(1.0, abs(r2["loss"]))
    ss = float((g_raw.astype(np.float64) ** 2).sum())
    want = (r["loss"], r["norm"], r["coef"], float(B), 0.0, 0.0, r["pnorm"], ss)
    for k, w in enumerate(want):
        assert abs(float(sc[k]) - w) <= R.SCALAR_RTOL * max(1.0, abs(w)), (tag, k, float(sc[k]), w)
    assert loss == float(sc[0])  # train() returns scalars[0]
    ref_p, ref_th, ref_st = tw.flat(), tw.theta.detach().numpy(), tw.state()
    e_th = float(np.abs(th1 - ref_th).max())
    assert np.isfinite(th1).all() and e_th <= R.AUX_ATOL, (tag, "theta", e_th)
    if h["optimizer"] == "adam":
        terms = np.concatenate([(1 - A.B1) * r["g_terms"], (1 - A.B2) * r["g_terms"] ** 2, (1 - A.B1) * np.abs(r["theta_final"]),
                                (1 - A.B2) * r["theta_final"] ** 2])
        e_p, e_s = A.excess(p1, ref_p, h["learning_rate"]), A.moment_excess(st1, ref_st, st0, terms)
        print("%s t=%d: parameters %.3e (bar %.3e), moments %.3e (bar %.3e)" % (tag, t, e_p, A.BAR, e_s, A.MOMENT_RTOL))
        assert e_p <= A.BAR and e_s <= A.MOMENT_RTOL
    else:
        e_p = float(np.abs(p1 - ref_p).max())
        print("%s t=%d: parameters %.3e (bar %.3e), theta %.3e" % (tag, t, e_p, R.PARAM_ATOL, e_th))
        assert np.isfinite(p1).all() and e_p <= R.PARAM_ATOL, (tag, "params", e_p)
        if h["optimizer"] == "ada":
            # STATE_RTOL relative to the accumulator, as tests/test_gpu_losses.py - for every entry whose gradient is not a cancelling
            # sum.  With l2_loss > 0 the update forms g = (a + b) coef, a = g_raw / D, b = l2_loss p, in float32: where a and b have
            # opposite signs the rounding of a and b (each of order 2^-24 of ITSELF) is kappa = (|a| + |b|) / |a + b| times larger
            # relative to g, and twice that relative to g^2, the accumulator's increment.  Only entries with kappa > 2 get
            # STATE_RTOL x kappa; the evidence is printed, and the module docstring records what was measured.
            rel = np.abs(st1 - ref_st) / np.maximum(ref_st, 1e-30)
            a_, b_ = g_raw.astype(np.float64) / B, h["l2_loss"] * p0.astype(np.float64)
            kappa = np.ones(len(ref_st))
            kappa[:P] = (np.abs(a_) + np.abs(b_)) / np.maximum(np.abs(a_ + b_), 1e-300)
            allowed = np.where(kappa > 2.0, R.STATE_RTOL * kappa, R.STATE_RTOL)
            e_s, k = float(rel.max()), int(rel.argmax())
            print("%s t=%d: accumulators %.3e (bar %.3e); %d entries with kappa > 2" % (tag, t, e_s, R.STATE_RTOL, int((kappa > 2.0).sum())))
            for j in np.nonzero(rel > R.STATE_RTOL)[0]:
                print("  entry %d beyond the plain bar: %.3e; g_raw / D = %.9e, l2_loss p = %.9e, sum = %.9e, kappa = %.3g, coef = %.9e, "
                      "s0 = %.3e, s' = %.9e (twin %.9e)" % (j, rel[j], a_[j], b_[j], a_[j] + b_[j], kappa[j], r["coef"], st0[j], st1[j], ref_st[j]))
            assert (rel <= allowed).all(), (tag, "state", e_s, k, float(kappa[k]))
        else:
            assert np.array_equal(st1, st0)
    assert not np.array_equal(p1, p0) and not np.array_equal(th1, th0)


def run_two_steps(model, hp):
    cls, model_hp, F, B, L = MODELS[model]
    algo = build(model, hp)
    assert type(algo).__name__ == "TwoTower" and algo.opt_steps == 0 and not algo.state_sum.any()
    init = T.LN9 if algo.hparams.tower_combination == "product" else 0.0
    assert tuple(algo.bias_logits.shape) == (L,) and algo.bias_logits.is_cuda
    assert np.array_equal(algo.bias_logits.cpu().numpy(), np.full(L, init, np.float32))
    dnn_hidden = {"DNN": [32, 16], "Linear": []}.get(model)
    other = model in ("SetRank", "DLCM", "GSF")
    for t in (1, 2):
        feats, ids, y = make_batch(10 * t, F, B, L)
        before = host_state(algo)
        sd0 = {k: v.detach().cpu().clone() for k, v in algo.model.state_dict().items()} if other else None
        loss, out, summary = algo.train(make_feed(algo, feats, ids, y))
        torch.cuda.synchronize()
        assert out is None and isinstance(summary, dict) and np.isfinite(loss) and algo.global_step == t and algo.opt_steps == t
        eng = algo._train_engines[(B, L)]
        hold_train("%s [%s]" % (model, hp), algo, eng, before, host_state(algo), loss, ids, y, feats.shape[0], t,
                   dnn=None if dnn_hidden is None else (feats, F, dnn_hidden), model_twin=(sd0, feats) if other else None)
    feats, ids, y = make_batch(99, F, B, L)
    _, scores, summary = algo.validation(make_feed(algo, feats, ids, y))
    assert tuple(scores.shape) == (B, L) and torch.isfinite(scores).all() and 0.0 <= summary["ndcg_3"] <= 1.0
    return algo


@pytest.mark.parametrize("model", list(MODELS))
def test_two_train_steps_per_ranking_model(model):
    algo = run_two_steps(model, "")
    p = algo.propensity
    assert tuple(p.shape) == (1, MODELS[model][4]) and ((p > 0) & (p < 1)).all()


@pytest.mark.parametrize("hp", ["grad_strategy=sgd,learning_rate=0.1,propensity_learning_rate=0.3",
                                "grad_strategy=adam,tower_combination=sum,mask_padding=False",
                                "grad_strategy=ada,l2_loss=0.01,max_gradient_norm=0.01,tower_combination=sum"])
def test_each_grad_strategy_on_the_dnn(hp):
    algo = run_two_steps("DNN", hp)
    eng = algo._train_engines[(7, 10)]
    if "max_gradient_norm=0.01" in hp:
        assert float(eng.scalars[2]) < 1.0  # l2_loss > 0 and the clip still applies
    if "tower_combination=sum" in hp:
        with pytest.raises(ValueError):
            algo.propensity


def test_an_unknown_combination_is_refused_at_construction():
    with pytest.raises(ValueError, match="tower_combination"):
        build("DNN", "tower_combination=ratio")


def test_three_steps_from_device_click_feed_batches():
    """Every step against the twin on the arrays read back from its batch, at the bars of the feed-dict steps.  The draw of the next
    batch rides behind the step (ultr_feed_train_step) whatever the algorithm: the batches handed out while training are the ones
    a feed of the same seed hands out when nobody trains, they differ from one another and carry PADs."""
    from tests.test_gpu_feed import DS
    from ultra_pytorch_amd.input_layer import DeviceClickFeed
    from ultra_pytorch_amd.utils import find_class
    F, L, B = 16, 10, 64
    ds = DS(200, (6, 10), F, seed=2)
    ds.pad(L)
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.TwoTower", "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=[32,16]",
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3]}
    torch.manual_seed(5)
    algo = find_class(exp["learning_algorithm"])(ds, exp)
    feed, spot = DeviceClickFeed(algo, B, "", seed=1), DeviceClickFeed(algo, B, "", seed=1)
    seen = []
    for t in (1, 2, 3):
        input_feed, _ = feed.get_batch(ds, check_validation=True)
        ids, y = input_feed["docids"].cpu().numpy().copy(), input_feed["labels"].cpu().numpy().copy()
        feats, n_docs = input_feed["features"].cpu().numpy().copy(), int(input_feed["n_docs"])
        seen.append((ids, y))
        assert (ids == n_docs).any()  # the batch has PADs: they are masked
        before = host_state(algo)
        loss, _, _ = algo.train(input_feed)
        torch.cuda.synchronize()
        assert np.isfinite(loss) and algo.global_step == t
        if t > 1:
            assert algo._train_engines[(B, L)].next_click_source is feed  # the engine drew this batch behind the step before
        hold_train("device feed", algo, algo._train_engines[(B, L)], before, host_state(algo), loss, ids, y, n_docs, t,
                   dnn=(feats[:n_docs], F, [32, 16]), pads=None)
    assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[1][0], seen[2][0])
    for k, (ids, y) in enumerate(seen):  # ... and they are the batches of a feed nobody draws ahead of
        f, _ = spot.get_batch(ds, check_validation=True)
        np.testing.assert_array_equal(f["docids"].cpu().numpy(), ids, err_msg="batch %d" % k)
        np.testing.assert_array_equal(f["labels"].cpu().numpy(), y, err_msg="batch %d" % k)
