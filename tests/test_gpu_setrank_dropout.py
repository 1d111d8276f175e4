"""SetRank's dropout on the GPU (csrc/ultr_sr_dropout.hip, ultr_setrank_forward_dropout / ultr_setrank_backward_dropout): rate 0 is
the plain step bit for bit, the step recorded from the reference with site masks, forward / loss / backward against the float64
restatement with restated masks (tests/setrank_dropout_ref.py) at the bars of test_gpu_setrank, determinism in (seed, step, stream),
evaluation that never drops, the plug-in classes, and the extra scratch at its declared size on the guarded arena."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import setrank_dropout_ref as R  # noqa: E402
from tests.hipref import dev, load_golden  # noqa: E402

KW = dict(learning_rate=0.05, max_gradient_norm=5.0)


def make_engine(shape, B, L, seed=0, step=0, stream=0, **kw):
    from ultra_pytorch_amd import engine
    eng = engine.SetRankStepEngine(shape, B, L, torch.device("cuda"), algo="softmax", **(kw or KW))
    shape.dropout_seed, shape.dropout_step, eng.dropout_stream = seed, step, stream
    return eng


def run_step(shape, B, L, params, state, feats, ids, labels, ipw, seed=0, step=0, stream=0, update=True, **kw):
    """One step through the stage calls of SetRankStepEngine: (scores, grads | tail, params, state, scalars)."""
    eng = make_engine(shape, B, L, seed, step, stream, **kw)
    p, s = dev(params.copy()), dev(state.copy())
    f = dev(np.asarray(feats, np.float32))
    i, y = dev(ids, torch.int32), dev(labels, torch.float32)
    eng.forward(p, f, f.shape[0], i, train=True)
    torch.cuda.synchronize()
    scores = eng.scores.cpu().numpy().copy()
    eng.loss(y, ipw_table=None if ipw is None else dev(np.asarray(ipw, np.float32)))
    eng.backward(p, f, f.shape[0], i)
    torch.cuda.synchronize()
    g = eng.grads.cpu().numpy().copy()
    if update:
        eng.update(p, s)
        torch.cuda.synchronize()
    out = scores, g, p.cpu().numpy(), s.cpu().numpy(), eng.scalars.cpu().numpy()
    eng.close()
    return out


def batch(B, L, F):
    from ultra_pytorch_amd import synthetic
    rng = np.random.RandomState(11)
    feats, ids, y = synthetic.make_batch(rng, B, L, F, n_pad=2 if L > 8 else 0)
    return feats, ids, y, np.asarray(synthetic.load_ipw(), np.float32)


def init(shape):
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    return init_setrank_params(shape, seed=9).numpy()


# ---- 1. rate 0 is today's step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,F,dm,H,nl,dff", [(5, 100, 220, 256, 8, 2, 64), (3, 37, 20, 48, 6, 1, 20)])
def test_rate_0_is_the_plain_step_bitwise(B, L, F, dm, H, nl, dff):
    from ultra_pytorch_amd import hip_ops
    shape = hip_ops.SetRankShape(F, dm, H, nl, dff)
    feats, ids, y, ipw = batch(B, L, F)
    p = dev(init(shape))
    f, i, yy, tab = dev(feats), dev(ids, torch.int32), dev(y, torch.float32), dev(ipw)
    lib, desc = shape.lib, ctypes.byref(shape.desc)
    scratch = torch.empty(max(shape.dropout_workspace_bytes(B * L) // 4, 1), dtype=torch.float32, device="cuda")
    assert shape.dropout_workspace_bytes(B * L) >= 4 * B * L * dm
    got = {}
    for mode in ("plain", "null", "rate0"):
        eng = make_engine(shape, B, L)
        drop = hip_ops.setrank_dropout(0.0, 77, 5, 1, scratch) if mode == "rate0" else None
        dref = ctypes.byref(drop) if drop is not None else None
        st = ctypes.c_void_p(hip_ops.raw_stream())
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        if mode == "plain":
            hip_ops.setrank_forward(shape, p, f, f.shape[0], i, B, L, eng.scores, eng.saved)
        else:
            hip_ops.check(lib.ultr_setrank_forward_dropout(desc, ptr(p), ptr(f), f.shape[0], ptr(i), B, L, ptr(eng.scores), ptr(eng.saved),
                                                           dref, st), "ultr_setrank_forward_dropout")
        eng.loss(yy, ipw_table=tab)
        n_parts = hip_ops.loss_part_count(B)
        if mode == "plain":
            hip_ops.setrank_backward(shape, p, B, L, eng.saved, eng.dscores, eng.loss_ws, n_parts, eng.sr_ws, eng.grads)
        else:
            hip_ops.check(lib.ultr_setrank_backward_dropout(desc, ptr(p), B, L, ptr(eng.saved), ptr(eng.dscores), ptr(eng.loss_ws), n_parts,
                                                            ptr(eng.sr_ws), ptr(eng.grads), dref, st), "ultr_setrank_backward_dropout")
        torch.cuda.synchronize()
        got[mode] = (eng.scores.cpu().numpy().view(np.int32).copy(), eng.grads.cpu().numpy().view(np.int32).copy())
        eng.close()
    for mode in ("null", "rate0"):
        assert np.array_equal(got[mode][0], got["plain"][0]), mode + ": scores"
        assert np.array_equal(got[mode][1], got["plain"][1]), mode + ": gradient vector"
    assert np.isfinite(got["plain"][1].view(np.float32)).all() and np.abs(got["plain"][1].view(np.float32)).max() > 0


def test_bad_rate_and_short_scratch_are_refused():
    from ultra_pytorch_amd import _lib, hip_ops
    B, L = 3, 7
    shape = hip_ops.SetRankShape(20, 48, 6, 1, 20)
    feats, ids, y, ipw = batch(B, L, 20)
    p, f, i = dev(init(shape)), dev(feats), dev(ids, torch.int32)
    eng = make_engine(shape, B, L)
    for bad in (1.0, -0.1, float("nan")):
        d = _lib.SetRankDropout()
        d.rate = bad
        with pytest.raises(_lib.UltrHipError):
            hip_ops.setrank_forward(shape, p, f, f.shape[0], i, B, L, eng.scores, eng.saved, dropout=d)
    d = hip_ops.setrank_dropout(0.5, 1, 0, 0, torch.empty(4, dtype=torch.float32, device="cuda"))
    hip_ops.setrank_forward(shape, p, f, f.shape[0], i, B, L, eng.scores, eng.saved, dropout=d)
    eng.loss(dev(y, torch.float32), ipw_table=dev(ipw))
    with pytest.raises(_lib.UltrHipError):  # a 16-byte scratch: ULTR_E_WORKSPACE, nothing launched
        hip_ops.setrank_backward(shape, p, B, L, eng.saved, eng.dscores, eng.loss_ws, hip_ops.loss_part_count(B), eng.sr_ws, eng.grads,
                                 dropout=d)
    torch.cuda.synchronize()
    eng.close()


# ---- 2. the golden step ----------------------------------------------------------------------------------------------------------------
def test_golden_step_with_site_masks():
    from ultra_pytorch_amd import hip_ops
    d, m = load_golden("setrank_dropout_tiny")
    F, dm, H, nl, dff = 20, 32, 4, 2, 16
    shape = hip_ops.SetRankShape(F, dm, H, nl, dff, rate=float(d["rate"]))
    assert [n for n, _, _ in shape.layout()] == m["param_keys"]
    B, L = m["B"], m["L"]
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        scores, g, params, state, sc = run_step(shape, B, L, d[p + "pre_params"], d[p + "pre_adagrad"], d[p + "features"],
                                                d[p + "docids"], d[p + "labels"], d["ipw_list"], seed=int(d["seed"]),
                                                step=int(d["steps"][t]), learning_rate=m["lr"], max_gradient_norm=m["max_gradient_norm"])
        assert shape.dropout_step == int(d["steps"][t]) + 1
        print("step %d: max |score diff| %.3g" % (t, float(np.abs(scores - d[p + "scores"]).max())))
        np.testing.assert_allclose(scores, d[p + "scores"], atol=1e-5, rtol=0, err_msg="scores")
        ref_loss = float(d[p + "loss"])
        assert abs(sc[0] - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (sc[0], ref_loss)
        gref = d[p + "grads"]
        gs = 1.0 / float(sc[3])
        np.testing.assert_allclose(g[: shape.n_params] * gs, gref, rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(gref).max())),
                                   err_msg="grads")
        sel = np.abs(gref) > 1e-6 * max(1.0, float(np.abs(gref).max()))
        np.testing.assert_allclose(params[sel], d[p + "post_params"][sel], atol=5e-6, rtol=1e-5, err_msg="params")


# ---- 3. against the float64 restatement ---------------------------------------------------------------------------------------------------
SHAPES = [(2, 5, 7, 30, 3, 1, 9),           # d_model no multiple of 4: a Philox quad straddles the row end
          (3, 37, 20, 48, 6, 1, 20),        # ragged row block, general row kernels, PAD rows
          (5, 100, 220, 256, 8, 2, 64),     # config 5's widths: the v4 row kernels, split-half products, five sites
          (4, 120, 24, 64, 2, 1, 16)]       # 8 token blocks in attention
CASES = [s + (False,) for s in SHAPES] + [SHAPES[2] + (True,)]


@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("B,L,F,dm,H,nl,dff,fp32_products", CASES,
                         ids=["B%d_L%d_F%d_d%d_H%d_nl%d_dff%d%s" % (c[:7] + ("_fp32" if c[7] else "",)) for c in CASES])
def test_step_against_the_restatement(B, L, F, dm, H, nl, dff, fp32_products, rate):
    from ultra_pytorch_amd import _lib, hip_ops
    shape = hip_ops.SetRankShape(F, dm, H, nl, dff, rate=rate)
    if fp32_products:
        shape.desc.flags = int(shape.desc.flags) | _lib.MODEL_FP32_PRODUCTS
    feats, ids, y, ipw = batch(B, L, F)
    p0 = init(shape)
    seed, step = 0x1234_5678_9ABC_DEF0, 3
    scores, g, _, _, sc = run_step(shape, B, L, p0, np.zeros_like(p0), feats, ids, y, ipw, seed=seed, step=step)
    r = R.train_step(p0, np.zeros_like(p0), (F, dm, H, nl, dff), feats, ids, y, ipw_list=ipw, rate=rate, seed=seed, step=step)
    gref = r["grads"]
    gs = 1.0 / float(sc[3])
    print("rate %.1f: scores %.3g, loss %.3g, grads %.3g (of max %.3g)" % (
        rate, float(np.abs(scores - r["scores"]).max()), abs(float(sc[0]) - r["loss"]),
        float(np.abs(g[: shape.n_params] * gs - gref).max()), float(np.abs(gref).max())))
    np.testing.assert_allclose(scores, r["scores"], atol=1e-5)
    assert abs(float(sc[0]) - r["loss"]) <= 1e-5 * max(1.0, abs(r["loss"]))
    np.testing.assert_allclose(g[: shape.n_params] * gs, gref, rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(gref).max())))
    # the masks are what is being tested: the same step without them is somewhere else
    r0 = R.train_step(p0, np.zeros_like(p0), (F, dm, H, nl, dff), feats, ids, y, ipw_list=ipw, rate=0.0)
    assert float(np.abs(r0["scores"] - r["scores"]).max()) > 1e-3


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------------
def test_same_key_same_bits_other_key_other_scores():
    from ultra_pytorch_amd import hip_ops
    B, L, F, dm, H, nl, dff = 3, 37, 20, 48, 6, 1, 20
    shape = hip_ops.SetRankShape(F, dm, H, nl, dff, rate=0.3)
    feats, ids, y, ipw = batch(B, L, F)
    p0 = init(shape)

    def go(step, stream):
        s, g, _, _, _ = run_step(shape, B, L, p0, np.zeros_like(p0), feats, ids, y, ipw, seed=99, step=step, stream=stream)
        return s.view(np.int32), g.view(np.int32)

    a, b = go(4, 0), go(4, 0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(go(5, 0)[0], a[0])
    assert not np.array_equal(go(4, 1)[0], a[0])


# ---- 5. evaluation never drops ---------------------------------------------------------------------------------------------------------------
def test_evaluation_never_drops(monkeypatch):
    from tests.test_gpu_eval_set import DS, NAMES, _algo
    from tests.test_gpu_plugins import load_flat, make_feed
    from ultra_pytorch_amd import input_layer
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    L, B, F = 12, 8, 24
    ds = DS(21, L, F, seed=6)
    hp = "d_model=32,num_heads=2,num_layers=1,diff=16"
    plain, drop = _algo(F, L, NAMES, "SetRank.SetRank", hp), _algo(F, L, NAMES, "SetRank.SetRank", hp + ",rate=0.3")
    assert drop.model.shape.rate == pytest.approx(0.3) and plain.model.shape.rate == 0.0

    def evaluate(algo):
        dfeed = input_layer.DeviceDirectLabelFeed(algo, B, "")
        _, set_scores, _ = algo.validation_set(dfeed, ds, want_scores=True)
        input_feed, _ = dfeed.get_next_batch(0, ds, check_validation=False)
        _, out, _ = algo.validation(input_feed)
        return set_scores.clone(), out.clone()

    rng = np.random.RandomState(2)
    feats = rng.uniform(-1, 1, size=(B * L, F)).astype(np.float32)
    ids = np.arange(B * L, dtype=np.int32).reshape(L, B)
    labels = (rng.uniform(size=(L, B)) < 0.4).astype(np.float32)
    labels[0] = 1.0
    for phase in ("before", "after"):
        load_flat(plain.model, drop.model.flat_params.cpu().numpy())
        a, b = evaluate(plain), evaluate(drop)
        assert torch.equal(a[0], b[0]), phase + " a training step: validation_set"
        assert torch.equal(a[1], b[1]), phase + " a training step: validation"
        if phase == "before":
            before = drop.model.flat_params.clone()
            loss, _, _ = drop.train(make_feed(drop, feats, ids, labels))
            assert math.isfinite(loss) and drop.model.dropout_step == 1 and not torch.equal(before, drop.model.flat_params)
    assert drop.model.dropout_step == 1  # evaluation counts no step


# ---- 6. the plug-in classes -------------------------------------------------------------------------------------------------------------------
def test_plugin_trains_with_the_restated_masks():
    from tests.test_gpu_plugins import DataSet, load_flat, make_feed
    from ultra_pytorch_amd.ranking_model.SetRank import SetRank
    from ultra_pytorch_amd.utils import find_class
    d, m = load_golden("setrank_dropout_tiny")
    cfg = (20, 32, 4, 2, 16)
    hp = "d_model=32,num_heads=4,num_layers=2,diff=16"
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.IPWrank", "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.SetRank.SetRank", "ranking_model_hparams": hp + ",rate=0.25",
           "max_candidate_num": m["L"], "selection_bias_cutoff": m["L"], "metrics": ["ndcg"], "metrics_topn": [1, 3, 5, 10]}
    torch.manual_seed(1234)
    algo = find_class(exp["learning_algorithm"])(DataSet(m["F"]), exp)
    model = algo.model
    assert model.dropout_seed == 1234 and model.dropout_step == 0 and model.training
    for t in range(2):
        p = "s%d_" % t
        pre, pre_state = model.flat_params.cpu().numpy().copy(), algo.state_sum.cpu().numpy().copy()
        loss, out, _ = algo.train(make_feed(algo, d[p + "features"], d[p + "docids"], d[p + "labels"]))
        r = R.train_step(pre, pre_state, cfg, d[p + "features"], d[p + "docids"], d[p + "labels"], ipw_list=d["ipw_list"], rate=0.25,
                         seed=1234, step=t, lr=m["lr"], max_norm=m["max_gradient_norm"])
        print("step %d: loss %.7f restated %.7f" % (t, loss, r["loss"]))
        assert out is None and abs(loss - r["loss"]) <= 1e-5 * max(1.0, abs(r["loss"]))
        g = r["grads"]
        sel = np.abs(g) > 1e-6 * max(1.0, float(np.abs(g).max()))
        np.testing.assert_allclose(model.flat_params.cpu().numpy()[sel], r["params"][sel], atol=5e-6, rtol=1e-5)
    assert model.dropout_step == 2
    # evaluation mode: build() is the rate-0 forward
    xs = [torch.from_numpy(d["s0_features"][d["s0_docids"][l]]) for l in range(m["L"])]
    model.eval()
    outs = model.build(xs)
    twin = SetRank(hp, m["F"]).cuda()
    load_flat(twin, model.flat_params.cpu().numpy())
    twin.eval()
    want = twin.build(xs)
    assert model.dropout_step == 2 and all(torch.equal(a, b) for a, b in zip(outs, want))
    # training mode: build() drops, with the model's next step
    model.train()
    dropped = model.build(xs)
    assert model.dropout_step == 3 and not all(torch.equal(a, b) for a, b in zip(dropped, want))
    x = R.gather(d["s0_features"], d["s0_docids"])
    ref = R.forward(torch.from_numpy(model.flat_params.cpu().numpy()).double(), cfg, x, R.masks(1234, 2, 0, m["B"], m["L"], 32, 2, 0.25))
    got = torch.cat(dropped, dim=1).cpu().numpy()  # [B, L]
    np.testing.assert_allclose(got, ref.numpy(), atol=1e-5)
    # the same model under DLA
    exp2 = dict(exp, learning_algorithm="ultra_pytorch_amd.learning_algorithm.DLA")
    dla = find_class(exp2["learning_algorithm"])(DataSet(m["F"]), exp2)
    load_flat(dla.model, model.flat_params.cpu().numpy())
    loss, _, _ = dla.train(make_feed(dla, d["s0_features"], d["s0_docids"], d["s0_labels"]))
    assert math.isfinite(loss) and dla.model.dropout_step == 1


# ---- 7. the workspace contract ----------------------------------------------------------------------------------------------------------------
def _guarded_run(guarded):
    from tests import guarded as G
    from tests import test_gpu_workspace_bounds as WB
    from ultra_pytorch_amd import hip_ops
    B, L, F, dm, H, nl, dff = 3, 37, 20, 48, 6, 1, 20
    shape = hip_ops.SetRankShape(F, dm, H, nl, dff, rate=0.1)
    feats, ids, y, ipw = batch(B, L, F)
    p0 = init(shape)
    eng = make_engine(shape, B, L, seed=31, step=0)
    n_drop = shape.dropout_workspace_bytes(B * L) // 4
    arena = None
    if guarded:
        sizes = [t.numel() * t.element_size() for _, t in WB._device_tensors(eng)] + [4 * n_drop]
        arena = G.Arena(torch.device("cuda"), G.bytes_for(sizes))
        WB.guard_engine(eng, arena)
        eng.drop_ws = arena.view(n_drop, name="drop_ws")  # exactly the declared size, poisoned
    p, st = dev(p0.copy()), dev(np.zeros_like(p0))
    f, i, yy, tab = dev(feats), dev(ids, torch.int32), dev(y, torch.float32), dev(ipw)
    eng.train_step(p, st, f, feats.shape[0], i, yy, ipw_table=tab)
    torch.cuda.synchronize()
    if arena is not None:
        arena.check()
        assert arena.untouched(eng.scores) == 0 and arena.untouched(eng.drop_ws) < n_drop  # the step ran on the arena's views
    out = WB.snapshot(eng, p, st, None)
    eng.close()
    return out


def test_dropout_step_stays_inside_its_workspaces():
    from tests import test_gpu_workspace_bounds as WB
    WB.hold_equal(_guarded_run(False), _guarded_run(True), "SetRank dropout step (rate 0.1)")
