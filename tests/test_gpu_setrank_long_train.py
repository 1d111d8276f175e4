"""SetRank training beyond the one-pass attention backward on the GPU (csrc/ultr_sr_attn_long.hip: sr_attn_bwd_long_kernel,
sr_attn_bwd_long_scalar_kernel), for a model with attention_backward=streaming: one step against the float64 reference of
tests/sr_attn_bwd_ref.py at the kernels' edges, with peaked attention, the same kernels below the hand-over point against the oracle,
the bits of a short list and of a repeated step, the workspace contract on the guarded arena, the IPWrank plug-in at
rank_list_size 300, and a dropout step.  Measured distances: profiles/setrank_long_train.md."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sr_attn_bwd_ref as RB  # noqa: E402
from tests import sr_attn_long_ref as R  # noqa: E402
from tests.hipref import dev  # noqa: E402
from tests.test_gpu_setrank_long import SHORT_MODELS, knob  # noqa: E402,F401  (knob: the ULTR_SR_ATTN_LONG_MIN fixture)

# (B, L, F, d, H, layers, dff)
EDGE_SHAPES = [(2, 129, 24, 64, 2, 1, 16),      # one token past the one-pass bound, head depth 32
               (2, 257, 24, 64, 4, 1, 16),      # two tiles + 1, head depth 16
               (3, 385, 24, 64, 1, 2, 16),      # head depth 64, two layers
               (2, 121, 20, 48, 6, 1, 20),      # head depth 8: one token past the scalar one-pass backward
               (2, 300, 20, 48, 6, 1, 20),      # ... and five partner tiles of 64
               (2, 1251, 136, 256, 8, 2, 64)]   # the MSLR length at full width
PEAKED_SHAPE = (2, 300, 24, 64, 4, 1, 16)
KW = dict(learning_rate=0.05, max_gradient_norm=5.0)


def _id(s):
    return "B%d_L%d_F%d_d%d_H%d_nl%d_dff%d" % tuple(s)


def streaming(F, dm, H, nl, dff, **kw):
    from ultra_pytorch_amd import hip_ops
    return hip_ops.SetRankShape(F, dm, H, nl, dff, attention_backward="streaming", **kw)


@functools.lru_cache(maxsize=None)
def case(shape, gain=None):
    """Inputs of one shape and both references of its step, computed once and read-only: (p0, feats, ids, labels, ipw, fp32 oracle
    step, float64 step)."""
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    B, L, F, dm, H, nl, dff = shape
    sh = streaming(F, dm, H, nl, dff)
    feats, ids, y = synthetic.make_batch(np.random.RandomState(11), B, L, F, n_pad=2)
    ipw = np.asarray(synthetic.load_ipw(), np.float32)
    p0 = init_setrank_params(sh, seed=9).numpy()
    if gain is not None:
        p0 = R.peaked(p0, sh, gain)
    r32 = O.train_step_setrank_softmax(p0, np.zeros_like(p0), (F, dm, H, nl, dff), feats, ids, y, ipw_list=ipw, lr=0.05, max_norm=5.0)
    r64 = RB.train_step(p0, (F, dm, H, nl, dff), feats, ids, y, ipw_list=ipw)
    for a in (p0, feats, ids, y, ipw):
        a.setflags(write=False)
    return p0, feats, ids, y, ipw, r32, r64


def run(sh, B, L, p0, feats, ids, y, ipw):
    """One step through the stage calls: (scores, gradient / the step's scale, loss, raw grads | tail, params after the update)."""
    from tests.test_gpu_setrank import run_step
    scores, g, params, _, sc = run_step(sh, B, L, KW, p0, np.zeros_like(p0), feats.copy(), ids.copy(), y.copy(), ipw.copy())
    return scores, g[: sh.n_params] / float(sc[3]), float(sc[0]), g, params


def hold_to_float64(what, got, r32, r64):
    """Per quantity the bound is the larger of the project's bar (scores 1e-5; loss 1e-5 relative; gradients rtol 1e-5 and
    atol 2e-6 max(1, max|g|)) and 4 x the fp32 oracle's own distance to float64 on the same inputs: fp32 sums over 1251 terms cannot
    beat the fp32 oracle's own rounding.  Prints what it measures before it asserts."""
    scores, grads, loss = got
    s64, g64, l64 = r64["scores"], r64["grads"], r64["loss"]
    o_s = float(np.abs(r32["scores"] - s64).max())
    o_l = abs(r32["loss"] - l64)
    o_g = float(np.abs(r32["grads"] - g64).max())
    e_s = float(np.abs(scores - s64).max())
    e_l = abs(loss - l64)
    gerr = np.abs(grads - g64)
    gmax = float(np.abs(g64).max())
    gbar = 1e-5 * np.abs(g64) + 2e-6 * max(1.0, gmax)
    print("%s: scores %.3g (oracle %.3g, max|s| %.3g), loss %.3g (oracle %.3g), grads %.3g (oracle %.3g, max|g| %.3g)"
          % (what, e_s, o_s, float(np.abs(s64).max()), e_l, o_l, float(gerr.max()), o_g, gmax))
    assert e_s <= max(1e-5, 4.0 * o_s)
    assert e_l <= max(1e-5 * max(1.0, abs(l64)), 4.0 * o_l)
    assert (gerr <= np.maximum(gbar, 4.0 * o_g)).all(), float((gerr - np.maximum(gbar, 4.0 * o_g)).max())


# ---- 1. gradients at the kernels' edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=_id)
def test_streaming_step_against_float64(shape, knob):
    from ultra_pytorch_amd import hip_ops
    B, L, F, dm, H, nl, dff = shape
    p0, feats, ids, y, ipw, r32, r64 = case(shape)
    sh = streaming(F, dm, H, nl, dff)
    family = "long_mfma" if dm // H in (16, 32, 64) else "long_scalar"
    assert hip_ops.setrank_attn_path(sh, L) == family and hip_ops.setrank_attn_path(sh, L, backward=True) == family
    scores, grads, loss, _, _ = run(sh, B, L, p0, feats, ids, y, ipw)
    assert np.isfinite(grads).all()
    hold_to_float64(_id(shape), (scores, grads, loss), r32, r64)


# ---- 2. peaked attention -------------------------------------------------------------------------------------------------------------------
def test_peaked_attention_against_float64(knob):
    """input_embedding.2.weight and every layernorm2.weight times 8 (tests/sr_attn_long_ref.peaked): logits of tens of units, rows with
    one dominant partner - P near 1 and near 0 in the same tile, dS a difference of like-sized terms."""
    B, L, F, dm, H, nl, dff = PEAKED_SHAPE
    p0, feats, ids, y, ipw, r32, r64 = case(PEAKED_SHAPE, 8.0)
    assert float(np.abs(r64["scores"]).max()) > 2.0  # (the gain did spread the probabilities)
    scores, grads, loss, _, _ = run(streaming(F, dm, H, nl, dff), B, L, p0, feats, ids, y, ipw)
    hold_to_float64(_id(PEAKED_SHAPE) + " peaked x 8", (scores, grads, loss), r32, r64)


# ---- 3. the same family at two lengths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", SHORT_MODELS, ids=lambda m: "dh%d" % (m[1] // m[2]))
@pytest.mark.parametrize("L", [37, 100, 120])
def test_streaming_backward_below_the_hand_over_point(L, model, knob):
    """With ULTR_SR_ATTN_LONG_MIN=17 a streaming model runs the streaming kernels in both directions at lists the one-pass kernels take:
    a ragged single tile (37), a ragged own block in a ragged tile (100), whole blocks (120, 112 + 8) - against the oracle at
    tests/test_gpu_setrank.py's tolerances."""
    from ultra_pytorch_amd import hip_ops
    shape = (3, L) + tuple(model)
    p0, feats, ids, y, ipw, r, _ = case(shape)
    sh = streaming(*model)
    assert not hip_ops.setrank_attn_path(sh, L, backward=True).startswith("long")  # the default does not use them here
    knob(17)
    assert hip_ops.setrank_attn_path(sh, L, backward=True).startswith("long") and hip_ops.setrank_attn_path(sh, L).startswith("long")
    scores, grads, loss, _, _ = run(sh, 3, L, p0, feats, ids, y, ipw)
    print("L %d %r: scores %.3g, grads %.3g of max %.3g" % (L, model, float(np.abs(scores - r["scores"]).max()),
                                                          float(np.abs(grads - r["grads"]).max()), float(np.abs(r["grads"]).max())))
    np.testing.assert_allclose(scores, r["scores"], atol=1e-5)
    assert abs(loss - r["loss"]) <= 1e-5 * max(1.0, abs(r["loss"]))
    np.testing.assert_allclose(grads, r["grads"], rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(r["grads"]).max())))


# ---- 4. bits ---------------------------------------------------------------------------------------------------------------------------------
def test_short_lists_keep_the_bits_of_a_model_without_the_flag(knob):
    from ultra_pytorch_amd import hip_ops
    shape = (3, 100, 24, 64, 2, 1, 16)
    B, L, F, dm, H, nl, dff = shape
    p0, feats, ids, y, ipw, _, _ = case(shape)
    plain, flagged = hip_ops.SetRankShape(F, dm, H, nl, dff), streaming(F, dm, H, nl, dff)
    assert hip_ops.setrank_attn_path(flagged, L, backward=True) == hip_ops.setrank_attn_path(plain, L, backward=True) == "split_half"
    a = run(plain, B, L, p0, feats, ids, y, ipw)
    b = run(flagged, B, L, p0, feats, ids, y, ipw)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


def test_two_streaming_steps_give_the_same_bits(knob):
    B, L, F, dm, H, nl, dff = PEAKED_SHAPE
    p0, feats, ids, y, ipw, _, _ = case(PEAKED_SHAPE)
    a = run(streaming(F, dm, H, nl, dff), B, L, p0, feats, ids, y, ipw)
    b = run(streaming(F, dm, H, nl, dff), B, L, p0, feats, ids, y, ipw)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


# ---- 5. workspace contract -------------------------------------------------------------------------------------------------------------------
def test_streaming_steps_stay_inside_their_workspaces(knob):
    """Two steps at (2, 300, 24, 64, 4, 1, 16) with the engine's buffers on the guarded arena: `sr_ws` is what
    ultr_setrank_workspace_bytes answers for the flagged descriptor, t [T, H] at its end - bands intact, every bit of the plain run."""
    from tests import test_gpu_workspace_bounds as W
    from ultra_pytorch_amd import engine
    B, L, F, dm, H, nl, dff = PEAKED_SHAPE
    p0, feats, ids, y, ipw, _, _ = case(PEAKED_SHAPE)
    runs = []
    for guarded in (False, True):
        eng = engine.SetRankStepEngine(streaming(F, dm, H, nl, dff), B, L, torch.device("cuda"), algo="softmax", **KW)
        arena = None
        if guarded:
            arena = W.arena_for(eng)
            W.guard_engine(eng, arena)
        p, st = dev(p0.copy()), dev(np.zeros_like(p0))
        f, i, yy, tab = dev(feats.copy()), dev(ids.copy(), torch.int32), dev(y.copy(), torch.float32), dev(ipw.copy())
        outs = []
        for _ in range(2):
            eng.train_step(p, st, f, feats.shape[0], i, yy, ipw_table=tab)
            torch.cuda.synchronize()
            if arena is not None:
                arena.check()
                assert arena.untouched(eng.scores) == 0
            outs.append(W.snapshot(eng, p, st, None))
        eng.close()
        runs.append(outs)
    for k, (a, b) in enumerate(zip(*runs)):
        W.hold_equal(a, b, "streaming SetRank step %d" % (k + 1))


# ---- 6. plug-in ------------------------------------------------------------------------------------------------------------------------------
SR_HP = "d_model=32,num_heads=2,num_layers=1,diff=16,attention_backward=streaming"


def _algo(name, F, L):
    from tests.test_gpu_plugins import DataSet
    from ultra_pytorch_amd.utils import find_class
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm." + name, "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.SetRank.SetRank", "ranking_model_hparams": SR_HP,
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3, 5, 10]}
    return find_class(exp["learning_algorithm"])(DataSet(F), exp)


@pytest.mark.parametrize("name", ["NavieAlgorithm", "DLA", "PRSrank"])
def test_learning_algorithms_construct_with_a_streaming_setrank_at_300(name):
    from ultra_pytorch_amd import _lib
    a = _algo(name, 24, 300)
    assert a.rank_list_size == 300 and int(a.model.shape.desc.flags) & _lib.MODEL_SR_STREAM_BWD


def adagrad_bound(g, state, bar, lr, eps=1e-10):
    """How far Adagrad's step p - lr g / (sqrt(state + g^2) + eps) can move when g moves by at most `bar` (float64, per element): the
    quotient is monotone in g, so the extremes sit at g - bar and g + bar."""
    g, state, bar = (np.asarray(a, np.float64) for a in (g, state, bar))

    def f(v):
        return v / (np.sqrt(state + v * v) + eps)

    return lr * np.maximum(np.abs(f(g + bar) - f(g)), np.abs(f(g - bar) - f(g)))


def test_ipwrank_trains_a_streaming_setrank_at_300(knob):
    """train() twice in a row at rank_list_size 300, batch 3.  Each call is held to the oracle's step from the state the call started
    from (parameters and Adagrad sums as the previous call left them): the loss at the loss bar, the parameters at the gradient bar
    (rtol 1e-5, atol 2e-6 max(1, max|g|)) carried through the update - adagrad_bound, plus 2e-7 |p| + 4e-8 for the float32 rounding of
    the update itself on both sides (the result's own rounding, 2^-24 |p| each; five roundings on the way to a quotient of magnitude
    <= 1 times lr = 0.05, 1.5e-8 each).  Adagrad's first step from a zero sum is lr sign(g): an element whose gradient is inside the
    gradient bar may land anywhere in p -+ lr and the bound says so, every other element is held to the rounding; the second step
    divides by sqrt(g1^2 + g2^2) and moves by lr bar g1^2 / (g1^2 + g2^2)^1.5.  So that the bound cannot go slack unnoticed the test
    requires it below 1e-6 for nine tenths of the elements in the first step and below 1e-4 in the second (the oracle's own two steps
    from a seeded initialisation: 98 % and 95 %).  No clipping: the oracle's gradient norm is below max_gradient_norm."""
    from oracle import ultr_oracle as O
    from tests.test_gpu_plugins import load_flat, make_feed
    from ultra_pytorch_amd import synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    F, L, B, lr = 24, 300, 3, 0.05
    algo = _algo("IPWrank", F, L)
    load_flat(algo.model, init_setrank_params(algo.model.shape, seed=3).numpy())  # (the figures above are this initialisation's)
    cfg = (F, 32, 2, 1, 16)
    for k in range(2):
        p = algo.model.flat_params.detach().cpu().numpy().copy()
        s = algo.state_sum.detach().cpu().numpy().copy()
        feats, ids, y = synthetic.make_batch(np.random.RandomState(20 + k), B, L, F, n_pad=2)
        loss, out, _ = algo.train(make_feed(algo, feats, ids, y))
        r = O.train_step_setrank_softmax(p, s, cfg, feats, ids, y, ipw_list=algo.IPW_list, lr=lr, max_norm=5.0)
        assert out is None and np.isfinite(loss) and abs(loss - r["loss"]) <= 1e-5 * max(1.0, abs(r["loss"])), (k, loss, r["loss"])
        assert r["norm"] < 5.0
        g = r["grads"].astype(np.float64)
        bar = 1e-5 * np.abs(g) + 2e-6 * max(1.0, float(np.abs(g).max()))
        tol = adagrad_bound(g, s, bar, lr) + 2e-7 * np.abs(r["params"]) + 4e-8
        err = np.abs(algo.model.flat_params.detach().cpu().numpy().astype(np.float64) - r["params"])
        moved = float(np.abs(r["params"] - p).max())
        print("step %d: loss %.6f (oracle %.6f), parameters moved by up to %.3g, largest distance to the oracle %.3g, median bound %.3g, "
              "elements bounded below 1e-6 / 1e-4: %d / %d of %d" % (k + 1, loss, r["loss"], moved, float(err.max()), float(np.median(tol)),
                                                                     int((tol < 1e-6).sum()), int((tol < 1e-4).sum()), tol.size))
        assert moved > 1e-3 and (err <= tol).all(), float((err - tol).max())
        assert (tol < (1e-6, 1e-4)[k]).sum() >= 0.9 * tol.size


# ---- 7. dropout ------------------------------------------------------------------------------------------------------------------------------
def test_dropout_step_at_300(knob):
    """One rate-0.1 step at 300 documents, twice from the same state and key: finite, the same bits, and the float64 restatement with the
    replayed masks (tests/setrank_dropout_ref.py) at tests/test_gpu_setrank_dropout.py's tolerances."""
    from tests import setrank_dropout_ref as D
    from tests.test_gpu_setrank_dropout import run_step
    B, L, F, dm, H, nl, dff = PEAKED_SHAPE
    p0, feats, ids, y, ipw, _, _ = case(PEAKED_SHAPE)
    seed, step = 0x1234_5678_9ABC_DEF0, 3
    outs = []
    for _ in range(2):
        sh = streaming(F, dm, H, nl, dff, rate=0.1)
        outs.append(run_step(sh, B, L, p0, np.zeros_like(p0), feats.copy(), ids.copy(), y.copy(), ipw.copy(), seed=seed, step=step))
    (scores, g, params, _, sc), again = outs
    assert np.isfinite(scores).all() and np.isfinite(g).all() and np.isfinite(params).all()
    assert np.array_equal(scores, again[0]) and np.array_equal(g, again[1]) and np.array_equal(params, again[2])
    r = D.train_step(p0.copy(), np.zeros_like(p0), (F, dm, H, nl, dff), feats, ids, y, ipw_list=ipw, rate=0.1, seed=seed, step=step)
    gref = r["grads"]
    grads = g[: sh.n_params] / float(sc[3])
    print("dropout 0.1 at L 300: scores %.3g, loss %.3g, grads %.3g (of max %.3g)" % (
        float(np.abs(scores - r["scores"]).max()), abs(float(sc[0]) - r["loss"]), float(np.abs(grads - gref).max()), float(np.abs(gref).max())))
    np.testing.assert_allclose(scores, r["scores"], atol=1e-5)
    assert abs(float(sc[0]) - r["loss"]) <= 1e-5 * max(1.0, abs(r["loss"]))
    np.testing.assert_allclose(grads, gref, rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(gref).max())))
