"""SetRank beyond 256 documents on the GPU (csrc/ultr_sr_attn_long.hip): the streaming attention forward against
oracle.setrank_forward at the project's score bar (1e-5), with peaked attention against a float64 run, the same kernels below the
hand-over point (ULTR_SR_ATTN_LONG_MIN), run-to-run determinism, the plug-in's validation() / validation_set() at
max_candidate_num 300 and 900, the workspace contract on the guarded arena, and the backward's refusal."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sr_attn_long_ref as R  # noqa: E402
from tests.hipref import dev  # noqa: E402

# (B, L, F, d, H, layers, dff)
LONG_SHAPES = [(2, 257, 20, 48, 6, 1, 20),      # one key past a tile, head depth 8: the long scalar kernel
               (2, 300, 24, 64, 4, 1, 16),      # head depth 16
               (3, 385, 24, 64, 2, 1, 16),      # head depth 32, 3 tiles + 1
               (2, 272, 24, 64, 1, 2, 16),      # head depth 64, two layers
               (2, 1251, 136, 256, 8, 2, 64),   # the MSLR length at full width
               (1, 4100, 24, 64, 4, 1, 16)]
MSLR = LONG_SHAPES[4]
PEAKED_SHAPES = [(2, 300, 24, 64, 4, 1, 16), (2, 385, 24, 64, 1, 2, 16)]
# (shape, gain): the issue's two cases at gain 8, and 33 key tiles with moderately peaked attention (gain 4: scores reach 2.6, the fp32
# oracle stays 1.1e-6 from float64 - at a larger gain it is itself 1e-5 away at such lengths)
PEAKED_CASES = [(PEAKED_SHAPES[0], 8.0), (PEAKED_SHAPES[1], 8.0), ((1, 4100, 24, 64, 2, 1, 16), 4.0)]
SR_MODEL = "ultra_pytorch_amd.ranking_model.SetRank.SetRank"
SR_HP = "d_model=32,num_heads=2,num_layers=1,diff=16"


def _id(s):
    return "B%d_L%d_F%d_d%d_H%d_nl%d_dff%d" % tuple(s)


@functools.lru_cache(maxsize=None)
def case(shape, gain=None):
    """Inputs and the oracle's scores of one shape, computed once: (SetRankShape, params, feats, ids, oracle scores [B, L])."""
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    B, L, F, dm, H, nl, dff = shape
    sh = hip_ops.SetRankShape(F, dm, H, nl, dff)
    feats, ids, _ = synthetic.make_batch(np.random.RandomState(11), B, L, F, clicks=False, n_pad=2)
    p0 = init_setrank_params(sh, seed=9).numpy()
    if gain is not None:
        p0 = R.peaked(p0, sh, gain)
    ref = O.setrank_forward(torch.from_numpy(p0), F, dm, H, nl, dff, feats, ids).numpy()
    for a in (p0, feats, ids, ref):
        a.setflags(write=False)
    return sh, p0, feats, ids, ref


def gpu_scores(sh, p0, feats, ids, attention_dtype=None):
    from ultra_pytorch_amd import engine, hip_ops
    if attention_dtype is not None:
        sh = hip_ops.SetRankShape(sh.feature_size, sh.d_model, sh.num_heads, sh.num_layers, sh.dff, attention_dtype=attention_dtype)
    L, B = ids.shape
    eng = engine.SetRankEvalEngine(sh, B, L, torch.device("cuda"))
    out = eng.forward(dev(p0.copy()), dev(feats.copy()), feats.shape[0], dev(ids.copy(), torch.int32))
    torch.cuda.synchronize()
    return out.clone()


@pytest.fixture
def knob(monkeypatch):
    """Set ULTR_SR_ATTN_LONG_MIN and have the library read it; the default is back when the test ends."""
    from ultra_pytorch_amd import _lib
    lib = _lib.load()

    def set_(value):
        if value is None:
            monkeypatch.delenv("ULTR_SR_ATTN_LONG_MIN", raising=False)
        else:
            monkeypatch.setenv("ULTR_SR_ATTN_LONG_MIN", str(value))
        lib.ultr_config_reload()

    set_(None)
    yield set_
    monkeypatch.undo()
    lib.ultr_config_reload()


# ---- 1. scores against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=_id)
def test_long_lists_against_the_oracle(shape, knob):
    from ultra_pytorch_amd import hip_ops
    sh, p0, feats, ids, ref = case(shape)
    assert hip_ops.setrank_attn_path(sh, shape[1]) == ("long_mfma" if sh.d_model // sh.num_heads in (16, 32, 64) else "long_scalar")
    got = gpu_scores(sh, p0, feats, ids).cpu().numpy()
    print("%s: largest distance to the oracle %.3g" % (_id(shape), float(np.abs(got - ref).max())))
    np.testing.assert_allclose(got, ref, atol=1e-5, rtol=0)


def test_fp16_request_runs_the_fp32_streaming_kernel(knob):
    """attention_dtype=fp16 keeps its meaning: fp16 operands where those kernels exist (L <= 128), the fp32 path elsewhere - beyond 256
    documents the streaming kernel, with the bits of the fp32 request."""
    from ultra_pytorch_amd import hip_ops
    shape = LONG_SHAPES[2]
    sh, p0, feats, ids, ref = case(shape)
    sh16 = hip_ops.SetRankShape(sh.feature_size, sh.d_model, sh.num_heads, sh.num_layers, sh.dff, attention_dtype="fp16")
    assert hip_ops.setrank_attn_path(sh16, shape[1]) == "long_mfma"
    assert torch.equal(gpu_scores(sh, p0, feats, ids, "fp16"), gpu_scores(sh, p0, feats, ids))


# ---- 2. peaked attention ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,gain", PEAKED_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else "gain%g" % v)
def test_peaked_attention_against_float64(shape, gain, knob):
    """input_embedding.2.weight and every layernorm2.weight times the gain.  At 8: layer-0 logits span about -24 .. 72, the mean largest probability
    of a row is 0.53 / 0.71, scores reach 4.5 / 5.3 - the running maximum moves.  Reference: the float64 forward of
    tests/sr_attn_long_ref.py.  Bound: the larger of the project's relative score bar 1e-5 max(1, max|score|) and 4 x the fp32 oracle's
    own distance to float64 on the same inputs (3.1e-6 and 4.4e-6 when the issue was written), computed here.  The third case walks
    33 key tiles with logits of several units: an error that grew with the tile count would show there (the float32 restatement in
    tests/test_sr_attn_long_cpu.py pins that property tile by tile).
    Measured on an MI355X: see profiles/setrank_long.md."""
    B, L, F, dm, H, nl, dff = shape
    sh, p0, feats, ids, ref32 = case(shape, gain)
    ref64 = R.setrank_forward(p0, F, dm, H, nl, dff, feats, ids)
    oracle_err = float(np.abs(ref32 - ref64).max())
    bound = max(1e-5 * max(1.0, float(np.abs(ref64).max())), 4.0 * oracle_err)
    got = gpu_scores(sh, p0, feats, ids).cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref64).max())
    print("%s peaked x %g: max|score| %.3g, oracle to float64 %.3g, kernel to float64 %.3g, bound %.3g"
          % (_id(shape), gain, float(np.abs(ref64).max()), oracle_err, err, bound))
    assert float(np.abs(ref64).max()) > 2.0  # (the gain did spread the scores)
    assert err <= bound


# ---- 3. the same family at two lengths ---------------------------------------------------------------------------------------------------
SHORT_MODELS = [(20, 48, 6, 1, 20), (24, 64, 4, 1, 16), (24, 64, 2, 1, 16), (24, 64, 1, 2, 16)]  # head depth 8 / 16 / 32 / 64


@pytest.mark.parametrize("model", SHORT_MODELS, ids=lambda m: "dh%d" % (m[1] // m[2]))
@pytest.mark.parametrize("L", [37, 100, 120])
def test_long_kernels_below_the_hand_over_point(L, model, knob):
    from ultra_pytorch_amd import hip_ops
    sh, p0, feats, ids, ref = case((3, L) + model)
    assert not hip_ops.setrank_attn_path(sh, L).startswith("long")  # the default does not use them here
    knob(17)
    assert hip_ops.setrank_attn_path(sh, L).startswith("long")
    got = gpu_scores(sh, p0, feats, ids).cpu().numpy()
    print("L %d %r: largest distance to the oracle %.3g" % (L, model, float(np.abs(got - ref).max())))
    np.testing.assert_allclose(got, ref, atol=1e-5, rtol=0)


@pytest.mark.parametrize("B,L,F,dm,H,nl,dff", [(4, 100, 24, 64, 2, 1, 16), (3, 37, 20, 48, 6, 1, 20), (4, 120, 24, 64, 1, 2, 16)],
                         ids=["dh32_split_half_backward", "dh8_scalar_backward", "dh64_two_layers"])
def test_streaming_forward_feeds_the_one_pass_backward(B, L, F, dm, H, nl, dff, knob):
    """A and lse have one layout whichever kernel wrote them: with the hand-over point lowered a training step runs the streaming forward
    and the one-pass backward (which reads lse on the matrix cores; the scalar backward recomputes its rows).  Scores, loss and
    gradients against the oracle at test_setrank_oracle's tolerances."""
    from oracle import ultr_oracle as O
    from tests.test_gpu_setrank import run_step
    from ultra_pytorch_amd import hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    shape = hip_ops.SetRankShape(F, dm, H, nl, dff)
    feats, ids, y = synthetic.make_batch(np.random.RandomState(11), B, L, F, n_pad=2)
    ipw = np.asarray(synthetic.load_ipw(), np.float32)
    p0 = init_setrank_params(shape, seed=9).numpy()
    knob(17)
    assert hip_ops.setrank_attn_path(shape, L).startswith("long") and not hip_ops.setrank_attn_path(shape, L, backward=True).startswith("long")
    scores, g, _, _, sc = run_step(shape, B, L, dict(learning_rate=0.05, max_gradient_norm=5.0), p0, np.zeros_like(p0), feats, ids, y, ipw)
    r = O.train_step_setrank_softmax(p0, np.zeros_like(p0), (F, dm, H, nl, dff), feats, ids, y, ipw_list=ipw, lr=0.05, max_norm=5.0)
    np.testing.assert_allclose(scores, r["scores"], atol=1e-5)
    assert abs(float(sc[0]) - r["loss"]) <= 1e-5 * max(1.0, abs(r["loss"]))
    np.testing.assert_allclose(g[: shape.n_params] / float(sc[3]), r["grads"], rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(r["grads"]).max())))


@pytest.mark.parametrize("L", [100, 200])
def test_short_lists_keep_their_bits_across_a_knob_round_trip(L, knob):
    from ultra_pytorch_amd import hip_ops
    sh, p0, feats, ids, _ = case((3, L, 24, 64, 2, 1, 16))
    before = gpu_scores(sh, p0, feats, ids)
    path = hip_ops.setrank_attn_path(sh, L)
    assert path == ("mfma" if L <= 128 else "scalar")
    knob(300)
    assert hip_ops.setrank_attn_path(sh, L) == path
    during = gpu_scores(sh, p0, feats, ids)
    knob(None)
    after = gpu_scores(sh, p0, feats, ids)
    assert torch.equal(before, during) and torch.equal(before, after)


# ---- 4. determinism --------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(knob):
    sh, p0, feats, ids, _ = case(MSLR)
    assert torch.equal(gpu_scores(sh, p0, feats, ids), gpu_scores(sh, p0, feats, ids))


# ---- 5. plug-in level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,B", [(300, 6), (900, 3)], ids=["L300", "L900_beyond_the_short_metric_kernel"])
def test_plugin_validation_at_long_lists(L, B, knob, monkeypatch):
    from oracle import ultr_oracle as O
    from tests import test_gpu_metrics_all as M
    from ultra_pytorch_amd import engine
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    F, names, topn = 24, ["ndcg", "mrr", "err"], [1, 3, 5, 10]
    assert engine.metrics_fit(L) and (L <= 813) == engine.metrics_fit_short(L)
    feats, ids, y = M._batch(B, L, F)
    algo = M._algo(F, L, names, model=SR_MODEL, model_hparams=SR_HP)
    _, scores, summary = algo.validation(M._feeds(algo, feats, ids, y, False))
    summary = dict(summary)
    assert tuple(scores.shape) == (B, L) and sorted(summary) == sorted("%s_%d" % (m, n) for m in names for n in topn)
    ref = O.setrank_forward(algo.model.flat_params.detach().cpu(), F, 32, 2, 1, 16, feats, ids).numpy()
    np.testing.assert_allclose(scores.cpu().numpy(), ref, atol=1e-5, rtol=0)
    for key, v in M._host_metrics(algo, y, names, topn).items():
        assert abs(summary[key] - v) <= 1e-6, (key, summary[key], v)


def test_resident_set_at_300_documents_is_the_per_batch_loop(knob, monkeypatch):
    from tests import test_gpu_eval_set as E
    from ultra_pytorch_amd import input_layer
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    L, B, F = 300, 8, 24
    ds = E.DS(37, L, F, seed=6)
    algo = E._algo(F, L, ["ndcg", "mrr", "err"], "SetRank.SetRank", SR_HP)
    dfeed = input_layer.DeviceDirectLabelFeed(algo, B, "")
    want, want_scores, _, sizes = E.per_batch_loop(algo, dfeed, ds)
    assert sizes == [8, 8, 8, 8, 5]
    summary, scores, _ = algo.validation_set(dfeed, ds, want_scores=True)
    assert set(want) == set(summary)
    for k in summary:
        assert summary[k] == want[k], (k, summary[k], want[k])
    assert tuple(scores.shape) == (37, L) and torch.equal(scores, want_scores)


# ---- 6. workspace contract -------------------------------------------------------------------------------------------------------------
def test_long_forward_stays_inside_its_workspaces(knob):
    """One forward at (2, 300, 24, 64, 4, 1, 16) with the engine's buffers on the guarded arena: bands intact, scores bit for bit those
    of the plain run - no write past `saved` or the scores, no poisoned word consumed."""
    from tests import test_gpu_workspace_bounds as W
    from ultra_pytorch_amd import engine
    shape = LONG_SHAPES[1]
    sh, p0, feats, ids, _ = case(shape)
    outs = []
    for guarded in (False, True):
        eng = engine.SetRankStepEngine(sh, shape[0], shape[1], torch.device("cuda"), algo="softmax")
        arena = None
        if guarded:
            arena = W.arena_for(eng)
            W.guard_engine(eng, arena)
        eng.forward(dev(p0.copy()), dev(feats.copy()), feats.shape[0], dev(ids.copy(), torch.int32))
        torch.cuda.synchronize()
        if arena is not None:
            arena.check()
            assert arena.untouched(eng.scores) == 0
        outs.append(W.bits(eng.scores))
        eng.close()
    assert np.array_equal(outs[0], outs[1])


# ---- 7. training is still refused --------------------------------------------------------------------------------------------------------
def test_training_beyond_the_one_pass_kernels_is_refused(knob):
    """There is no streaming attention backward: at 300 documents the forward and the loss run, the backward raises."""
    from ultra_pytorch_amd import _lib, engine, hip_ops
    shape = LONG_SHAPES[1]
    sh, p0, feats, ids, ref = case(shape)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.setrank_attn_path(sh, shape[1], backward=True)
    eng = engine.SetRankStepEngine(sh, shape[0], shape[1], torch.device("cuda"), algo="softmax")
    p, f, i = dev(p0.copy()), dev(feats.copy()), dev(ids.copy(), torch.int32)
    eng.forward(p, f, feats.shape[0], i, train=True)
    eng.loss(torch.ones(shape[1], shape[0], device="cuda"))
    torch.cuda.synchronize()
    np.testing.assert_allclose(eng.scores.cpu().numpy(), ref, atol=1e-5, rtol=0)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        eng.backward(p, f, feats.shape[0], i)
    torch.cuda.synchronize()
    eng.close()
