"""ultr_setrank_score on the GPU: the evaluation forward that keeps no record for a backward (csrc/ultr_sr_plan.h:
sr_make_score_plan).  Its scores are the training forward's bit for bit on every route and attention family; its buffer is
ultr_setrank_score_bytes long and no longer (guarded arena), never read before written (poisoned against zeroed), independent of
num_layers; the range word is raised as in the training forward and SetRankEvalEngine acts on it; refusals mirror the forward's."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import guarded  # noqa: E402
from tests.hipref import dev  # noqa: E402

KNOBS = ("ULTR_SR_BLOCK", "ULTR_SR_H3", "ULTR_SR_SCALAR_ATTN", "ULTR_SR_ATTN_LONG_MIN")
CFG5 = (136, 256, 8, 2, 64)   # F, d_model, heads, layers, dff: the persistent launches take these widths
ROUND5 = (12, 64, 4, 1, 32)
ODD = (13, 24, 3, 2, 10)      # nothing aligned: the plain kernels throughout


@pytest.fixture
def knob(monkeypatch):
    """Set SetRank knobs and have the library read them; the defaults are back when the test ends."""
    from ultra_pytorch_amd import _lib
    lib = _lib.load()

    def set_(**kw):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            assert k in KNOBS
            monkeypatch.setenv(k, str(v))
        lib.ultr_config_reload()

    set_()
    yield set_
    monkeypatch.undo()
    lib.ultr_config_reload()


def make_shape(model, **kw):
    from ultra_pytorch_amd import hip_ops
    F, d, H, nl, dff = model
    return hip_ops.SetRankShape(F, d_model=d, num_heads=H, num_layers=nl, dff=dff, **kw)


@functools.lru_cache(maxsize=None)
def inputs(model, B, L, seed=9):
    """(params, features, docids) of one case as read-only numpy, computed once."""
    from ultra_pytorch_amd import synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    feats, ids, _ = synthetic.make_batch(np.random.RandomState(11), B, L, model[0], clicks=False, n_pad=2 if L > 4 else 0)
    p0 = init_setrank_params(make_shape(model), seed=seed).numpy()
    for a in (p0, feats, ids):
        a.setflags(write=False)
    return p0, feats, ids


def poisoned(n_bytes, offset_floats=0, fill=float("nan")):
    """n_bytes of NaN (or `fill`) starting offset_floats * 4 bytes past a 512-byte boundary."""
    n = n_bytes // 4
    return torch.full((n + offset_floats,), fill, dtype=torch.float32, device="cuda")[offset_floats:]


def run_both(sh, model, B, L, offset_floats=0):
    """(scores of ultr_setrank_score, scores of ultr_setrank_forward) on NaN-poisoned buffers."""
    from ultra_pytorch_amd import hip_ops
    p0, feats, ids = inputs(model, B, L)
    p, f, i = dev(p0.copy()), dev(feats.copy()), dev(ids.copy(), torch.int32)
    T = B * L
    out = []
    for score in (True, False):
        scores = torch.full((B, L), float("nan"), device="cuda")
        if score:
            work = poisoned(sh.score_bytes(T), offset_floats)
            assert work.numel() * 4 == sh.score_bytes(T) and work.data_ptr() % 16 == (4 * offset_floats) % 16
            hip_ops.setrank_score(sh, p, f, feats.shape[0], i, B, L, scores, work)
        else:
            saved = poisoned(sh.saved_bytes(T), offset_floats)
            hip_ops.setrank_forward(sh, p, f, feats.shape[0], i, B, L, scores, saved)
        torch.cuda.synchronize()
        out.append(scores)
    assert bool(torch.isfinite(out[1]).all())
    return out


# ---- 1. the bits of the training forward -------------------------------------------------------------------------------------------------
# (id, model, B, L, shape keywords, knobs, offset of the buffers in floats, the forward attention family expected or None)
CASES = [
    # T = 111: tiles of 4 rows, the last one of 3 (sr_bwd_geometry takes every T > 0: rows per tile = T / CUs rounded up to 4)
    ("persistent_ragged_tile", CFG5, 3, 37, {}, {}, 0, "mfma"),
    # T = 16500 > 64 rows x 256 workgroups: every workgroup walks two tiles, requesting the second while it works on the first
    ("persistent_two_tiles_per_workgroup", CFG5, 165, 100, {}, {}, 0, "mfma"),
    ("round5", ROUND5, 5, 23, {}, {}, 0, "mfma"),
    ("round5_at_persistent_widths", CFG5, 3, 37, {}, {"ULTR_SR_BLOCK": 2}, 0, "mfma"),
    ("separate_odd_widths", ODD, 5, 23, {}, {}, 0, "scalar"),
    ("separate_aligned_widths", CFG5, 3, 37, {}, {"ULTR_SR_BLOCK": 0}, 0, "mfma"),
    ("separate_aligned_d64", ROUND5, 5, 23, {}, {"ULTR_SR_BLOCK": 0}, 0, "mfma"),
    ("separate_buffers_off_by_4_bytes", CFG5, 3, 37, {}, {}, 1, "mfma"),
    ("fp32_products_knob", CFG5, 3, 37, {}, {"ULTR_SR_H3": 0}, 0, "mfma"),
    ("fp32_products_descriptor", CFG5, 3, 37, {"fp32_products": True}, {}, 0, "mfma"),
    ("fp16_attention_L100", CFG5, 2, 100, {"attention_dtype": "fp16"}, {}, 0, "f16"),
    ("scalar_attention_knob", ROUND5, 5, 23, {}, {"ULTR_SR_SCALAR_ATTN": 1}, 0, None),
    ("one_pass_scalar_L129", ROUND5, 2, 129, {}, {}, 0, "scalar"),
    ("streaming_L300_dh16", ROUND5, 2, 300, {}, {}, 0, "long_mfma"),
    ("streaming_L270_dh8", (12, 64, 8, 1, 32), 2, 270, {}, {}, 0, "long_scalar"),
    ("stream_backward_flag_L200", ROUND5, 2, 200, {"attention_backward": "streaming"}, {}, 0, "long_mfma"),
]


@pytest.mark.parametrize("name,model,B,L,kw,knobs,off,family", CASES, ids=[c[0] for c in CASES])
def test_same_bits_as_the_training_forward(name, model, B, L, kw, knobs, off, family, knob):
    from ultra_pytorch_amd import _lib, hip_ops
    kw = dict(kw)
    fp32 = kw.pop("fp32_products", False)
    sh = make_shape(model, **kw)
    if fp32:
        sh.desc.flags = int(sh.desc.flags) | _lib.MODEL_FP32_PRODUCTS
    knob(**knobs)
    if family is not None:
        assert hip_ops.setrank_attn_path(sh, L) == family
    got, want = run_both(sh, model, B, L, off)
    assert torch.equal(got, want), "largest difference %.3g" % float((got - want).abs().max())


# ---- 2. the buffer contract --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,B,L", [(CFG5, 3, 37), (ODD, 5, 23)], ids=["persistent", "odd"])
def test_buffer_contract(model, B, L, knob):
    """`work` of exactly score_bytes on the guarded arena, two calls in a row: bands intact, the bits of a zeroed buffer (nothing is read
    before it is written, nothing survives from the first call into the second); one byte less: refused before any launch."""
    from ultra_pytorch_amd import _lib, hip_ops
    sh = make_shape(model)
    p0, feats, ids = inputs(model, B, L)
    p, f, i = dev(p0.copy()), dev(feats.copy()), dev(ids.copy(), torch.int32)
    n = sh.score_bytes(B * L)
    arena = guarded.Arena("cuda", guarded.bytes_for([n, n, 4 * B * L, 4 * B * L]))
    outs = []
    for zero in (False, True):
        work = arena.view(n // 4, zero=zero, name="work_zeroed" if zero else "work_poisoned")
        scores = arena.view(B * L, name="scores%d" % zero).view(B, L)
        for _ in range(2):
            hip_ops.setrank_score(sh, p, f, feats.shape[0], i, B, L, scores, work)
        torch.cuda.synchronize()
        outs.append(scores.clone())
    arena.check()
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
    # one byte less than the library asks for (the binding passes the tensor's byte length: call the C entry itself)
    scores = torch.full((B, L), float("nan"), device="cuda")
    work = poisoned(n)
    import ctypes
    args = [ctypes.byref(sh.desc), p.data_ptr(), f.data_ptr(), feats.shape[0], i.data_ptr(), B, L, scores.data_ptr(), work.data_ptr()]
    assert sh.lib.ultr_setrank_score(*args, n - 1, hip_ops.raw_stream()) == -3  # ULTR_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(scores).all()) and bool(torch.isnan(work).all())  # nothing was launched
    with pytest.raises(_lib.UltrHipError, match="workspace too small"):
        hip_ops.setrank_score(sh, p, f, feats.shape[0], i, B, L, scores, work[:-1])
    assert sh.lib.ultr_setrank_score(*args, n, hip_ops.raw_stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(scores, outs[0])


# ---- 3. layers reuse the buffers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [3, 0], ids=["fused", "separate"])
def test_four_layers_share_the_buffers(block, knob):
    from oracle import ultr_oracle as O
    model, B, L = (12, 64, 4, 4, 32), 5, 23
    sh = make_shape(model)
    assert sh.score_bytes(B * L) - sh.score_bytes(0) == make_shape(model[:3] + (1,) + model[4:]).score_bytes(B * L) - \
        make_shape(model[:3] + (1,) + model[4:]).score_bytes(0)
    knob(ULTR_SR_BLOCK=block)
    got, want = run_both(sh, model, B, L)
    assert torch.equal(got, want)
    p0, feats, ids = inputs(model, B, L)
    ref = O.setrank_forward(torch.from_numpy(p0.copy()), *model, feats, ids).numpy()
    print("four layers: largest distance to the oracle %.3g" % float(np.abs(got.cpu().numpy() - ref).max()))
    np.testing.assert_allclose(got.cpu().numpy(), ref, atol=1e-5, rtol=0)


# ---- 4. the range word -------------------------------------------------------------------------------------------------------------------
def test_range_word_and_the_engines_fallback(knob):
    from ultra_pytorch_amd import _lib, engine, hip_ops
    model, B, L = ROUND5, 5, 23
    sh = make_shape(model)
    p0, feats, ids = inputs(model, B, L)
    p1 = p0.copy()
    off = {n: o for n, _, o in sh.layout()}
    name = [n for n in off if n.endswith("mha.dense.weight")][0]
    p1[off[name] + 3] = 70.0  # |w| >= 64: near the end of the planes' range
    p, f, i = dev(p1), dev(feats.copy()), dev(ids.copy(), torch.int32)
    T = B * L
    for params, raised in ((dev(p0.copy()), False), (p, True)):
        work = poisoned(sh.score_bytes(T))
        scores = torch.empty(B, L, device="cuda")
        hip_ops.setrank_score(sh, params, f, feats.shape[0], i, B, L, scores, work)
        torch.cuda.synchronize()
        word = int(work[sh.score_range_flag_offset(T):][:1].view(torch.int32).item())
        saved = poisoned(sh.saved_bytes(T))
        hip_ops.setrank_forward(sh, params, f, feats.shape[0], i, B, L, scores, saved)
        torch.cuda.synchronize()
        assert word == int(saved[sh.range_flag_offset(T):][:1].view(torch.int32).item())  # as in the training forward
        assert (word != 0) == raised
    # the fp32-products forward of the same weights
    sh32 = make_shape(model)
    sh32.desc.flags = int(sh32.desc.flags) | _lib.MODEL_FP32_PRODUCTS
    want = torch.empty(B, L, device="cuda")
    hip_ops.setrank_forward(sh32, p, f, feats.shape[0], i, B, L, want, poisoned(sh32.saved_bytes(T)))
    eng = engine.SetRankEvalEngine(sh, B, L, torch.device("cuda"))
    labels = torch.zeros(L, B, device="cuda")
    assert hip_ops.split_half_enabled(sh)
    with pytest.warns(RuntimeWarning, match="fp32 matrix cores"):
        got, _ = eng.run(p, f, feats.shape[0], i, labels)
    torch.cuda.synchronize()
    assert int(sh.desc.flags) & _lib.MODEL_FP32_PRODUCTS and not hip_ops.split_half_enabled(sh)
    assert torch.equal(got, want)


# ---- 5. the engine -----------------------------------------------------------------------------------------------------------------------
def test_engine_holds_the_scoring_buffer_at_the_mslr_length(knob):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine
    model, B, L = (24, 64, 4, 2, 16), 2, 1251
    sh = make_shape(model)
    p0, feats, ids = inputs(model, B, L)
    eng = engine.SetRankEvalEngine(sh, B, L, torch.device("cuda"))
    assert eng.work.numel() * 4 == sh.score_bytes(B * L) < sh.saved_bytes(B * L)
    got = eng.forward(dev(p0.copy()), dev(feats.copy()), feats.shape[0], dev(ids.copy(), torch.int32))
    torch.cuda.synchronize()
    ref = O.setrank_forward(torch.from_numpy(p0.copy()), *model, feats, ids).numpy()
    print("B 2 x L 1251: largest distance to the oracle %.3g, %d bytes (saved: %d)"
          % (float(np.abs(got.cpu().numpy() - ref).max()), sh.score_bytes(B * L), sh.saved_bytes(B * L)))
    np.testing.assert_allclose(got.cpu().numpy(), ref, atol=1e-5, rtol=0)


def test_validation_set_over_three_chunks_is_the_per_batch_loop(knob, monkeypatch):
    from tests import test_gpu_eval_set as E
    from ultra_pytorch_amd import engine, input_layer
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0)
    L, B, F = 12, 8, 24
    ds = E.DS(20, L, F, seed=6)
    algo = E._algo(F, L, E.NAMES, "SetRank.SetRank", "d_model=32,num_heads=2,num_layers=2,diff=16")
    dfeed = input_layer.DeviceDirectLabelFeed(algo, B, "")
    want, want_scores, _, sizes = E.per_batch_loop(algo, dfeed, ds)
    assert sizes == [8, 8, 4]
    summary, scores, _ = algo.validation_set(dfeed, ds, want_scores=True)
    assert set(want) == set(summary)
    for k in summary:
        assert summary[k] == want[k], (k, summary[k], want[k])
    assert tuple(scores.shape) == (20, L) and torch.equal(scores, want_scores)
    evs = [e for e in algo._eval_engines.values() if isinstance(e, engine.SetRankEvalEngine)]
    assert evs and all(e.work.numel() * 4 == algo.model.shape.score_bytes(e.B * e.L) for e in evs)


# ---- 6. refusals mirror the forward's ----------------------------------------------------------------------------------------------------
def test_refusals_are_the_forwards(knob):
    import ctypes
    from ultra_pytorch_amd import _lib, hip_ops
    # head depth 424 at 300 documents: the streaming scalar kernel's rows do not fit in LDS
    model, B, L = (8, 424, 1, 1, 8), 1, 300
    sh = make_shape(model)
    p0, feats, ids = inputs(model, B, L)
    p, f, i = dev(p0.copy()), dev(feats.copy()), dev(ids.copy(), torch.int32)
    scores = torch.full((B, L), float("nan"), device="cuda")
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.setrank_forward(sh, p, f, feats.shape[0], i, B, L, scores, poisoned(sh.saved_bytes(B * L)))
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.setrank_score(sh, p, f, feats.shape[0], i, B, L, scores, poisoned(sh.score_bytes(B * L)))
    torch.cuda.synchronize()
    assert bool(torch.isnan(scores).all())
    # NULL work
    model, B, L = ODD, 5, 23
    sh = make_shape(model)
    p0, feats, ids = inputs(model, B, L)
    p, f, i = dev(p0.copy()), dev(feats.copy()), dev(ids.copy(), torch.int32)
    scores = torch.full((B, L), float("nan"), device="cuda")
    n = sh.score_bytes(B * L)
    rc = sh.lib.ultr_setrank_score(ctypes.byref(sh.desc), p.data_ptr(), f.data_ptr(), feats.shape[0], i.data_ptr(), B, L,
                                   scores.data_ptr(), None, n, hip_ops.raw_stream())
    assert rc == -1  # ULTR_E_BADARG
    rc = sh.lib.ultr_setrank_forward(ctypes.byref(sh.desc), p.data_ptr(), f.data_ptr(), feats.shape[0], i.data_ptr(), B, L,
                                     scores.data_ptr(), None, hip_ops.raw_stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(scores).all())
