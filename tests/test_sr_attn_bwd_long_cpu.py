"""SetRank training beyond the one-pass attention backward, the part that needs no GPU: the float64 reference of the streaming backward
(tests/sr_attn_bwd_ref.py) against the float64 forward of tests/sr_attn_long_ref.py, the fp32 oracle's step and direct autograd; the
dispatch table of a model with attention_backward=streaming (hip_ops.setrank_attn_path is host-only); the hparam; the workspace size."""
import numpy as np
import pytest

from tests import sr_attn_bwd_ref as RB
from tests import sr_attn_long_ref as R
from tests.test_sr_attn_long_cpu import DEFAULT_TABLE, _table

SMALL = (2, 37, 20, 48, 6, 1, 20)  # (B, L, F, d, H, layers, dff)


def _small_case():
    from ultra_pytorch_amd import hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    B, L, F, d, H, nl, dff = SMALL
    shape = hip_ops.SetRankShape(F, d, H, nl, dff)
    feats, ids, y = synthetic.make_batch(np.random.RandomState(11), B, L, F, n_pad=2)
    ipw = np.asarray(synthetic.load_ipw(), np.float32)
    return init_setrank_params(shape, seed=9).numpy(), feats, ids, y, ipw


def test_float64_forward_is_the_numpy_float64_forward():
    """Two float64 evaluations of the same forward (torch here, numpy there): 1e-12 is four orders above float64's rounding of sums of
    a few hundred terms at scores of order 1."""
    B, L, F, d, H, nl, dff = SMALL
    p0, feats, ids, _, _ = _small_case()
    got = RB.setrank_forward(p0, F, d, H, nl, dff, feats, ids).numpy()
    want = R.setrank_forward(p0, F, d, H, nl, dff, feats, ids)
    assert got.dtype == np.float64 and np.abs(got - want).max() < 1e-12


def test_float64_step_is_the_oracle_step():
    """Scores, loss and gradients of the float64 helper against the fp32 oracle at the tolerances the kernels are held to against that
    oracle (tests/test_gpu_setrank.py): the helper is a reference for them only if the oracle itself passes."""
    from oracle import ultr_oracle as O
    B, L, F, d, H, nl, dff = SMALL
    p0, feats, ids, y, ipw = _small_case()
    r = O.train_step_setrank_softmax(p0, np.zeros_like(p0), (F, d, H, nl, dff), feats, ids, y, ipw_list=ipw, lr=0.05, max_norm=5.0)
    g = RB.train_step(p0, (F, d, H, nl, dff), feats, ids, y, ipw_list=ipw)
    np.testing.assert_allclose(r["scores"], g["scores"], atol=1e-5, rtol=0)
    assert abs(r["loss"] - g["loss"]) <= 1e-5 * max(1.0, abs(g["loss"]))
    np.testing.assert_allclose(r["grads"], g["grads"], rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(g["grads"]).max())))


@pytest.mark.parametrize("dh", [8, 32])
@pytest.mark.parametrize("L", [130, 257, 385])
def test_tiled_two_role_walk_is_direct_autograd(L, dh):
    """Tiles of 128 partners, own blocks of 16: 130 leaves 2 tokens in the last tile and in the last own block (padding queries and
    padding keys in the same tile), 257 one token in a third tile, 385 one in a fourth.  Both sides are float64 evaluations of the same
    real function; 1e-12 relative to the largest entry is four orders above float64's rounding of sums of 385 terms."""
    rng = np.random.RandomState(100 * dh + L)
    x = rng.normal(size=(L, dh)) * 1.5  # logits of several units: rows with a few dominant partners
    dA = rng.normal(size=(L, dh))
    want = RB.attention_backward_autograd(x, dA)
    got = RB.attention_backward_tiled(x, dA, tile=128, own=16)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    other = RB.attention_backward_tiled(x, dA, tile=64, own=4)  # the scalar kernel's geometry
    np.testing.assert_allclose(other, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def _streaming_table():
    from ultra_pytorch_amd import hip_ops
    s32 = hip_ops.SetRankShape(24, 64, 2, 1, 16, attention_backward="streaming")
    s8 = hip_ops.SetRankShape(20, 48, 6, 1, 20, attention_backward="streaming")
    sh = hip_ops.SetRankShape(24, 64, 2, 1, 16, attention_dtype="fp16", attention_backward="streaming")
    path = hip_ops.setrank_attn_path
    rows = {("dh32 backward", L): path(s32, L, True) for L in (100, 128, 129, 257, 1251)}
    rows.update({("dh32", L): path(s32, L) for L in (128, 129)})
    rows.update({("dh8 backward", 120): path(s8, 120, True), ("dh8 backward", 121): path(s8, 121, True), ("dh8", 121): path(s8, 121)})
    rows.update({("dh32 fp16 backward", 100): path(sh, 100, True), ("dh32 fp16 backward", 300): path(sh, 300, True)})
    return rows


STREAMING_TABLE = {("dh32 backward", 100): "split_half", ("dh32 backward", 128): "split_half", ("dh32 backward", 129): "long_mfma",
                   ("dh32 backward", 257): "long_mfma", ("dh32 backward", 1251): "long_mfma",
                   ("dh32", 128): "mfma", ("dh32", 129): "long_mfma",
                   ("dh8 backward", 120): "scalar", ("dh8 backward", 121): "long_scalar", ("dh8", 121): "long_scalar",
                   ("dh32 fp16 backward", 100): "f16", ("dh32 fp16 backward", 300): "long_mfma"}


def test_streaming_dispatch_table(monkeypatch):
    """A model with attention_backward=streaming hands BOTH directions over where its one-pass backward refuses (beyond 128 documents
    on the matrix cores, 120 on the scalar kernel); below, today's families.  A model without the flag keeps today's table, refusals
    included.  ULTR_SR_ATTN_LONG_MIN lowers the hand-over of a streaming model's backward too, and of no other backward."""
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    for k in ("ULTR_SR_ATTN_LONG_MIN", "ULTR_SR_SCALAR_ATTN", "ULTR_SR_ATTN_H3", "ULTR_SR_ATTN_H3_MASK"):
        monkeypatch.delenv(k, raising=False)
    try:
        lib.ultr_config_reload()
        assert _streaming_table() == STREAMING_TABLE
        assert _table() == DEFAULT_TABLE
        monkeypatch.setenv("ULTR_SR_ATTN_LONG_MIN", "17")
        lib.ultr_config_reload()
        flagged = hip_ops.SetRankShape(24, 64, 2, 1, 16, attention_backward="streaming")
        plain = hip_ops.SetRankShape(24, 64, 2, 1, 16)
        assert hip_ops.setrank_attn_path(flagged, 100, True) == "long_mfma"
        assert hip_ops.setrank_attn_path(plain, 100, True) == "split_half"
        assert hip_ops.setrank_attn_path(flagged, 16, True) == "split_half"  # below the lowered hand-over point
    finally:
        monkeypatch.delenv("ULTR_SR_ATTN_LONG_MIN", raising=False)
        lib.ultr_config_reload()
    assert _streaming_table() == STREAMING_TABLE and _table() == DEFAULT_TABLE


def test_streaming_scalar_backward_refuses_head_depths_beyond_its_lds():
    """The scalar streaming backward keeps 160 (dh + 1) + 16 dh + 640 floats in LDS: 160 KiB at head depth 228.  The dispatch answers
    for the launch; the forward of such a model still streams (its kernel holds head depth 420)."""
    from ultra_pytorch_amd import _lib, hip_ops
    ok = hip_ops.SetRankShape(24, 456, 2, 1, 16, attention_backward="streaming")     # head depth 228
    wide = hip_ops.SetRankShape(24, 460, 2, 1, 16, attention_backward="streaming")   # head depth 230
    assert hip_ops.setrank_attn_path(ok, 300, True) == "long_scalar"
    assert hip_ops.setrank_attn_path(wide, 300) == "long_scalar"
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.setrank_attn_path(wide, 300, True)


def test_hparam_sets_the_flag():
    from ultra_pytorch_amd import _lib, hip_ops
    from ultra_pytorch_amd.ranking_model.SetRank import SetRank
    hp = "d_model=32,num_heads=2,num_layers=1,diff=16"
    assert _lib.MODEL_SR_STREAM_BWD == 2 and _lib.MODEL_FP32_PRODUCTS == 1
    m = SetRank(hp + ",attention_backward=streaming", 24)
    assert int(m.shape.desc.flags) & _lib.MODEL_SR_STREAM_BWD and m.shape.attention_backward == "streaming"
    assert int(SetRank(hp, 24).shape.desc.flags) == 0
    assert int(SetRank(hp + ",attention_backward=one_pass", 24).shape.desc.flags) == 0
    with pytest.raises(ValueError, match="attention_backward"):
        SetRank(hp + ",attention_backward=flash", 24)
    with pytest.raises(ValueError, match="attention_backward"):
        hip_ops.SetRankShape(24, 32, 2, 1, 16, attention_backward="")
    # the fp32-products switch joins the flag, it does not replace it
    m.shape.desc.flags = int(m.shape.desc.flags) | _lib.MODEL_FP32_PRODUCTS
    assert int(m.shape.desc.flags) == 3 and hip_ops.setrank_attn_path(m.shape, 300, True) == "long_mfma"


def test_fp32_fallback_keeps_the_streaming_flag(monkeypatch):
    import warnings
    from ultra_pytorch_amd import _lib, hip_ops
    monkeypatch.delenv("ULTR_SR_H3", raising=False)
    s = hip_ops.SetRankShape(24, 64, 2, 1, 16, attention_backward="streaming")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert hip_ops.fall_back_to_fp32_products(s, "test")
    assert int(s.desc.flags) == _lib.MODEL_SR_STREAM_BWD | _lib.MODEL_FP32_PRODUCTS


@pytest.mark.parametrize("model", [(24, 64, 2, 1, 16), (136, 256, 8, 2, 64), (20, 48, 6, 1, 20)], ids=lambda m: "d%d_H%d" % (m[1], m[2]))
def test_workspace_grows_for_a_streaming_model_only(model):
    """ultr_setrank_workspace_bytes: a descriptor without the flag returns what a second such descriptor returns (nothing in the call
    depends on anything but the descriptor and n_rows); one with the flag has room for t [n_rows, heads] on top."""
    from ultra_pytorch_amd import hip_ops
    a, b = hip_ops.SetRankShape(*model), hip_ops.SetRankShape(*model, attention_backward="one_pass")
    s = hip_ops.SetRankShape(*model, attention_backward="streaming")
    for n in (1, 37, 600, 2502, 102400):
        assert a.workspace_bytes(n) == b.workspace_bytes(n) > 0
        assert s.workspace_bytes(n) >= a.workspace_bytes(n) + 4 * n * model[2]
        assert s.workspace_bytes(n) <= a.workspace_bytes(n) + 4 * n * model[2] + 32
        assert s.saved_bytes(n) == a.saved_bytes(n)
