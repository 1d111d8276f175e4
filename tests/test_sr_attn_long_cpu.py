"""SetRank beyond 256 documents, the part that needs no GPU: the float64 restatement of the streaming attention recurrence
(tests/sr_attn_long_ref.py) against the direct softmax and, end to end, against oracle.setrank_forward; and the dispatch table of the
attention kernels through hip_ops.setrank_attn_path (host-only: the library loads without a GPU)."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import sr_attn_long_ref as R

ROOT = Path(__file__).resolve().parents[1]
LENGTHS = [1, 16, 127, 128, 129, 257, 385]
TILES = [16, 64, 100, 128]  # 16 / 64 / 128 divide some of the lengths, 100 divides none; the kernels use 128 and 64


@pytest.mark.parametrize("dh", [8, 16, 64])
@pytest.mark.parametrize("L", LENGTHS)
def test_streamed_recurrence_is_the_direct_softmax(L, dh):
    """Running maximum and sum, rescale, masked tail rows, first tile: float64, every tile size - against softmax(q q^T / sqrt(dh)) q.
    Bound: both sides are float64 evaluations of the same real function; the streamed one adds at most one rounding per tile to every
    probability and reorders sums of <= 385 positive terms - 1e-12 relative is 4 orders above float64's 1.1e-16 x that count."""
    rng = np.random.RandomState(1000 * dh + L)
    x = rng.normal(size=(L, dh)) * 2.0  # logits up to ~ +-4 dh / sqrt(dh): a maximum that moves between tiles
    A, lse = R.direct_attention(x)
    for tile in TILES:
        As, ls = R.streamed_attention(x, tile)
        np.testing.assert_allclose(As, A, rtol=1e-12, atol=1e-12 * np.abs(A).max(), err_msg="tile %d" % tile)
        np.testing.assert_allclose(ls, lse, rtol=1e-12, atol=1e-12, err_msg="tile %d" % tile)


@pytest.mark.parametrize("dh", [8, 16, 64])
@pytest.mark.parametrize("L", [129, 257, 385])
def test_streamed_recurrence_with_all_negative_tiles(L, dh):
    """Score rows that are negative everywhere but on the diagonal: document 0 points one way, every other document the opposite way
    (query 0 sees only negative scores in every tile but the first; the others see a negative score for key 0), and the LAST document is
    almost zero, so its own key - the only non-negative score of its row - sits in the ragged last tile next to the zero rows past L.
    Those rows would score exactly 0; unmasked they would share the row's maximum and its sum."""
    rng = np.random.RandomState(7 * L + dh)
    u = rng.normal(size=dh)
    u *= 3.0 / np.linalg.norm(u)
    x = -u[None, :] * (1.0 + 0.1 * rng.uniform(size=(L, 1))) + 0.01 * rng.normal(size=(L, dh))
    x[0] = u * 2.0
    x[L - 1] = 1e-3 * rng.normal(size=dh) - 1e-2 * u
    s = (x @ x.T) / np.sqrt(dh)
    assert (s[0, 1:] < 0).all() and (s[1:, 0] < 0).all() and s[L - 1, L - 1] < 1e-3
    A, lse = R.direct_attention(x)
    for tile in TILES:
        As, ls = R.streamed_attention(x, tile)
        np.testing.assert_allclose(As, A, rtol=1e-12, atol=1e-12 * np.abs(A).max(), err_msg="tile %d" % tile)
        np.testing.assert_allclose(ls, lse, rtol=1e-12, atol=1e-12, err_msg="tile %d" % tile)


MODELS = {8: (20, 48, 6, 1, 20), 16: (24, 64, 4, 1, 16), 64: (24, 64, 1, 2, 16)}  # head depth -> (F, d, H, layers, dff)


@pytest.mark.parametrize("dh", [8, 16, 64])
@pytest.mark.parametrize("L", LENGTHS)
def test_streamed_forward_is_the_oracle_forward(L, dh):
    """End to end: the float64 forward with the streamed attention (tile 128, and 100, which divides no length) against the fp32
    oracle.  Bound 2e-6: the fp32 oracle's own distance to float64 at these widths is 1.6e-7 .. 2.9e-7 (measured with the direct
    float64 forward below, asserted at 1e-6), the streamed float64 forward adds nothing visible at that scale."""
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    F, d, H, nl, dff = MODELS[dh]
    shape = hip_ops.SetRankShape(F, d, H, nl, dff)
    feats, ids, _ = synthetic.make_batch(np.random.RandomState(11), 2, L, F, clicks=False, n_pad=2 if L > 8 else 0)
    p0 = init_setrank_params(shape, seed=9)
    ref = O.setrank_forward(p0, F, d, H, nl, dff, feats, ids).numpy()
    direct = R.setrank_forward(p0.numpy(), F, d, H, nl, dff, feats, ids)
    assert np.abs(direct - ref).max() < 1e-6
    for tile in (128, 100):
        got = R.setrank_forward(p0.numpy(), F, d, H, nl, dff, feats, ids, tile=tile)
        assert np.abs(got - direct).max() < 1e-12
        np.testing.assert_allclose(got, ref, atol=2e-6, rtol=0)


def test_header_declares_the_entry_point_within_abi_8():
    from ultra_pytorch_amd import _lib
    hdr = (ROOT / "include" / "ultr_hip.h").read_text()
    assert re.search(r"\bint32_t ultr_setrank_attn_path\(const ultr_setrank_desc\* c, int32_t list_size, int32_t backward\);", hdr)
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION
    enum = re.search(r"enum ultr_setrank_attn_path_id \{(.*?)\};", hdr, re.S).group(1)
    names = re.findall(r"ULTR_SR_ATTN_(\w+) = (\d+)", enum)
    assert [n.lower() for n, _ in names] == list(_lib.SR_ATTN_PATHS) and [int(v) for _, v in names] == list(range(6))


def _table():
    from ultra_pytorch_amd import hip_ops
    s32 = hip_ops.SetRankShape(24, 64, 2, 1, 16)            # head depth 32
    s8 = hip_ops.SetRankShape(20, 48, 6, 1, 20)             # head depth 8
    sh = hip_ops.SetRankShape(24, 64, 2, 1, 16, attention_dtype="fp16")

    def path(shape, L, backward=False):
        try:
            return hip_ops.setrank_attn_path(shape, L, backward)
        except hip_ops._lib.UltrHipError as e:
            assert "unsupported shape" in str(e)
            return "unsupported"

    rows = {("dh32", L): path(s32, L) for L in (16, 100, 128, 129, 256, 257, 8128, 20000)}
    rows[("dh8", 257)] = path(s8, 257)
    rows[("dh8", 100)] = path(s8, 100)
    rows[("dh32 backward", 100)] = path(s32, 100, True)
    rows[("dh32 backward", 256)] = path(s32, 256, True)
    rows[("dh32 backward", 257)] = path(s32, 257, True)
    rows[("dh32 fp16", 100)] = path(sh, 100)
    rows[("dh32 fp16", 300)] = path(sh, 300)
    return rows


DEFAULT_TABLE = {("dh32", 16): "mfma", ("dh32", 100): "mfma", ("dh32", 128): "mfma",  # today's families
                 ("dh32", 129): "scalar", ("dh32", 256): "scalar",                     # unchanged
                 ("dh32", 257): "long_mfma", ("dh32", 8128): "long_mfma", ("dh32", 20000): "long_mfma",
                 ("dh8", 257): "long_scalar", ("dh8", 100): "scalar",
                 ("dh32 backward", 100): "split_half", ("dh32 backward", 256): "unsupported", ("dh32 backward", 257): "unsupported",
                 ("dh32 fp16", 100): "f16", ("dh32 fp16", 300): "long_mfma"}


def test_dispatch_table(monkeypatch):
    """Which kernel family a shape takes.  ULTR_SR_ATTN_LONG_MIN lowers the forward's hand-over point and nothing else: at 17 every
    forward row from 17 documents on is a long family (L = 100 among them; 128, 129 and 256 lie above the hand-over point as well), while
    L = 16, the rows that were long already, every backward row and the refusals stay where they were; a value above 257 moves nothing."""
    from ultra_pytorch_amd import _lib
    lib = _lib.load()
    for k in ("ULTR_SR_ATTN_LONG_MIN", "ULTR_SR_SCALAR_ATTN", "ULTR_SR_ATTN_H3", "ULTR_SR_ATTN_H3_MASK"):
        monkeypatch.delenv(k, raising=False)
    try:
        lib.ultr_config_reload()
        assert _table() == DEFAULT_TABLE
        monkeypatch.setenv("ULTR_SR_ATTN_LONG_MIN", "17")
        assert _table() == DEFAULT_TABLE  # knobs are read once: nothing moves before the reload
        lib.ultr_config_reload()
        low = dict(DEFAULT_TABLE)
        for L in (100, 128, 129, 256):
            low[("dh32", L)] = "long_mfma"
        low[("dh8", 100)] = "long_scalar"
        low[("dh32 fp16", 100)] = "long_mfma"  # the streaming kernels are fp32: above the hand-over point attention_dtype=fp16 runs them
        assert _table() == low
        monkeypatch.setenv("ULTR_SR_ATTN_LONG_MIN", "300")
        lib.ultr_config_reload()
        assert _table() == DEFAULT_TABLE  # 257 .. 299 are streamed all the same (("dh32", 257) above)
    finally:
        monkeypatch.delenv("ULTR_SR_ATTN_LONG_MIN", raising=False)
        lib.ultr_config_reload()
    assert _table() == DEFAULT_TABLE


def test_bad_descriptor_is_a_bad_argument():
    import ctypes
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    shape = hip_ops.SetRankShape(24, 64, 2, 1, 16)
    assert lib.ultr_setrank_attn_path(ctypes.byref(shape.desc), 0, 0) == -1
    assert lib.ultr_setrank_attn_path(None, 100, 0) == -1
    with pytest.raises(_lib.UltrHipError, match="bad argument"):
        hip_ops.setrank_attn_path(shape, -3)


@pytest.mark.parametrize("L,g", [(1251, 2.0), (4100, 2.0), (8128, 1.5), (8128, 2.5)])
def test_float32_error_does_not_grow_with_the_tile_count(L, g):
    """The matrix-core kernel's arithmetic restated in float32 (sr_attn_long_ref.streamed_attention_f32), head depth 32, normal inputs
    times g (logits of several units: a maximum that rises in a handful of tiles and then stands), 10 to 64 tiles of 128 keys, the first
    256 queries, against a float64 softmax.  Bound: twice the error of the SAME arithmetic with the whole list as one tile (no rescale
    at all).  The rescale factor is exactly 1 while the maximum stands, so tiling adds one rounding per rise and a reordering of the
    sums - nothing that scales with the tile count; the factor 2 is room for two maxima over 8192 entries of like-sized errors.
    The factor formed as 2^(fma(m, c1, -m2)) is not 1 there: measured 1.8e-5 / 2.7e-5 / 3.8e-5 at the three longer cases against
    4.9e-6 / 4.9e-6 / 5.0e-6 - the test has to see that, and says so."""
    nq = 256
    x = (np.random.RandomState(L).normal(size=(L, 32)) * g).astype(np.float32)
    x64 = x.astype(np.float64)
    s = (x64[:nq] @ x64.T) / np.sqrt(32.0)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    ref = (e / e.sum(axis=1, keepdims=True)) @ x64
    one_tile = float(np.abs(R.streamed_attention_f32(x, L, nq) - ref).max())
    tiled = float(np.abs(R.streamed_attention_f32(x, 128, nq) - ref).max())
    defect = float(np.abs(R.streamed_attention_f32(x, 128, nq, rescale="fma") - ref).max())
    print("L %d g %.1f: one tile %.3g, tiles of 128 %.3g, with the fma-formed factor %.3g" % (L, g, one_tile, tiled, defect))
    assert tiled <= 2.0 * one_tile
    if L >= 4100:
        assert defect > 2.0 * one_tile


def test_head_depths_beyond_the_lds_are_refused_by_the_gate():
    """The scalar kernels keep rows of the head depth in LDS: 80 (dh + 1) + 16 dh + 256 floats for the streaming one (160 KiB at head
    depth 424), L (dh + 5) floats for the one-pass forward.  The dispatch answers for the launch: a shape it names is a shape that runs."""
    from ultra_pytorch_amd import _lib, hip_ops
    ok, wide = hip_ops.SetRankShape(24, 840, 2, 1, 16), hip_ops.SetRankShape(24, 1024, 2, 1, 16)  # head depth 420 / 512
    assert hip_ops.setrank_attn_path(ok, 300) == "long_scalar" and hip_ops.setrank_attn_path(ok, 20000) == "long_scalar"
    assert hip_ops.setrank_attn_path(wide, 16) == "scalar"
    for L in (100, 256, 257, 1251):
        with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
            hip_ops.setrank_attn_path(wide, L)
