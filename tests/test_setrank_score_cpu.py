"""The scoring entry of SetRank's C ABI, host side (no GPU): ultr_setrank_score and its two sizing queries are declared and bound,
and ultr_setrank_score_bytes obeys the conditions the scoring layout was derived from (csrc/ultr_sr_plan.h: sr_make_score_plan) -
the activation part does not grow with num_layers, is at most 0.45 of `saved` at config 5's model from 1024 rows on and smaller
than `saved` everywhere; the range word lies inside the buffer behind 16-byte aligned planes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ultr_setrank_score_bytes", "ultr_setrank_score_range_flag_offset", "ultr_setrank_score")
TS = (1, 10, 1024, 320256)
CFG5 = (136, 256, 8, 2, 64)  # F, d_model, heads, layers, dff
ODD = [(13, 24, 3, nl, 10) for nl in (1, 2, 3, 4)]


def shape(m, **kw):
    from ultra_pytorch_amd import hip_ops
    return hip_ops.SetRankShape(m[0], d_model=m[1], num_heads=m[2], num_layers=m[3], dff=m[4], **kw)


def test_header_and_bindings_have_the_entry():
    from ultra_pytorch_amd import _lib
    src = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH) if os.path.exists(_lib.LIB_PATH) else _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"int64_t\s+ultr_setrank_score_bytes\(const ultr_setrank_desc\* c, int64_t n_rows\);", src)
    assert re.search(r"int64_t\s+ultr_setrank_score_range_flag_offset\(const ultr_setrank_desc\* c, int64_t n_rows\);", src)
    # eleven arguments: the training forward's with (work, work_bytes) for `saved`
    assert len(_lib.SIGNATURES["ultr_setrank_score"][1]) == len(_lib.SIGNATURES["ultr_setrank_forward"][1]) + 1
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION == 8
    assert _lib.load().ultr_abi_version() == 8


@pytest.mark.parametrize("T", TS)
def test_activation_part_does_not_depend_on_num_layers(T):
    acts = set()
    for m in ODD + [CFG5, CFG5[:3] + (4,) + CFG5[4:]]:
        sh = shape(m)
        acts.add((m[:3] + m[4:], sh.score_bytes(T) - sh.score_bytes(0)))
        # ... and the planes are the training forward's: two descriptors that differ in num_layers differ by them alone
        assert sh.score_bytes(0) == sh.saved_bytes(0)
    assert len(acts) == 2, acts  # one figure per (F, d, H, dff)


@pytest.mark.parametrize("T", [1024, 1025, 4100, 102400, 320256])
def test_config5_activations_are_at_most_045_of_saved(T):
    """Derived, not measured: 2 F + dff + 4 d = 1360 of the 3368 floats per token the backward's record holds is 0.40 (the layout here
    keeps the normalised input rows only, F + dff + 4 d = 1224: 0.36)."""
    sh = shape(CFG5)
    score, saved = sh.score_bytes(T) - sh.score_bytes(0), sh.saved_bytes(T) - sh.saved_bytes(0)
    print("T %d: %d of %d activation bytes (%.3f), %.0f bytes per token" % (T, score, saved, score / saved, score / T))
    assert score <= 0.45 * saved
    assert score <= 0.45 * sh.saved_bytes(T)  # (the planes, rebuilt per call, are the same in both buffers)
    assert score <= (2 * 136 + 64 + 4 * 256) * 4 * T + 6 * 16  # the issue's arithmetic (six buffers, each rounded up to 16 bytes)


@pytest.mark.parametrize("m", ODD + [CFG5, (12, 64, 4, 1, 32), (1, 1, 1, 1, 1), (700, 1024, 8, 8, 512)], ids=str)
def test_sizes_over_descriptors(m):
    prev = None
    for kw in ({}, {"attention_backward": "streaming"}, {"attention_dtype": "fp16"}):
        sh = shape(m, **kw)
        sizes = []
        for T in TS:
            n, off = sh.score_bytes(T), sh.score_range_flag_offset(T)
            assert 0 < n < sh.saved_bytes(T), (T, n, sh.saved_bytes(T))
            assert n % 4 == 0 and 0 <= off and 4 * off + 4 <= n  # the word lies inside the buffer
            # the planes sit between the activations and the word, a multiple of 16 bytes from the start
            planes_off = off - (sh.range_flag_offset(T) - _planes_float_offset(sh, T))
            assert planes_off % 4 == 0 and planes_off * 4 < n
            sizes.append(n)
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)  # monotone in T
        assert sh.score_bytes(0) > 0  # planes and word alone
        # a stream-backward-flagged (or fp16-attention) descriptor sizes as the plain one
        assert prev is None or sizes == prev
        prev = sizes


def _planes_float_offset(sh, T):
    """Float offset of the planes in `saved`: the activations of sr_make_plan, each piece rounded up to four floats, four floats
    spare, rounded up to eight (ultr_sr_plan.h) - restated here so the test does not take the offset from the code it checks."""
    F, d, H, nl, dff = sh.feature_size, sh.d_model, sh.num_heads, sh.num_layers, sh.dff
    up = lambda n: (n + 3) & ~3  # noqa: E731
    s = up(T * F) * 2 + up(T) * 2 + up(T * dff) * 2 + (nl + 1) * up(T * d)
    s += nl * (4 * up(T * d) + up(T * dff) + 4 * up(T) + up(T * H))
    return (s + 4 + 7) & ~7


def test_planes_offset_restated():
    """The restatement above against the library: `saved` of 0 rows is planes + word, so saved_bytes(T) - saved_bytes(0) is the
    planes' offset (up to the rounding of an empty layout)."""
    for m in ODD + [CFG5]:
        sh = shape(m)
        for T in TS:
            assert sh.saved_bytes(T) - sh.saved_bytes(0) == 4 * (_planes_float_offset(sh, T) - _planes_float_offset(sh, 0))


def test_bad_descriptors_size_to_nothing():
    from ultra_pytorch_amd import _lib
    lib = _lib.load()
    bad = [_lib.SetRankDesc(0, 24, 3, 1, 10, 0), _lib.SetRankDesc(13, 24, 5, 1, 10, 0), _lib.SetRankDesc(13, 24, 3, 9, 10, 0),
           _lib.SetRankDesc(13, 24, 3, 0, 10, 0), _lib.SetRankDesc(13, 24, 3, 1, 0, 0), _lib.SetRankDesc(13, 24, 3, 1, 10, 7)]
    for d in bad:
        for T in TS:
            assert lib.ultr_setrank_score_bytes(ctypes.byref(d), T) == 0
            assert lib.ultr_setrank_score_range_flag_offset(ctypes.byref(d), T) == -1
    good = _lib.SetRankDesc(13, 24, 3, 1, 10, 0)
    assert lib.ultr_setrank_score_bytes(ctypes.byref(good), -1) == 0
    assert lib.ultr_setrank_score_bytes(None, 10) == 0 and lib.ultr_setrank_score_range_flag_offset(None, 10) == -1
