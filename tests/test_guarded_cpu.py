"""tests/guarded.py proved on CPU tensors with torch writes only (no project kernel involved): a word written one past the end or one
before the start of a view is reported with the right name, side and offset, a write at the far end of a band is caught, writes inside
a view are not reported, view lengths are exact, view starts are 512-byte aligned, zeroed views are zero and poisoned views hold
the pattern.  tests/test_gpu_workspace_bounds.py relies on exactly these properties."""
import numpy as np
import pytest
import torch

from tests import guarded as G

PAT = int(np.array([G.PATTERN], np.uint32).view(np.int32)[0])
LENGTHS = [1, 7, 128, 129, 1000, 4097]


def make():
    arena = G.Arena("cpu", G.bytes_for([4 * n for n in LENGTHS] + [8 * 5]))
    views = [arena.view(n, zero=(k % 2 == 1), name="v%d" % k) for k, n in enumerate(LENGTHS)]
    return arena, views


def word_of(arena, view, index):
    """The arena word `index` words from the start of `view` (negative: in front of it)."""
    _, start, _, _, _ = arena._record(view)
    return arena.buf[start + index:start + index + 1]


def test_pattern_is_a_quiet_nan_with_a_payload():
    f = np.array([G.PATTERN], np.uint32).view(np.float32)[0]
    assert np.isnan(f) and (G.PATTERN >> 22) & 0x1FF == 0x1FF and G.PATTERN & 0x3FFFFF == 0x05A5A5


def test_views_are_exact_aligned_disjoint_and_filled():
    arena, views = make()
    spans = []
    for k, (v, n) in enumerate(zip(views, LENGTHS)):
        assert v.dtype == torch.float32 and v.numel() == n and v.is_contiguous()
        assert v.data_ptr() % 512 == 0
        as_int = v.view(torch.int32)
        if k % 2 == 1:
            assert (as_int == 0).all()
            assert arena.untouched(v) == 0
        else:
            assert (as_int == PAT).all() and torch.isnan(v).all()
            assert arena.untouched(v) == n
        spans.append((v.data_ptr(), v.data_ptr() + 4 * n))
    lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + 4 * arena.buf.numel()
    for a, b in spans:  # one allocation, at least 1 MiB of band on either side of every view
        assert lo + G.BAND_BYTES <= a and b + G.BAND_BYTES <= hi
    for (a0, b0), (a1, b1) in zip(spans, spans[1:]):
        assert a1 - b0 >= 2 * G.BAND_BYTES  # a band of its own behind one view and in front of the next
    arena.check()


def test_the_64_bit_view():
    arena, _ = make()
    w = arena.view64(5, zero=True, name="ws64")
    assert w.dtype == torch.float64 and w.numel() == 5 and w.data_ptr() % 512 == 0 and (w == 0).all()
    arena.check()
    w.fill_(3.0)
    arena.check()
    word_of(arena, w, 10).fill_(1)  # the first word past five doubles
    with pytest.raises(G.GuardBreach) as e:
        arena.check()
    assert (e.value.name, e.value.side, e.value.first, e.value.last, e.value.count) == ("ws64", "behind", 10, 10, 1)
    p = G.Arena("cpu", G.bytes_for([8 * 3])).view64(3)
    # two pattern words read as a double are no NaN (its exponent field is 0x7FC, not 0x7FF) but 3.04e307: still nothing a sum survives
    assert (p.view(torch.int32) == PAT).all() and (p > 1e307).all()


def test_writes_inside_the_views_are_not_reported():
    arena, views = make()
    for v in views:
        v.fill_(1.5)
        v[0], v[-1] = -2.0, float("nan")
    arena.check()
    assert arena.untouched(views[0]) == 0


def test_partly_written_view_counts_the_untouched_words():
    arena, views = make()
    v = views[4]
    v[:300] = 0.0
    assert arena.untouched(v) == LENGTHS[4] - 300
    arena.check()


@pytest.mark.parametrize("k", range(len(LENGTHS)))
def test_one_word_past_the_end_is_reported(k):
    arena, views = make()
    n = LENGTHS[k]
    word_of(arena, views[k], n).fill_(0)
    with pytest.raises(G.GuardBreach) as e:
        arena.check()
    b = e.value
    assert (b.name, b.side, b.first, b.last, b.count, b.n_words) == ("v%d" % k, "behind", n, n, 1, n)
    assert "v%d" % k in str(b) and "behind" in str(b)


@pytest.mark.parametrize("k", range(len(LENGTHS)))
def test_one_word_before_the_start_is_reported(k):
    arena, views = make()
    word_of(arena, views[k], -1).fill_(0)
    with pytest.raises(G.GuardBreach) as e:
        arena.check()
    b = e.value
    assert (b.name, b.side, b.first, b.last, b.count) == ("v%d" % k, "front", -1, -1, 1)
    assert "in front of" in str(b)


def test_the_far_ends_of_the_bands_are_watched():
    band = G.BAND_BYTES // 4
    arena, views = make()
    word_of(arena, views[2], LENGTHS[2] + band - 1).fill_(7)  # 1 MiB behind the view, last word
    with pytest.raises(G.GuardBreach) as e:
        arena.check()
    assert (e.value.name, e.value.side, e.value.first) == ("v2", "behind", LENGTHS[2] + band - 1)
    arena, views = make()
    word_of(arena, views[0], -band).fill_(7)  # 1 MiB in front of the FIRST view: the arena's own first band word
    with pytest.raises(G.GuardBreach) as e:
        arena.check()
    assert (e.value.name, e.value.side, e.value.first) == ("v0", "front", -band)


def test_a_run_of_words_reports_first_last_and_count():
    arena, views = make()
    _, start, n, _, _ = arena._record(views[3])
    arena.buf[start + n + 4:start + n + 20:2] = 0  # eight words, every other one
    with pytest.raises(G.GuardBreach) as e:
        arena.check()
    assert (e.value.name, e.value.side, e.value.first, e.value.last, e.value.count) == ("v3", "behind", n + 4, n + 18, 8)


def test_a_nan_with_other_bits_is_a_change():
    """The compare is on the bits: another NaN, which no float compare could tell from the pattern, is reported."""
    arena, views = make()
    word_of(arena, views[1], LENGTHS[1]).view(torch.float32).fill_(float("nan"))
    with pytest.raises(G.GuardBreach):
        arena.check()


def test_a_full_arena_refuses():
    arena = G.Arena("cpu", G.bytes_for([4 * 10]))
    arena.view(10)
    with pytest.raises(MemoryError):
        arena.view(10)
