"""A guarded arena for workspace-bounds tests (plain torch: the same code serves CPU and GPU tensors).

Every view is carved from ONE allocation, is exactly as long as asked (torch's caching allocator rounds every request up and packs
tensors into shared blocks, so a write a few KB past the end of an ordinary tensor lands in slack or in a neighbour and faults nothing),
starts on a 512-byte boundary (what the caching allocator gives the engines' own buffers: the kernels take the same aligned paths) and
has a guard band of at least 1 MiB in front of it and one behind it.  Bands, and views that are not asked zeroed, hold one quiet-NaN
bit pattern with a recognisable payload; check() compares the bands as int32 (NaN never equals NaN as a float) and names the view,
the side, the first and the last changed word and their count.  A kernel that READS a poisoned word it never wrote turns its result
into NaN or into other bits, which a bitwise comparison with an ordinary run shows."""
import numpy as np
import torch

PATTERN = 0x7FC5A5A5            # a quiet NaN (exponent all ones, top mantissa bit set) with the payload 0x45A5A5
BAND_BYTES = 1 << 20            # at least this much in front of and behind every view
ALIGN = 512                     # bytes: the caching allocator's granule

_PATTERN_I32 = int(np.array([PATTERN], np.uint32).view(np.int32)[0])


class GuardBreach(AssertionError):
    """A band changed.  first / last: word (4-byte) indices relative to the START of the view - front: -1 is the word just before the
    view, behind: n_words is the first word past its end."""

    def __init__(self, name, side, first, last, count, n_words):
        self.name, self.side, self.first, self.last, self.count, self.n_words = name, side, first, last, count, n_words
        where = ("%d .. %d words before its start" % (-first, -last) if side == "front"
                 else "%d .. %d words past its last word" % (first - n_words + 1, last - n_words + 1))
        super().__init__("guard band %s view '%s' (%d words) was written: %d word(s) changed, first at index %d, last at index %d "
                         "(%s)" % ("in front of" if side == "front" else "behind", name, n_words, count, first, last, where))


def _up(n, a):
    return (n + a - 1) // a * a


def bytes_for(lengths_in_bytes):
    """Capacity (bytes) an Arena needs for views of these byte lengths."""
    return sum(_up(int(n), ALIGN) + 2 * BAND_BYTES + ALIGN for n in lengths_in_bytes)


class Arena:
    def __init__(self, device, capacity_bytes=64 << 20):
        self.device = torch.device(device)
        n_words = (int(capacity_bytes) + ALIGN) // 4 + 1
        self.buf = torch.full((n_words,), _PATTERN_I32, dtype=torch.int32, device=self.device)
        # word offset of the first 512-byte boundary of the allocation (a CPU allocation is 64-byte aligned only)
        self._base = (-self.buf.data_ptr() % ALIGN) // 4
        self._cursor = self._base   # first word not yet given to a view or a band
        self.views = []             # (name, first word, n_words) in carving order; the bands follow from them

    # ---- carving ----------------------------------------------------------------------------------------------------------
    def _carve(self, n_bytes, name, zero):
        n_words = int(n_bytes) // 4
        front = self._cursor
        start = front + _up(BAND_BYTES // 4, ALIGN // 4)  # cursor is on a 512-byte boundary, so is start
        end = start + n_words
        behind_end = self._base + _up(end - self._base + BAND_BYTES // 4, ALIGN // 4)
        if behind_end > self.buf.numel():
            raise MemoryError("guarded arena of %d bytes is full: view '%s' of %d bytes needs %d more" %
                              (self.buf.numel() * 4, name, n_bytes, (behind_end - self.buf.numel()) * 4))
        self._cursor = behind_end
        name = name if name is not None else "view%d" % len(self.views)
        self.views.append((name, start, n_words, front, behind_end))
        words = self.buf[start:end]
        if zero:
            words.zero_()
        assert (self.buf.data_ptr() + 4 * start) % ALIGN == 0
        return words

    def view(self, n_floats, zero=False, name=None):
        """An exactly n_floats long float32 view: poisoned with PATTERN, or zeroed."""
        return self._carve(4 * int(n_floats), name, zero).view(torch.float32)

    def view64(self, n_doubles, zero=False, name=None):
        """The 64-bit variant: an exactly n_doubles long float64 view (512-byte, hence 8-byte, aligned).  Poisoned, a double reads
        as 3.04e307 (two pattern words: the exponent field is 0x7FC), not as a NaN."""
        return self._carve(8 * int(n_doubles), name, zero).view(torch.float64)

    # ---- checking ---------------------------------------------------------------------------------------------------------
    def _bands(self):
        for name, start, n, front, behind_end in self.views:
            yield name, "front", front, start, start, n
            yield name, "behind", start + n, behind_end, start, n

    def check(self):
        """Raise GuardBreach if any band word differs from PATTERN (the first breached band in carving order is reported)."""
        changed = None
        for _, _, a, b, _, _ in self._bands():
            c = (self.buf[a:b] != _PATTERN_I32).sum()
            changed = c if changed is None else changed + c
        if changed is None or int(changed.item()) == 0:   # one host read when all is well
            return
        for name, side, a, b, start, n in self._bands():
            idx = torch.nonzero(self.buf[a:b] != _PATTERN_I32).view(-1)
            if idx.numel():
                raise GuardBreach(name, side, a + int(idx[0].item()) - start, a + int(idx[-1].item()) - start, int(idx.numel()), n)

    def _record(self, view):
        ptr = view.data_ptr()
        for rec in self.views:
            if self.buf.data_ptr() + 4 * rec[1] == ptr and rec[2] * 4 == view.numel() * view.element_size():
                return rec
        raise KeyError("not a view of this arena")

    def untouched(self, view):
        """How many 4-byte words of a (poisoned) view still hold PATTERN - for reporting how loose a declared size is."""
        _, start, n, _, _ = self._record(view)
        return int((self.buf[start:start + n] == _PATTERN_I32).sum().item())

    def name_of(self, view):
        return self._record(view)[0]
