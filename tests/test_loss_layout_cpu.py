"""The LDS layouts of the seven list-loss kernels on the host (ultr_loss_lds_bytes reads the structs of csrc/ultr_listloss.h that the
kernels carve their dynamic LDS with and that their launchers request).  No GPU.

FLOATS pins every layout's total to the polynomial its launcher spelled out by hand before the layouts existed, LIMIT and L_MAX
to what those launchers accepted: an array added to a kernel moves the answer here, at every list size, not only near the longest
accepted list where the allocation granule stops hiding an overrun."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
JW = 16  # csrc/ultr_listloss.h: LOSS_JW, wavefronts per list of the pair-walk kernels (one list per workgroup)


def _tail(L):
    return 4 + 2 * L


# floats of dynamic LDS per algorithm
FLOATS = {
    "softmax": lambda L: _tail(L) + 2 * L,
    "regem": lambda L: _tail(L),
    "dla": lambda L: _tail(L) + 3 * L,
    "pairdebias": lambda L: _tail(L) + 2 * L + 2 * L + JW * L * 4,
    "lambdarank": lambda L: _tail(L) + 6 * L + 5 * L + JW * L * 4,
    "prs": lambda L: _tail(L) + 8 * L + L + JW * L * 2,
    "pdgd": lambda L: 6 * L + 1 + 4 + L * (L + 3) // 2,
}
LIMIT = {"softmax": 64 * 1024, "regem": 64 * 1024, "dla": 64 * 1024, "pairdebias": 160 * 1024, "lambdarank": 160 * 1024,
         "prs": 160 * 1024, "pdgd": None}  # PDGD: no LDS limit of its own, list_size <= 256 (one thread per position)
L_MAX = {"softmax": 4095, "dla": 3276, "regem": 8190, "pairdebias": 585, "lambdarank": 531, "prs": 952, "pdgd": 256}
E_BADARG, E_UNSUPPORTED = -1, -2


def _algo_id(name):
    from ultra_pytorch_amd import _lib
    return getattr(_lib, "ALGO_" + name.upper())


def _query(name, L):
    from ultra_pytorch_amd import _lib
    return int(_lib.load().ultr_loss_lds_bytes(_algo_id(name), L))


def _accepted(name, L):
    return L <= 256 if LIMIT[name] is None else FLOATS[name](L) * 4 <= LIMIT[name]


def test_declarations_agree():
    import ctypes
    from ultra_pytorch_amd import _lib
    hdr = (ROOT / "include" / "ultr_hip.h").read_text()
    assert re.search(r"\bint64_t ultr_loss_lds_bytes\(int32_t algo, int32_t list_size\);", hdr)
    assert _lib.SIGNATURES["ultr_loss_lds_bytes"] == (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32])
    assert _lib.load().ultr_loss_lds_bytes is not None  # (AttributeError: the built library does not export it)


def test_the_stated_bounds_follow_from_the_polynomials():
    for name, lmax in L_MAX.items():
        assert lmax == max(L for L in range(1, 10000) if _accepted(name, L)), name


@pytest.mark.parametrize("name", list(FLOATS))
def test_layout_bytes_equal_the_parents_polynomial(name):
    lengths = set(range(1, 1025)) | {L_MAX[name] - 1, L_MAX[name]}
    for L in sorted(lengths):
        if _accepted(name, L):
            assert _query(name, L) == FLOATS[name](L) * 4, (name, L)
        else:
            assert _query(name, L) == E_UNSUPPORTED, (name, L)


@pytest.mark.parametrize("name", list(FLOATS))
def test_longest_accepted_list_and_the_refusal_one_past_it(name):
    lmax = L_MAX[name]
    got = _query(name, lmax)
    assert got == FLOATS[name](lmax) * 4
    assert LIMIT[name] is None or got <= LIMIT[name]
    assert _query(name, lmax + 1) == E_UNSUPPORTED
    assert _query(name, 2 ** 31 - 1) == E_UNSUPPORTED  # (no 32-bit wrap-around back below the limit)


def test_bad_arguments():
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    for name in FLOATS:
        assert _query(name, 0) == E_BADARG and _query(name, -3) == E_BADARG
    assert int(lib.ultr_loss_lds_bytes(_lib.ALGO_DBGD, 10)) == E_BADARG  # no stand-alone loss kernel
    assert int(lib.ultr_loss_lds_bytes(-1, 10)) == E_BADARG and int(lib.ultr_loss_lds_bytes(99, 10)) == E_BADARG
    assert hip_ops.loss_lds_bytes(_lib.ALGO_PRS, 952) == FLOATS["prs"](952) * 4
    with pytest.raises(_lib.UltrHipError):
        hip_ops.loss_lds_bytes(_lib.ALGO_PRS, 953)


def test_the_header_states_each_bound():
    hdr = (ROOT / "include" / "ultr_hip.h").read_text()
    entry = {"softmax": "ultr_softmax_ce", "dla": "ultr_dla_loss", "regem": "ultr_regem_loss", "pairdebias": "ultr_pairdebias_loss",
             "lambdarank": "ultr_lambdarank_loss", "prs": "ultr_prs_loss", "pdgd": "ultr_pdgd_loss"}
    for name, fn in entry.items():
        comment = hdr[:hdr.index("int %s(" % fn)].rsplit("/*", 1)[1]
        assert "list_size up to %d " % L_MAX[name] in comment, (fn, L_MAX[name])
