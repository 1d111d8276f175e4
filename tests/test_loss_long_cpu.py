"""The long-list entries of the pair-walk losses on the host: declarations, the LDS layouts of csrc/ultr_listloss.h
(PairDebiasLongLds, LambdaRankLongLds, PrsLongLds) through ultr_loss_long_lds_bytes / ultr_loss_long_max_list, the routing rule
(hip_ops.loss_route), and the float32 oracle on an MSLR-sized case: the bars of tests/loss_ref.py are attainable in float32 at 1251
documents before a GPU is involved.  No GPU."""
import ctypes
import re
from pathlib import Path

import pytest

from tests import loss_long_ref as LR
from tests import loss_ref as R

ROOT = Path(__file__).resolve().parents[1]
E_BADARG, E_UNSUPPORTED = -1, -2
ALGOS = ("pairdebias", "lambdarank", "prs")
ENTRIES = {"ultr_pairdebias_loss_long": "pairdebias", "ultr_lambdarank_loss_long": "lambdarank", "ultr_prs_loss_long": "prs",
           "ultr_prs_loss_pw_long": "prs"}


def _id(name):
    from ultra_pytorch_amd import _lib
    return getattr(_lib, "ALGO_" + name.upper())


def _bytes(name, L):
    from ultra_pytorch_amd import _lib
    return int(_lib.load().ultr_loss_long_lds_bytes(_id(name), L))


def _max(name):
    from ultra_pytorch_amd import _lib
    return int(_lib.load().ultr_loss_long_max_list(_id(name)))


def test_declarations_agree_and_the_abi_is_still_8():
    from ultra_pytorch_amd import _lib
    hdr = (ROOT / "include" / "ultr_hip.h").read_text()
    assert re.search(r"#define ULTR_ABI_VERSION 8\b", hdr)
    assert re.search(r"\bint64_t ultr_loss_long_lds_bytes\(int32_t algo, int32_t list_size\);", hdr)
    assert re.search(r"\bint32_t ultr_loss_long_max_list\(int32_t algo\);", hdr)
    assert _lib.SIGNATURES["ultr_loss_long_lds_bytes"] == (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32])
    assert _lib.SIGNATURES["ultr_loss_long_max_list"] == (ctypes.c_int32, [ctypes.c_int32])
    lib = _lib.load()
    for fn in list(ENTRIES) + ["ultr_loss_long_lds_bytes", "ultr_loss_long_max_list"]:
        assert getattr(lib, fn) is not None  # (AttributeError: the built library does not export it)
    for fn in ENTRIES:  # a long entry takes the arguments of its short counterpart
        short = fn[:-len("_long")]
        assert re.search(r"\bint %s\(" % fn, hdr), fn
        assert _lib.SIGNATURES[fn] == _lib.SIGNATURES[short], fn
        args = lambda f: re.sub(r"\s+", " ", hdr[hdr.index("int %s(" % f):].split(";", 1)[0].split("(", 1)[1])
        assert args(fn) == args(short), fn


@pytest.mark.parametrize("name", ALGOS)
def test_layout_bytes_are_the_float_count_and_grow_with_the_list(name):
    lengths = sorted(set(range(1, 130)) | {585, 586, 1023, 1024, 1025, LR.MSLR, LR.MAX_LIST[name] - 1, LR.MAX_LIST[name]})
    got = [_bytes(name, L) for L in lengths]
    assert got == [LR.floats(name, L) * 4 for L in lengths]
    assert all(a < b for a, b in zip(got, got[1:]))


@pytest.mark.parametrize("name", ALGOS)
def test_bound_and_the_refusal_one_past_it(name):
    lmax = _max(name)
    assert lmax == LR.MAX_LIST[name] and LR.MSLR <= lmax < 20000
    assert 0 < _bytes(name, lmax) <= LR.LIMIT
    assert _bytes(name, lmax + 1) == E_UNSUPPORTED and LR.floats(name, lmax + 1) * 4 > LR.LIMIT
    assert _bytes(name, 20000) == E_UNSUPPORTED
    assert _bytes(name, 2 ** 31 - 1) == E_UNSUPPORTED  # (no 32-bit wrap-around back below the limit)
    assert _bytes(name, 0) == E_BADARG and _bytes(name, -3) == E_BADARG


def test_algorithms_without_a_long_kernel():
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    for algo in (_lib.ALGO_SOFTMAX, _lib.ALGO_DLA, _lib.ALGO_REGEM, _lib.ALGO_PDGD, _lib.ALGO_DBGD, -1, 99):
        assert int(lib.ultr_loss_long_lds_bytes(algo, 10)) == E_BADARG and int(lib.ultr_loss_long_max_list(algo)) == E_BADARG
    with pytest.raises(_lib.UltrHipError):
        hip_ops.loss_long_max_list(_lib.ALGO_SOFTMAX)
    assert hip_ops.loss_long_lds_bytes(_lib.ALGO_PRS, 1251) == LR.floats("prs", 1251) * 4
    with pytest.raises(_lib.UltrHipError):
        hip_ops.loss_long_lds_bytes(_lib.ALGO_PRS, LR.MAX_LIST["prs"] + 1)


def test_the_header_states_each_bound():
    hdr = (ROOT / "include" / "ultr_hip.h").read_text()
    for fn, name in ENTRIES.items():
        comment = hdr[:hdr.index("int %s(" % fn)].rsplit("/*", 1)[1]
        assert "list_size up to %d " % LR.MAX_LIST[name] in comment, (fn, LR.MAX_LIST[name])


def test_routing_hands_over_at_the_short_bound_and_nowhere_else():
    from ultra_pytorch_amd import _lib, hip_ops
    for name in ALGOS:
        algo, smax = _id(name), LR.SHORT_MAX[name]
        assert [hip_ops.loss_route(algo, L) for L in (1, 64, smax)] == ["short"] * 3
        assert [hip_ops.loss_route(algo, L) for L in (smax + 1, LR.MSLR, LR.MAX_LIST[name])] == ["long"] * 3
        for L in (LR.MAX_LIST[name] + 1, 20000, 2 ** 31 - 1):
            with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
                hip_ops.loss_route(algo, L)
        with pytest.raises(_lib.UltrHipError, match="bad argument"):
            hip_ops.loss_route(algo, 0)
    # the other losses keep their one kernel and its bound
    assert hip_ops.loss_route(_lib.ALGO_SOFTMAX, 4095) == "short" and hip_ops.loss_route(_lib.ALGO_PDGD, 256) == "short"
    for algo, L in ((_lib.ALGO_SOFTMAX, 4096), (_lib.ALGO_DLA, 3277), (_lib.ALGO_REGEM, 8191), (_lib.ALGO_PDGD, 257)):
        with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
            hip_ops.loss_route(algo, L)


@pytest.mark.parametrize("name", ("pairdebias", "lambdarank"))
def test_step_cases_leave_the_code_most_of_the_gradient_bar(name):
    """The whole-step cases of tests/test_gpu_losses_long.py compare with the float32 oracle: on them the oracle's own gradient is within
    half the bar of its float64 evaluation (loss_long_ref.STEP_SEED says how the seeds were chosen, at a quarter)."""
    share = LR.oracle_share(name)
    print("%s step case, seed %d: the float32 oracle uses %.2f of the gradient bar" % (name, LR.STEP_SEED[name], share))
    assert share <= LR.ORACLE_SHARE


@pytest.mark.parametrize("name", ("pairdebias", "lambdarank"))
def test_float32_oracle_holds_the_bars_at_1251_documents(name):
    """oracle.ultr_oracle.pairdebias_loss / lambdarank_loss (float32 torch) against the float64 restatement at L = 1251, B = 2, at
    TERMS_RTOL and SCALAR_RTOL as they stand."""
    from tests.test_loss_ref_cpu import hold_loss_bars, oracle_losses
    case = LR.make_case("long-cpu-%s-L%d" % (name, LR.MSLR), name, 2, LR.MSLR)
    hold_loss_bars(case, oracle_losses(case), LR.reference(case))
    whole = R.reference(case)  # ... and the list-by-list reference is the whole-batch restatement
    ref = LR.reference(case)
    for k in ("tail", "ds"):
        assert R.terms_excess(ref[k], whole[k], whole[k + "_abs"]) <= 1e-12, k
