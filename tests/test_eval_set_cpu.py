"""The set-evaluation entry points (csrc/ultr_eval.hip) as far as they go without a GPU: declared in the header, typed in the binding,
exported by the library, refused on bad arguments before anything is launched; the device label feed reachable by class path."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ultr_eval_pick", "ultr_eval_accumulate", "ultr_dnn_eval_set")
BADARG = -1  # ULTR_E_BADARG
P = 0x1000   # a non-NULL pointer that is never dereferenced: every call below is refused before a launch


@pytest.fixture(scope="module")
def lib():
    from ultra_pytorch_amd import _lib, build
    build.build_library()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        fn = getattr(so, n)
        fn.restype, fn.argtypes = _lib.SIGNATURES[n]
    return so


def test_header_declares_the_three_entry_points_within_abi_8():
    h = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", h).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
    from ultra_pytorch_amd import _lib
    assert int(re.search(r"#define\s+ULTR_EVAL_RESET\s+(\d+)", h).group(1)) == _lib.EVAL_RESET
    assert int(re.search(r"#define\s+ULTR_EVAL_FINISH\s+(\d+)", h).group(1)) == _lib.EVAL_FINISH
    assert _lib.EVAL_SEQ_BYTE == 129 * 8 and re.search(r"#define\s+ULTR_EVAL_SEQ_BYTE\s+\(129 \* 8\)", h)
    assert _lib.ABI_VERSION == 8


def test_binding_lists_the_three_entry_points():
    from ultra_pytorch_amd import _lib
    for n in NAMES:
        assert n in _lib.SIGNATURES, n
    assert len(_lib.SIGNATURES["ultr_eval_pick"][1]) == 12
    assert len(_lib.SIGNATURES["ultr_eval_accumulate"][1]) == 8
    assert len(_lib.SIGNATURES["ultr_dnn_eval_set"][1]) == 30


def test_library_exports_the_three_entry_points(lib):
    for n in NAMES:
        assert getattr(lib, n) is not None
    assert lib.ultr_abi_version() == 8


def _pick(lib, lists=P, labels=P, n_queries=11, lmax=7, n_docs=100, start=0, batch=4, list_size=7, docids=P, labels_out=P):
    return lib.ultr_eval_pick(lists, labels, n_queries, lmax, n_docs, start, batch, list_size, docids, labels_out, None, None)


@pytest.mark.parametrize("kw", [dict(lists=None), dict(labels=None), dict(docids=None), dict(labels_out=None), dict(start=-1),
                                dict(batch=0), dict(batch=-3), dict(start=8, batch=4), dict(start=11, batch=1), dict(start=0, batch=12),
                                dict(list_size=0), dict(list_size=-1)])
def test_pick_refuses_bad_arguments(lib, kw):
    assert _pick(lib, **kw) == BADARG


@pytest.mark.parametrize("n_values", [0, 129, -1])
def test_accumulate_refuses_a_value_count_outside_1_to_128(lib, n_values):
    assert lib.ultr_eval_accumulate(P, n_values, 4, P, 0, P, 1, None) == BADARG


def test_accumulate_refuses_missing_pointers_and_unknown_flags(lib):
    assert lib.ultr_eval_accumulate(None, 4, 4, P, 0, P, 1, None) == BADARG
    assert lib.ultr_eval_accumulate(P, 4, 4, None, 0, P, 1, None) == BADARG
    assert lib.ultr_eval_accumulate(P, 4, 0, P, 0, P, 1, None) == BADARG
    assert lib.ultr_eval_accumulate(P, 4, 4, P, 4, P, 1, None) == BADARG
    assert lib.ultr_eval_accumulate(P, 4, 4, P, 2, None, 1, None) == BADARG  # ULTR_EVAL_FINISH without a report to write


def test_device_label_feed_resolves_by_class_path():
    from ultra_pytorch_amd import input_layer
    from ultra_pytorch_amd.utils import find_class
    assert find_class("ultra_pytorch_amd.input_layer.DeviceDirectLabelFeed") is input_layer.DeviceDirectLabelFeed
