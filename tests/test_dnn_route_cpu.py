"""The DNN route query on the host (ultr_dnn_route: the route ultr_dnn_forward, ultr_dnn_backward, ultr_dnn_backward_softmax and the
fused step decide once per call; the older queries ultr_dnn_forward_tile_rows / ultr_dnn_backward_tile_rows / ultr_fused_fb_waves are
views of it).  No GPU: the planners fall back to 256 compute units where no device answers.

PARENT pins the older queries to what they answered before the route existed, recorded from that library on this CU count, for every
shape of the planner sweep, of the wide-tile tests and of the benchmark's DNN configs whose widths are all multiples of 4 - there the
answers must not move.  Two kinds of shape moved on purpose, because the older queries named a kernel that was not launched: widths that
are no multiple of 4 (not in the table; test_the_route_names_the_kernel_that_is_launched) and, under ULTR_NO_VEC=1, the shapes the table
records as per-layer (0): nothing takes the float4 paths there, the per-layer launches need them, and the call runs the 16-row tile
kernels (test_knob_subset_is_pinned_to_the_parent spells the rule out)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
ROUTE_FIELDS = ("fused_waves", "fwd", "fwd_rows", "bwd", "bwd_rows", "loss", "wg_split_half")
KNOBS = ("ULTR_FWD_WIDE", "ULTR_BIG_BWD", "ULTR_NO_FUSED_FB", "ULTR_NO_VEC", "ULTR_BWD_WIDE", "ULTR_BIG_FWD", "ULTR_FWD_R", "ULTR_BWD_R",
         "ULTR_FWD_NW", "ULTR_BWD_NW", "ULTR_FB_NW", "ULTR_FB_H3", "ULTR_FWD_H3", "ULTR_BWD_H3", "ULTR_WG_H3", "ULTR_FWD_WIDE_RMAX",
         "ULTR_FB_MAX_WG_PER_CU", "ULTR_WG_H3_MIN_ROWS")

# (F, hidden, B, L): (ultr_dnn_forward_tile_rows training, the same for evaluation, ultr_dnn_backward_tile_rows, ultr_fused_fb_waves)
PARENT = {
    (136, (), 4100, 1): (16, 16, 16, 0),  # sweep 00
    (24, (), 242, 17): (16, 16, 16, 0),  # sweep 03
    (24, (), 41, 100): (16, 16, 16, 0),  # sweep 04
    (24, (64,), 43, 101): (1017, 1017, 1017, 0),  # sweep 11
    (220, (128, 256), 12259, 1): (1048, 1048, 1048, 0),  # sweep 12
    (136, (128, 32, 128, 128), 1366, 9): (1049, 1049, 1049, 0),  # sweep 13
    (700, (), 1230, 10): (16, 16, 16, 0),  # sweep 14
    (24, (), 724, 17): (16, 16, 32, 0),  # sweep 15
    (220, (), 123, 100): (16, 16, 32, 0),  # sweep 16
    (136, (128, 64, 128), 1254, 10): (1049, 1049, 1049, 0),  # sweep 20
    (24, (40,), 737, 17): (16, 16, 32, 0),  # sweep 21
    (136, (), 125, 100): (16, 16, 32, 0),  # sweep 22
    (700, (), 125, 101): (16, 16, 16, 0),  # sweep 23
    (220, (), 1825, 9): (16, 16, 32, 0),  # sweep 25
    (700, (), 978, 17): (16, 16, 16, 0),  # sweep 33
    (136, (64,), 166, 100): (16, 16, 1033, 0),  # sweep 34
    (700, (), 7674, 1): (16, 16, 16, 0),  # sweep 42
    (220, (96, 64, 64), 41, 100): (1017, 1017, 1017, 0),  # sweep 52
    (136, (), 41, 101): (16, 16, 16, 0),  # sweep 53
    (700, (32,), 1229, 10): (0, 1049, 1049, 0),  # sweep 62
    (136, (96,), 123, 100): (1049, 1049, 1049, 0),  # sweep 64
    (24, (256, 128, 32, 32), 12528, 1): (1049, 1049, 1049, 0),  # sweep 66
    (24, (256,), 1251, 10): (1049, 1049, 1049, 0),  # sweep 68
    (220, (256,), 738, 17): (1050, 1050, 1050, 0),  # sweep 69
    (700, (48, 256), 124, 101): (0, 16, 0, 0),  # sweep 71
    (136, (512, 256, 128), 512, 20): (1040, 1040, 1040, 0),  # wide cfg3_three_tiles, bench 3
    (136, (256, 256), 300, 23): (1027, 1027, 1027, 0),  # wide two_tiles_ragged
    (700, (512, 256, 128), 256, 50): (1025, 1025, 1050, 0),  # wide cfg4_wide_input, bench 4pair / 4lambda
    (220, (96, 64), 200, 40): (1032, 1032, 1032, 0),  # wide odd_slices
    (136, (768, 32), 256, 40): (16, 16, 0, 0),  # wide chunks_beyond_waves
    (48, (64, 64, 32), 128, 60): (1030, 1030, 1030, 0),  # wide sigmoid_narrow
    (136, (256,), 400, 30): (1047, 1047, 1047, 0),  # wide one_hidden_layer
    (64, (128, 256, 128, 64), 350, 25): (1035, 1035, 1035, 0),  # wide four_hidden_layers
    (136, (256, 256), 256, 10): (16, 16, 16, 16),  # bench 2
}
# the wide-tile tests' shapes and the benchmark's, under one knob each
PARENT_KNOBS = {
    "ULTR_FWD_WIDE=0": {
        (136, (512, 256, 128), 512, 20): (16, 16, 1040, 0),
        (136, (256, 256), 300, 23): (16, 16, 1027, 0),
        (700, (512, 256, 128), 256, 50): (16, 16, 1050, 0),
        (220, (96, 64), 200, 40): (16, 16, 1032, 0),
        (136, (768, 32), 256, 40): (16, 16, 0, 0),
        (48, (64, 64, 32), 128, 60): (16, 16, 1030, 0),
        (136, (256,), 400, 30): (16, 16, 1047, 0),
        (64, (128, 256, 128, 64), 350, 25): (16, 16, 1035, 0),
        (136, (256, 256), 256, 10): (16, 16, 16, 16),
    },
    "ULTR_BIG_BWD=2": {
        (136, (512, 256, 128), 512, 20): (1040, 1040, 0, 0),
        (136, (256, 256), 300, 23): (1027, 1027, 0, 0),
        (700, (512, 256, 128), 256, 50): (1025, 1025, 0, 0),
        (220, (96, 64), 200, 40): (1032, 1032, 0, 0),
        (136, (768, 32), 256, 40): (16, 16, 0, 0),
        (48, (64, 64, 32), 128, 60): (1030, 1030, 0, 0),
        (136, (256,), 400, 30): (1047, 1047, 0, 0),
        (64, (128, 256, 128, 64), 350, 25): (1035, 1035, 0, 0),
        (136, (256, 256), 256, 10): (16, 16, 0, 16),
    },
    "ULTR_NO_FUSED_FB=1": {
        (136, (512, 256, 128), 512, 20): (1040, 1040, 1040, 0),
        (136, (256, 256), 300, 23): (1027, 1027, 1027, 0),
        (700, (512, 256, 128), 256, 50): (1025, 1025, 1050, 0),
        (220, (96, 64), 200, 40): (1032, 1032, 1032, 0),
        (136, (768, 32), 256, 40): (16, 16, 0, 0),
        (48, (64, 64, 32), 128, 60): (1030, 1030, 1030, 0),
        (136, (256,), 400, 30): (1047, 1047, 1047, 0),
        (64, (128, 256, 128, 64), 350, 25): (1035, 1035, 1035, 0),
        (136, (256, 256), 256, 10): (16, 16, 16, 0),
    },
    "ULTR_NO_VEC=1": {
        (136, (512, 256, 128), 512, 20): (16, 16, 16, 0),
        (136, (256, 256), 300, 23): (16, 16, 16, 0),
        (700, (512, 256, 128), 256, 50): (16, 16, 0, 0),
        (220, (96, 64), 200, 40): (16, 16, 16, 0),
        (136, (768, 32), 256, 40): (16, 16, 0, 0),
        (48, (64, 64, 32), 128, 60): (16, 16, 16, 0),
        (136, (256,), 400, 30): (16, 16, 32, 0),
        (64, (128, 256, 128, 64), 350, 25): (16, 16, 32, 0),
        (136, (256, 256), 256, 10): (16, 16, 16, 0),
    },
}


@pytest.fixture
def knob(monkeypatch):
    from ultra_pytorch_amd import _lib
    lib = _lib.load()

    def set_(**kw):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            assert k in KNOBS
            monkeypatch.setenv(k, str(v))
        lib.ultr_config_reload()

    try:
        set_()
        yield set_
    finally:
        monkeypatch.undo()
        lib.ultr_config_reload()


def _shape(F, hidden, act="elu"):
    from ultra_pytorch_amd import hip_ops
    return hip_ops.DnnShape(F, list(hidden), act)


def _legacy(F, hidden, B, L):
    sh = _shape(F, hidden)
    n = B * L
    return (sh.lib.ultr_dnn_forward_tile_rows(sh.desc, n, 1), sh.lib.ultr_dnn_forward_tile_rows(sh.desc, n, 0),
            sh.lib.ultr_dnn_backward_tile_rows(sh.desc, n), sh.lib.ultr_fused_fb_waves(sh.desc, B, L))


def _route(F, hidden, B, L, call):
    """ultr_dnn_route with the family and loss ids as their names."""
    from ultra_pytorch_amd import _lib
    r = _shape(F, hidden).route(B, L, call=call)
    return dict(r, fwd=_lib.DNN_FAMILIES[r["fwd"]], bwd=_lib.DNN_FAMILIES[r["bwd"]], loss=_lib.DNN_LOSS_PLACES[r["loss"]])


def _code(family, rows):
    """The older queries' encoding of a family."""
    return 0 if family == "per_layer" else 1000 + rows if family == "wide" else rows


def _sweep_cases():
    from tests import test_gpu_planner_sweep as S
    return S.CASES


def test_declarations_agree():
    from ultra_pytorch_amd import _lib
    hdr = (ROOT / "include" / "ultr_hip.h").read_text()
    assert re.search(r"\bint ultr_dnn_route\(const ultr_dnn_desc\* d, int32_t batch, int32_t list_size, int64_t n_docs, int32_t call, "
                     r"ultr_dnn_route_info\* out\);", hdr)
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION
    body = re.search(r"typedef struct ultr_dnn_route_info \{(.*?)\} ultr_dnn_route_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"int32_t ([^;]+);", body) for n in decl.split(",")]
    bound = [n if n != "reserved" else "reserved[5]" for n, _ in _lib.DnnRouteInfo._fields_]
    assert names == bound == list(ROUTE_FIELDS) + ["reserved[5]"]
    assert all(t is ctypes.c_int32 for n, t in _lib.DnnRouteInfo._fields_ if n != "reserved")
    assert ctypes.sizeof(_lib.DnnRouteInfo) == 4 * 12

    def enum(name):
        text = re.sub(r"/\*.*?\*/", "", re.search(r"enum %s \{(.*?)\};" % name, hdr, re.S).group(1), flags=re.S)
        return [(k, int(v)) for k, v in re.findall(r"(\w+) = (\d+)", text)]

    assert enum("ultr_dnn_route_call") == [("ULTR_DNN_CALL_" + n.upper(), i) for i, n in enumerate(_lib.DNN_CALLS)]
    assert enum("ultr_dnn_family") == [("ULTR_DNN_" + n.upper(), i) for i, n in enumerate(_lib.DNN_FAMILIES)]
    assert enum("ultr_dnn_loss_place") == [("ULTR_DNN_LOSS_" + n.upper(), i) for i, n in enumerate(_lib.DNN_LOSS_PLACES)]
    res, args = _lib.SIGNATURES["ultr_dnn_route"]
    assert res is ctypes.c_int32
    assert args == [ctypes.POINTER(_lib.DnnDesc), ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                    ctypes.POINTER(_lib.DnnRouteInfo)]
    lib = _lib.load()
    assert int(lib.ultr_abi_version()) == 8
    assert lib.ultr_dnn_route is not None  # (AttributeError: the built library does not export it)


def test_the_table_holds_every_shape_it_is_meant_to():
    import bench
    from tests import test_gpu_wide_tiles as W
    want = {(c["F"], tuple(c["hidden"]), c["B"], c["L"]) for c in _sweep_cases()[:72]
            if c["F"] % 4 == 0 and all(h % 4 == 0 for h in c["hidden"])}
    subset = {(F, tuple(hidden), B, L) for F, hidden, B, L, _, _ in W.SHAPES.values()}
    subset |= {(c["F"], tuple(c["hidden"]), c["B"], c["L"]) for c in bench.CONFIGS.values() if c["model"] == "dnn"}
    assert set(PARENT) == want | subset and len(want) == 25 and len(subset) == 9
    assert all(set(t) == subset for t in PARENT_KNOBS.values())


def test_older_queries_are_pinned_to_the_parent(knob):
    got = {k: _legacy(*k) for k in PARENT}
    assert got == PARENT, {k: (got[k], PARENT[k]) for k in PARENT if got[k] != PARENT[k]}


@pytest.mark.parametrize("setting", sorted(PARENT_KNOBS))
def test_knob_subset_is_pinned_to_the_parent(knob, setting):
    name, value = setting.split("=")
    knob(**{name: int(value)})
    want = dict(PARENT_KNOBS[setting])
    if name == "ULTR_NO_VEC":
        # The one rule by which answers moved: with no float4 path at all the per-layer launches do not apply (they need aligned
        # float4 operands, as ultr_dnn_forward / backward_impl always tested), so a shape the older query called per-layer (0)
        # launches the 16-row tile kernel - which its LDS fits at every shape here.
        moved = {k: tuple(16 if v == 0 else v for v in t[:3]) + t[3:] for k, t in want.items()}
        assert sum(moved[k] != want[k] for k in want) == 2  # cfg4_wide_input and chunks_beyond_waves: the backward
        want = moved
    got = {k: _legacy(*k) for k in want}
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    if name == "ULTR_NO_VEC":  # and the route says the same, kernel by kernel
        for k in want:
            r = _route(*k, call="step_dscores")
            assert (r["fwd"], r["bwd"], r["loss"], r["wg_split_half"]) == ("tile", "tile", "launch", 0), (k, r)


def test_older_queries_are_views_of_the_route(knob):
    for c in _sweep_cases():
        key = (c["F"], c["hidden"], c["B"], c["L"])
        fwd_train, fwd_eval, bwd, fused = _legacy(*key)
        step, ev, sm = _route(*key, call="step_dscores"), _route(*key, call="eval"), _route(*key, call="step_softmax")
        assert fwd_train == _code(step["fwd"], step["fwd_rows"]), (c, step)
        assert fwd_eval == _code(ev["fwd"], ev["fwd_rows"]), (c, ev)
        assert bwd == _code(step["bwd"], step["bwd_rows"]), (c, step)
        assert fused == sm["fused_waves"] and step["fused_waves"] == ev["fused_waves"] == 0, (c, sm)
        assert (ev["bwd"], ev["bwd_rows"], ev["loss"], ev["wg_split_half"]) == ("none", 0, "none", 0)
        if not fused:  # the separate calls of a softmax step: the same kernels, the loss placed by the backward's family
            assert {k: sm[k] for k in sm if k != "loss"} == {k: step[k] for k in step if k != "loss"}, (c, sm, step)


def test_the_route_names_the_kernel_that_is_launched(knob):
    """(Before the route existed the older queries answered "wide tile" for the first five, and nothing reached the fused launch.)"""
    cases = _sweep_cases()
    for k, F in ((43, 13), (44, 137), (45, 46), (58, 46), (70, 137)):
        c = cases[k]
        assert c["k"] == k and c["F"] == F and F % 4 != 0
        key = (c["F"], c["hidden"], c["B"], c["L"])
        r = _route(*key, call="step_softmax" if c["algo"] == "softmax" else "step_dscores")
        assert (r["fused_waves"], r["fwd"], r["fwd_rows"], r["bwd"], r["bwd_rows"]) == (0, "tile", 16, "tile", 16), (k, r)
        assert _legacy(*key)[:3] == (16, 16, 16), k
    r = _route(13, [64], 8, 10, "step_softmax")  # 80 rows in five 16-row tiles, but 13 features are no float4s
    assert (r["fused_waves"], r["fwd"], r["bwd"], r["loss"]) == (0, "tile", "tile", "prologue")
    r = _route(24, [256], 5, 16, "step_softmax")
    assert (r["fused_waves"], r["fwd"], r["fwd_rows"], r["bwd"], r["bwd_rows"], r["loss"]) == (16, "fused", 16, "fused", 16, "fused")
    r = _route(24, [256], 5, 17, "step_softmax")  # a list does not fit the 16-row tile
    assert (r["fused_waves"], r["fwd"], r["bwd"], r["loss"]) == (0, "tile", "tile2", "prologue")
    r = _route(24, [64, 32], 6, 9, "step_softmax")  # no split-half copies below 256 columns: 8 waves; one list of 9 per tile
    assert (r["fused_waves"], r["fwd"], r["fwd_rows"], r["bwd"], r["bwd_rows"], r["loss"]) == (8, "fused", 9, "fused", 9, "fused")
    for key in ((13, [64], 8, 10), (24, [256], 5, 16), (24, [256], 5, 17), (24, [64, 32], 6, 9)):
        r = _route(*key, call="step_dscores")
        assert r["fused_waves"] == 0 and r["fwd"] == "tile" and r["bwd"] in ("tile", "tile2") and r["loss"] == "launch", (key, r)
    assert _legacy(24, [256], 5, 16)[3] == 16 and _legacy(24, [256], 5, 17)[3] == 0 and _legacy(24, [64, 32], 6, 9)[3] == 8


def test_loss_placement_follows_the_backward(knob):
    place = {"wide": "launch", "per_layer": "launch", "tile": "prologue", "tile2": "prologue", "fused": "fused"}
    seen = set()
    for c in _sweep_cases():
        key = (c["F"], c["hidden"], c["B"], c["L"])
        r = _route(*key, call="step_softmax")
        assert r["loss"] == place[r["bwd"]], (c, r)
        seen.add((r["bwd"], r["loss"]))
        assert _route(*key, call="step_dscores")["loss"] == "launch" and _route(*key, call="eval")["loss"] == "none"
    assert seen == {(b, l) for b, l in place.items()}, seen


def test_a_call_the_library_refuses(knob):
    from ultra_pytorch_amd import _lib
    sh = _shape(4096, [])  # a 16-row tile of 4096 columns does not fit the LDS, and one Linear has no per-layer path
    info = _lib.DnnRouteInfo()
    for call, bwd in ((0, "none"), (1, "unsupported"), (2, "unsupported")):
        assert sh.lib.ultr_dnn_route(ctypes.byref(sh.desc), 8, 10, 80, call, ctypes.byref(info)) == -2
        assert (_lib.DNN_FAMILIES[info.fwd], _lib.DNN_FAMILIES[info.bwd]) == ("unsupported", bwd) and list(info.reserved) == [0] * 5
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        sh.route(8, 10)


def test_bad_arguments():
    from ultra_pytorch_amd import _lib
    sh = _shape(24, [64, 32])
    lib, info, d = sh.lib, _lib.DnnRouteInfo(), ctypes.byref(sh.desc)
    assert lib.ultr_dnn_route(d, 6, 9, 54, 1, ctypes.byref(info)) == 0 and info.fused_waves == 8
    assert lib.ultr_dnn_route(None, 6, 9, 54, 1, ctypes.byref(info)) == -1
    assert lib.ultr_dnn_route(d, 6, 9, 54, 1, None) == -1
    assert lib.ultr_dnn_route(d, 0, 9, 54, 1, ctypes.byref(info)) == -1
    assert lib.ultr_dnn_route(d, 6, 0, 54, 1, ctypes.byref(info)) == -1
    assert lib.ultr_dnn_route(d, 6, -9, 54, 1, ctypes.byref(info)) == -1
    assert lib.ultr_dnn_route(d, 6, 9, -1, 1, ctypes.byref(info)) == -1
    assert lib.ultr_dnn_route(d, 6, 9, 54, 3, ctypes.byref(info)) == -1
    assert lib.ultr_dnn_route(d, 6, 9, 54, -1, ctypes.byref(info)) == -1
    bad = _lib.make_desc(24, [64, 0])
    assert lib.ultr_dnn_route(ctypes.byref(bad), 6, 9, 54, 1, ctypes.byref(info)) == -1
    with pytest.raises(_lib.UltrHipError, match="bad argument"):
        sh.route(6, -1)
    with pytest.raises(ValueError):
        sh.route(6, 9, call="train")
