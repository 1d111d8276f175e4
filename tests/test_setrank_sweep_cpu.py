"""The SetRank sweep, the part that needs no GPU: the route query is declared, bound and exported within ABI 8; the case table
(tests/setrank_sweep_cases.py) holds every rule it names and is the same on every import; the torch-fp32 oracle alone stays within
half of every bar against the float64 restatement on every case - the condition under which a miss on the GPU means the kernel; and
the route query's answers on the host, where no device answers and sr_cu_count falls back to 256 compute units."""
import ctypes
import importlib
import re
from pathlib import Path

import pytest

from tests import setrank_sweep_cases as C

ROOT = Path(__file__).resolve().parents[1]
ROUTE_FIELDS = ("embed", "block", "head_rides", "skip_out1", "bwd_head", "bwd_blocks", "bwd_embed", "rows_per_tile", "tiles",
                "workgroups", "block_rows", "embed_rows", "wgrad_split")


def test_route_query_is_declared_bound_and_exported_within_abi_8():
    from ultra_pytorch_amd import _lib
    hdr = (ROOT / "include" / "ultr_hip.h").read_text()
    assert re.search(r"\bint ultr_setrank_route\(const ultr_setrank_desc\* c, int32_t batch, int32_t list_size, int32_t dropout, "
                     r"ultr_setrank_route_info\* out\);", hdr)
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION
    body = re.search(r"typedef struct ultr_setrank_route_info \{(.*?)\} ultr_setrank_route_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"int32_t ([^;]+);", body) for n in decl.split(",")]
    bound = [n if n != "reserved" else "reserved[3]" for n, _ in _lib.SetRankRouteInfo._fields_]
    assert names == bound == list(ROUTE_FIELDS) + ["reserved[3]"]
    assert ctypes.sizeof(_lib.SetRankRouteInfo) == 4 * 16
    res, args = _lib.SIGNATURES["ultr_setrank_route"]
    assert res is ctypes.c_int32 and len(args) == 5
    lib = _lib.load()
    assert int(lib.ultr_abi_version()) == 8
    assert lib.ultr_setrank_route is not None  # (AttributeError: the built library does not export it)


def test_case_table_holds_every_rule_and_is_the_same_on_every_import():
    tags = {c.tag for c in C.CASES}
    assert tags == set(C.TAGS), (tags ^ set(C.TAGS))
    assert set(C.DETERMINISM_TAGS) <= tags and set(C.WIDENED) <= set(C.BY_ID) and set(C.SALT) <= set(C.BY_ID)
    before = C.CASES
    again = importlib.reload(C)
    assert again.CASES == before and [c.id for c in again.CASES] == [c.id for c in before]
    by = {}
    for c in C.CASES:
        by.setdefault(c.tag, []).append(c)
        assert c.kind in ("whole", "live") and c.features_offset_bytes in (0, 4) and c.L >= 2 and c.B * c.L < 17000
        assert c.d % c.H == 0 and 1 <= c.nl <= 8
    # the rules by value
    assert all(c.dff < 16 for c in by["dff_below_16"]) and all(c.dff > 256 for c in by["dff_above_256"])
    assert {c.dff % 4 for c in by["dff_above_256"]} == {0, 2}
    assert [c.dff for c in by["dff_96"]] == [96]
    assert sorted(c.d for c in by["d_ln_v4"]) == [512, 768, 1024] and all(c.d > 1024 for c in by["d_above_1024"])
    assert sorted(c.F for c in by["F_edges"]) == [256, 257, 260, 700, 1024, 1028, 1030]
    assert sorted(c.F for c in by["persistent_mixed"]) == [221, 256, 260] and all((c.d, c.dff) == (256, 64) for c in by["persistent_mixed"])
    assert {c.nl for c in by["depth"]} == {3, 5, 8} and all(c.H == 1 for c in by["one_head"])
    assert sorted(c.B * c.L for c in by["wg_split"]) == [1022, 1024, 1536]
    assert sorted(c.B * c.L for c in by["partials"]) == [64, 64, 65, 65, 128, 128, 129, 129]
    knobs = [dict(c.knobs) for c in by["knobs"]]
    assert sorted(k["ULTR_SR_BWD_FUSED"] for k in knobs if "ULTR_SR_BWD_FUSED" in k) == [1, 2, 3, 4, 5]
    assert sorted(k["ULTR_SR_BLOCK"] for k in knobs if "ULTR_SR_BLOCK" in k) == [0, 2]
    assert {"ULTR_SR_WG_H3": 0} in knobs and sum(c.fp32_products for c in by["knobs"]) == 1
    assert len(by["features_misaligned"]) == 3 and all(c.features_offset_bytes == 4 for c in by["features_misaligned"])
    assert all(c.features_offset_bytes == 0 for c in C.CASES if c.tag != "features_misaligned")
    live = [c for c in C.CASES if c.kind == "live"]
    assert {c.tag for c in live} == {"persistent_geometry", "round5_geometry", "round5_lds_cap", "round5_on_persistent_widths"}
    assert sorted(c.B * c.L for c in by["persistent_geometry"]) == [255, 4097, 16384, 16400]
    assert sorted(c.B * c.L for c in by["round5_geometry"]) == [8208, 16384, 16400]
    assert sorted(c.B * c.L for c in by["round5_lds_cap"]) == [13312, 13328]


def test_inputs_are_seeded_per_case():
    a, b = C.CASES[0].id, C.CASES[1].id
    first = C.inputs(a)
    C.inputs.cache_clear()
    again = C.inputs(a)
    assert all((x == y).all() for x, y in zip(first[:4], again[:4]))
    assert C.inputs(a).params[:8].tolist() != C.inputs(b).params[:8].tolist()
    live = C.inputs([c.id for c in C.CASES if c.kind == "live"][0])
    B = live.docids.shape[1]
    assert live.live[0] == 0 and live.live[-1] == B - 1 and len(set(live.live.tolist())) == 5
    y = C.labels_for([c.id for c in C.CASES if c.kind == "live"][0], "na")
    assert (y[:, live.live] == live.labels[:, live.live]).all() and (y[:, 1 if 1 not in live.live else 2] < 0).all()


@pytest.mark.parametrize("case", C.CASES, ids=[c.id for c in C.CASES])
def test_the_fp32_oracle_alone_is_within_half_of_every_bar(case):
    """torch-fp32 autograd against the float64 restatement at the case's own inputs (kind "live": the five live lists): every figure
    of setrank_sweep_cases.figures at most 0.5.  Two independently rounded fp32 implementations of the same step then sit within the bar
    of each other's float64 limit, so a kernel that misses a bar against float64 is wrong, not unlucky."""
    wide_names = C.WIDENED.get(case.id, ((), ""))[0]
    justified = False
    for algo in C.ALGOS:
        f = C.oracle_figures(case.id, algo)
        print("%s %s: oracle / bar  scores %.3f  loss %.3f  grads %.3f  tensor %.3f (%s)"
              % (case.id, algo, f["scores"], f["loss"], f["grads"], f["tensor"], f["worst_tensor"]))
        wide = C.tensor_bars(case.id, algo)
        assert set(wide) == set(wide_names)
        for k in ("scores", "loss", "grads"):
            assert f[k] <= 0.5, (case.id, algo, k, f[k])
        for n, v in f["tensors"].items():
            # a widened bar is 4 x the oracle's figure there (or the golden bar where that is the larger): the oracle sits at a quarter
            assert v <= 0.5 * wide.get(n, 1.0), (case.id, algo, n, v)
            justified = justified or (n in wide and 4.0 * v > 1.0)
    # a bar is widened only where the oracle alone, times 4, exceeds it
    assert justified == bool(wide_names), (case.id, wide_names)


# ---- the route query on the host -----------------------------------------------------------------------------------------------------
@pytest.fixture
def knob(monkeypatch):
    from ultra_pytorch_amd import _lib
    lib = _lib.load()

    def set_(**kw):
        for k in C.KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            assert k in C.KNOBS
            monkeypatch.setenv(k, str(v))
        lib.ultr_config_reload()

    try:
        set_()
        yield set_
    finally:
        monkeypatch.undo()
        lib.ultr_config_reload()


def _shape(F, d=256, H=8, nl=2, dff=64):
    from ultra_pytorch_amd import hip_ops
    return hip_ops.SetRankShape(F, d_model=d, num_heads=H, num_layers=nl, dff=dff)


def test_route_of_the_persistent_widths_by_feature_size(knob):
    """(6, 20, F, 256, 8, 2, 64): 120 rows on 256 compute units - tiles of 4 rows, 30 of them, one workgroup each."""
    geometry = dict(rows_per_tile=4, tiles=30, workgroups=30, block_rows=16, wgrad_split=1)
    fused = dict(block=2, head_rides=1, skip_out1=1, bwd_head=1, bwd_blocks=1)
    r = _shape(256).route(6, 20)
    assert set(r) == set(ROUTE_FIELDS)
    assert r == dict(fused, embed=1, bwd_embed=1, embed_rows=16, **geometry)
    for F in (260, 221):  # beyond 256 features / no whole float4s: both embedding launches step aside, the rest stays fused
        assert _shape(F).route(6, 20) == dict(fused, embed=0, bwd_embed=0, embed_rows=0, **geometry), F


def test_route_under_the_block_knob(knob):
    want = {0: dict(block=0, embed=0, head_rides=0, skip_out1=0, block_rows=0, embed_rows=0),
            2: dict(block=1, embed=1, head_rides=1, skip_out1=1, block_rows=16, embed_rows=16),
            3: dict(block=2, embed=1, head_rides=1, skip_out1=1, block_rows=16, embed_rows=16)}
    sh = _shape(24)
    for v, w in want.items():
        knob(ULTR_SR_BLOCK=v)
        r = sh.route(6, 20)
        assert {k: r[k] for k in w} == w, (v, r)
        # the backward's fused launches do not depend on the forward's block kernel
        assert (r["bwd_head"], r["bwd_blocks"], r["bwd_embed"], r["rows_per_tile"], r["tiles"], r["workgroups"]) == (1, 1, 1, 4, 30, 30)
    knob()
    assert sh.route(6, 20)["block"] == 2  # the default is 3


def test_route_under_the_fused_backward_bits(knob):
    sh = _shape(24)
    for bits in range(8):
        knob(ULTR_SR_BWD_FUSED=bits)
        r = sh.route(6, 20)
        assert (r["bwd_blocks"], r["bwd_head"], r["bwd_embed"]) == (bits & 1, (bits >> 1) & 1, (bits >> 2) & 1), (bits, r)
        assert r["skip_out1"] == (bits & 1) and r["block"] == 2


def test_dropout_and_fp32_products_take_the_all_zero_route(knob):
    from ultra_pytorch_amd import _lib
    sh = _shape(24)
    zero = {k: 0 for k in ROUTE_FIELDS if k != "wgrad_split"}
    r = sh.route(6, 20, dropout=True)
    assert {k: r[k] for k in zero} == zero and r["wgrad_split"] == 1  # (wgrad_split is the plan's, not the route's)
    assert sh.route(6, 20)["block"] == 2
    sh.desc.flags = int(sh.desc.flags) | _lib.MODEL_FP32_PRODUCTS
    r = sh.route(6, 20)
    assert {k: r[k] for k in zero} == zero
    knob(ULTR_SR_H3=0)  # the same through the process-wide knob
    r = _shape(24).route(6, 20)
    assert {k: r[k] for k in zero} == zero


def test_route_geometry_on_256_compute_units(knob):
    """What the geometry cases are chosen for, as the library answers where no device does (256 compute units)."""
    P, R5, CAP = _shape(24, 256, 8, 1, 64), _shape(24, 64, 2, 1, 32), _shape(24, 256, 8, 1, 128)
    r = P.route(1024, 16)
    assert (r["rows_per_tile"], r["tiles"], r["workgroups"]) == (64, 256, 256)
    r = P.route(1025, 16)  # one list more: a second round, tiles of 36 rows
    assert (r["rows_per_tile"], r["tiles"], r["workgroups"]) == (36, 456, 256)
    r = P.route(241, 17)
    assert (r["rows_per_tile"], r["tiles"], r["workgroups"]) == (20, 205, 205) and 4097 % 20 != 0
    r = P.route(17, 15)
    assert (r["rows_per_tile"], r["tiles"], r["workgroups"]) == (4, 64, 64)
    assert [R5.route(B, 16)["block_rows"] for B in (1024, 1025, 513)] == [32, 17, 17] and R5.route(1024, 16)["block"] == 1
    cap = max(CAP.route(B, 16)["block_rows"] for B in range(32, 4097, 32))
    assert 16 < cap < 32 and CAP.route(832, 16)["block_rows"] == cap and CAP.route(833, 16)["block_rows"] == 16
    assert [_shape(13, 24, 3, 1, 10).route(B, L)["wgrad_split"] for B, L in ((64, 16), (511, 2), (96, 16))] == [2, 1, 3]


def test_bad_arguments():
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    sh = _shape(24)
    info = _lib.SetRankRouteInfo()
    assert lib.ultr_setrank_route(None, 6, 20, 0, ctypes.byref(info)) == -1
    assert lib.ultr_setrank_route(ctypes.byref(sh.desc), 6, 20, 0, None) == -1
    assert lib.ultr_setrank_route(ctypes.byref(sh.desc), 0, 20, 0, ctypes.byref(info)) == -1
    assert lib.ultr_setrank_route(ctypes.byref(sh.desc), 6, 0, 0, ctypes.byref(info)) == -1
    bad = _lib.SetRankDesc(24, 256, 7, 2, 64, 0)  # 256 % 7 != 0
    assert lib.ultr_setrank_route(ctypes.byref(bad), 6, 20, 0, ctypes.byref(info)) == -1
    with pytest.raises(_lib.UltrHipError, match="bad argument"):
        sh.route(6, -1)
    assert hip_ops.SetRankShape.route is not None
