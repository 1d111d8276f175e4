"""The edge cases of tests/test_gpu_dlcm_edges.py and tests/test_gpu_gsf_edges.py (dlcm_ref.EDGES / FWD_ONLY, gsf_ref.EDGES), without a
GPU: the boundary arithmetic of csrc/ultr_dlcm_plan.h, csrc/ultr_gsf_plan.h, csrc/ultr_rowgrad_plan.h, csrc/ultr_gemm.h and csrc/ultr_sr_rows.hip restated in
Python, checked against the library's own size queries, and for every case the proof that it sits on the boundary it is named for - a
later change of a constant makes these tests say that a case has left its boundary.  Also the room the parity bar leaves: e32, the
float64 twin evaluated in float32 on the CPU, per case."""
import pytest

from tests import dlcm_ref as D
from tests import gsf_ref as G

# ---- the restatement ------------------------------------------------------------------------------------------------------------------
LDS_MAX = 160 * 1024      # DL_LDS_MAX; also the LDS of a compute unit
CUS = 256                 # compute units of an MI355X
LISTS = 16                # DL_LISTS
CS_ROWS = 256             # RG_CS_ROWS
WG_SPLITS = 64            # RG_WG_SPLITS
WG_FLOOR = 128            # rows per weight-gradient split at least
WIDE_FOLD = 256           # SrFoldQueue::add: nparts >= 256 takes the 16-column fold ...
WIDE2_LEN = 1024          # ... and partials this long its float4 form (out of scope here: SetRank's tests own it)
MAX_GROUP = 8             # GSF_MAX_GROUP


def ceil_div(a, b):
    return -(-a // b)


def up4(n):
    return (n + 3) & ~3


def cs_chunks(T):
    return ceil_div(T, CS_ROWS)


def wg_chunk(K):
    return max(WG_FLOOR, up4(ceil_div(K, WG_SPLITS)))


def wg_splits(K):
    return 0 if K <= 0 else ceil_div(K, wg_chunk(K))


def hp(H):
    return ceil_div(H, 16) * 16


def lds_fwd(H):
    return 2 * LISTS * (hp(H) + 8) * 4


def lds_bwd(H):
    """(bytes, dh_global): dg and dh in LDS while both fit, dg alone otherwise."""
    both = LISTS * ((3 * hp(H) + 8) + (hp(H) + 8)) * 4
    return (both, False) if both <= LDS_MAX else (LISTS * (3 * hp(H) + 8) * 4, True)


def ugemm(R, N, n_major):
    """ugemm::run's tile for N output columns and ugemm::launch's schedule for R rows: (BN, chunks, the most workgroups the GPU holds at
    once).  LDS per workgroup as Cfg<64, BN, 4, BN / 64, n_major>: two stages of an A tile [64][40] and a B tile ([BN][40] n-major,
    [32][BN] k-major), or the [64][BN + 4] output tile of the n-major epilogue."""
    BN = 128 if N > 64 else 64
    stage = 2 * (64 * 40 + (BN * 40 if n_major else 32 * BN))
    floats = max(stage, 64 * (BN + 4)) if n_major else stage
    per_cu = min(LDS_MAX // (4 * floats), 32 // (4 * (BN // 64)))
    chunks = ceil_div(ceil_div(R, 16), 4) * ceil_div(N, BN)
    return BN, chunks, per_cu * CUS


def dlcm_saved_floats(F, H, heads, n):
    """ultr_dlcm_saved_bytes / 4 at n rows (the query plans B = L = T = n: the bound for every B x L = n)."""
    return 2 * up4(n) + n * 3 * H + n * H + n * heads * H + n * H + n * F + n * 4 * H


def dlcm_ws_floats(B, L, F, H, heads, with_dh=True):
    T = B * L
    dh = ceil_div(B, LISTS) * LISTS * (hp(H) + 8) if with_dh and lds_bwd(H)[1] else 0
    return (2 * T * 3 * H + T * F + B * heads * H + B * H + up4(B * heads) + cs_chunks(T) * (6 * H + 2 * F) + cs_chunks(B) * heads * H +
            wg_splits(T) * 3 * H * F + wg_splits(T - 1) * 3 * H * H + dh)


def gsf_dims(F, m, hidden):
    dims, k = [], F * m
    for out in list(hidden) + [m]:
        dims.append((k, out))
        k = out
    return dims


def gsf_saved_floats(F, m, hidden, T):
    dims = gsf_dims(F, m, hidden)
    return T * MAX_GROUP + len(dims) * 2 * up4(T) + sum(T * out for _, out in dims[:-1]) + up4(T * m) + T * dims[0][0]


def gsf_ws_floats(B, L, F, m, hidden):
    T, dims = B * L, gsf_dims(F, m, hidden)
    n = up4(T * m) + sum(T * out for _, out in dims[:-1]) + T * max(k for k, _ in dims)
    for k, out in dims:
        n += up4(cs_chunks(T) * (out + 2 * k)) + up4(wg_splits(T) * out * k)
    return n


# ---- the restatement against the library ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.EDGES) + list(D.FWD_ONLY))
def test_dlcm_restatement_is_the_librarys_size_queries(name):
    from ultra_pytorch_amd import hip_ops
    B, L, F, H, heads = {**D.EDGES, **D.FWD_ONLY}[name]
    shape = hip_ops.DlcmShape(F, H, heads)
    assert shape.workspace_bytes(B, L) == 4 * dlcm_ws_floats(B, L, F, H, heads)
    assert shape.saved_bytes(B * L) == 4 * dlcm_saved_floats(F, H, heads, B * L)
    # single quantities as differences of the query: four more features give the token splits of dW_ih, one more head the row chunks of
    # dM's column sums, and what the restatement without the carried dh leaves over is that buffer
    T = B * L
    dF = (hip_ops.DlcmShape(F + 4, H, heads).workspace_bytes(B, L) - shape.workspace_bytes(B, L)) // 4
    assert dF - 4 * T - 8 * cs_chunks(T) == wg_splits(T) * 3 * H * 4
    dh = (hip_ops.DlcmShape(F, H, heads + 1).workspace_bytes(B, L) - shape.workspace_bytes(B, L)) // 4
    assert dh - B * H - (up4(B * (heads + 1)) - up4(B * heads)) == cs_chunks(B) * H
    carried = shape.workspace_bytes(B, L) // 4 - dlcm_ws_floats(B, L, F, H, heads, with_dh=False)
    assert carried == (ceil_div(B, LISTS) * LISTS * (hp(H) + 8) if H >= 628 else 0)


def test_dlcm_chunk_arithmetic_leaves_its_floor_where_the_header_says():
    assert wg_chunk(8192) == 128 and wg_splits(8192) == 64 and wg_chunk(8193) == 132      # past 64 x 128 tokens the chunk grows
    assert wg_splits(128) == 1 and wg_splits(129) == 2 and wg_splits(0) == 0
    assert cs_chunks(256) == 1 and cs_chunks(257) == 2
    assert all(wg_splits(K) <= WG_SPLITS and wg_chunk(K) % 4 == 0 for K in (1, 127, 8191, 8580, 75899, 75900, 10 ** 7))


@pytest.mark.parametrize("name", list(G.EDGES))
def test_gsf_restatement_is_the_librarys_size_queries(name):
    from ultra_pytorch_amd import hip_ops
    B, L, F, m, hidden, act = G.EDGES[name]
    shape = hip_ops.GsfShape(F, hidden, act, m)
    assert shape.workspace_bytes(B, L) == 4 * gsf_ws_floats(B, L, F, m, hidden)
    assert shape.saved_bytes(B * L) == 4 * gsf_saved_floats(F, m, hidden, B * L)


def test_lds_limits_are_the_ones_the_header_promises():
    """include/ultr_hip.h: hidden_size <= 848 trains, the forward runs up to 1264; dh leaves the LDS at Hp = 640."""
    assert lds_bwd(624) == (160768, False) and lds_bwd(640)[1] and lds_bwd(636)[1] and hp(636) == 640
    assert lds_bwd(848) == (163328, True) and lds_bwd(852)[0] > LDS_MAX
    assert lds_fwd(852) <= LDS_MAX and lds_fwd(1264) == 162816 and lds_fwd(1268) > LDS_MAX
    assert max(H for H in range(4, 2000, 4) if not lds_bwd(H)[1]) == 624
    assert max(H for H in range(4, 2000, 4) if lds_bwd(H)[0] <= LDS_MAX) == 848
    assert max(H for H in range(4, 2000, 4) if lds_fwd(H) <= LDS_MAX) == 1264
    # no instance of the persistent product holds more than 1024 workgroups at once
    assert max(ugemm(1, N, nm)[2] for N in (64, 65) for nm in (False, True)) <= 1024


# ---- every case on its boundary -------------------------------------------------------------------------------------------------------
def test_dlcm_cases_sit_on_their_boundaries():
    E = D.EDGES
    B, L, F, H, heads = E["tile-exact"]
    assert B == LISTS and heads == 1
    B, L, F, H, heads = E["tile+1"]
    assert B == LISTS + 1 and heads == 4
    B, L, F, H, heads = E["many-lists"]
    T = B * L
    assert T > WG_FLOOR * WG_SPLITS and wg_chunk(T) == wg_chunk(T - 1) == 136 and wg_chunk(T - 1) % L != 0
    assert wg_splits(T) == wg_splits(T - 1) == WG_SPLITS
    assert cs_chunks(B) == 2 and B >= WIDE_FOLD and heads < WIDE2_LEN            # dM's column sums in two chunks; dv's fold is wide
    assert heads > 4 and up4(B * heads) == B * heads                             # a second trip of the head backward's loop over heads
    assert cs_chunks(T) < WIDE_FOLD                                              # (the column-sum folds stay narrow here)
    B, L, F, H, heads = E["lds-max-resident"]
    assert lds_bwd(H) == (160768, False) and lds_bwd(H + 4)[1]
    B, L, F, H, heads = E["dh-global-first"]
    assert lds_bwd(H)[1] and not lds_bwd(H - 16)[1] and hp(H) == H and ceil_div(B, LISTS) == 3 and B % LISTS != 0
    B, L, F, H, heads = E["dh-global-ragged"]
    assert lds_bwd(H)[1] and hp(H) == 640 and H % 16 != 0 and ceil_div(B, LISTS) == 2 and heads == 1
    B, L, F, H, heads = E["bwd-max"]
    assert lds_bwd(H)[0] <= LDS_MAX < lds_bwd(H + 4)[0]
    for name, edge in (("fwd-only-852", 848), ("fwd-only-1264", 1264)):
        B, L, F, H, heads = D.FWD_ONLY[name]
        assert lds_bwd(H)[0] > LDS_MAX and lds_fwd(H) <= LDS_MAX and (H == edge + 4 or H == edge)
    assert lds_fwd(D.FWD_ONLY["fwd-only-1264"][3] + 4) > LDS_MAX
    assert E["saturated"] == D.SHAPES[0] and D.GRU_SCALE["saturated"] == 8.0
    B, L, F, H, heads = E["long"]
    T = B * L
    bn, chunks, slots = ugemm(T, 3 * H, True)                                    # gi: the gathering LayerNorm producer
    assert (bn, chunks) == (128, 1186) and chunks > 1024 >= slots
    bn, chunks, slots = ugemm(T, F, False)                                       # d xh
    assert (bn, chunks) == (64, 1186) and chunks > 1024 >= slots
    assert cs_chunks(T) == 297 and cs_chunks(T) >= WIDE_FOLD and 3 * H < WIDE2_LEN
    assert wg_chunk(T) == wg_chunk(T - 1) == 1188 and wg_chunk(T - 1) % L == 0 and cs_chunks(B) == 9 and B >= WIDE_FOLD
    # the largest call of the earlier suite never walked a second chunk
    assert max(ugemm(b * l, 3 * h, True)[1] for b, l, f, h, _ in D.ALL_SHAPES) <= 24


def test_gsf_cases_sit_on_their_boundaries():
    E = G.EDGES
    acts = {(E[n][5], E[n][:5] == G.SHAPES[4]) for n in E if n.startswith("act-") and n != G.NO_HIDDEN_EDGE}
    assert acts == {(a, wide) for a in ("relu", "tanh", "sigmoid") for wide in (False, True)}
    assert ugemm(1, G.SHAPES[0][4][0], True)[0] == 64 and ugemm(1, G.SHAPES[4][4][0], True)[0] == 128   # both tile widths
    assert E[G.NO_HIDDEN_EDGE][4] == [] and E[G.NO_HIDDEN_EDGE][5] != "elu"
    assert [E["slots-%d" % m][3] for m in (5, 6, 7)] == [5, 6, 7] and E["slots-6"][3] > E["slots-6"][1]  # m > L: the wrap
    assert {E["slots-%d" % m][5] for m in (5, 6, 7)} == {"elu", "relu", "tanh"}
    B, L, F, m, hidden, act = E["wide-N-walk"]
    T = B * L
    bn, chunks, slots = ugemm(T, hidden[0], True)
    assert (bn, chunks) == (128, 1088) and chunks > 1024 >= slots
    assert wg_chunk(T) == 272 and wg_splits(T) == WG_SPLITS and cs_chunks(T) < WIDE_FOLD
    B, L, F, m, hidden, act = E["long"]
    T = B * L
    bn, chunks, slots = ugemm(T, hidden[0], True)                                # AGroupLN
    assert (bn, chunks) == (64, 1186) and chunks > 1024 >= slots
    bn, chunks, slots = ugemm(T, hidden[1], True)                                # ALayerNorm without ids
    assert (bn, chunks) == (64, 1186) and chunks > 1024 >= slots
    assert cs_chunks(T) == 297 and cs_chunks(T) >= WIDE_FOLD and max(F * m, *hidden) < WIDE2_LEN and wg_chunk(T) == 1188
    assert max(ugemm(b * l, h[0], True)[1] for b, l, f, mm, h in G.SHAPES if h) <= 24


# ---- the room under the bar -----------------------------------------------------------------------------------------------------------
LONG_CAP = 4e-5  # no widened bar may reach this: the rule must not hide a real error


def check_room(tag, e32, long_case):
    worst = max(e32.values())
    print("%s: e32 (twin float32 vs float64) %.3g; %s" % (tag, worst, ", ".join("%s %.2g" % kv for kv in e32.items())))
    if long_case:
        assert max(1e-5, 4.0 * worst) < LONG_CAP, (tag, e32)
    else:
        assert worst <= 1e-5, (tag, e32)


@pytest.mark.parametrize("name", list(D.EDGES) + list(D.FWD_ONLY))
def test_dlcm_twin_float32_against_float64(name):
    assert D.BAR == 1e-5
    e32 = D.edge_case(name)[6]
    if name in D.FWD_ONLY:
        e32 = {"scores": e32["scores"]}
    check_room("DLCM " + name, e32, name in D.LONG_EDGES)


def test_dlcm_saturated_case_saturates():
    """gru.* x 8: in float32 some update / reset gates are exactly 1 (their derivative z (1 - z) is 0) and some candidate states exactly
    +-1.  (expf(-x) itself overflows only past |x| = 88; the gate inputs reach about 18 here.  Scales that reach it - x 48 and more -
    put the float32 twin 4e-5 .. 5e-3 from float64: such a case would measure the data, not the kernel.)"""
    import torch
    model, feats, ids, _, _, _, _ = D.edge_case("saturated")
    B, L, F, H, heads = D.EDGES["saturated"]
    tw = D.twin_from(model.state_dict(), F, H, heads, torch.float32)
    with torch.no_grad():
        xh = tw.layer_norm(D.gather(feats, ids, torch.float32))
        out, _ = tw.gru(torch.flip(xh, dims=[1]))
        o = torch.flip(out, dims=[1])
        hprev = torch.cat([o[:, 1:], torch.zeros(B, 1, H)], dim=1)
        gi = xh @ tw.gru.weight_ih_l0.T + tw.gru.bias_ih_l0
        gh = hprev @ tw.gru.weight_hh_l0.T + tw.gru.bias_hh_l0
        gates = torch.sigmoid((gi + gh)[..., :2 * H])
        n = torch.tanh(gi[..., 2 * H:] + gates[..., :H] * gh[..., 2 * H:])
    assert int((gates == 1.0).sum()) > 0 and float(gates.min()) < 1e-7 and int((n.abs() == 1.0).sum()) > 0


@pytest.mark.parametrize("name,permuted", G.EDGE_RUNS, ids=["%s-%s" % (n, "perm" if pm else "identity") for n, pm in G.EDGE_RUNS])
def test_gsf_twin_float32_against_float64(name, permuted):
    assert G.BAR == 1e-5
    check_room("GSF %s %s" % (name, "perm" if permuted else "identity"), G.edge_case(name, permuted)[7], name == "long")
