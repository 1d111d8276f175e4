"""tests/dnn_ref.py - the float64 restatement the operand tests and the ReLU sweep cases are held to - checked on the host, and the
route query with operand facts (ultr_dnn_route_operands) pinned.  No GPU.

1. The restatement's closed-form gradients against float64 central differences (all four activations).
2. The fp32 oracle (oracle.ultr_oracle) against the restatement on every case of tests/test_gpu_dnn_operands.py: within ONE THIRD of
   the bars the GPU is held to, so that a GPU result inside its bar of the restatement cannot owe that to the oracle's own error.
3. What clearing an operand bit does to the route, over those shapes and the planner sweep's 75."""
import numpy as np
import pytest

from tests import dnn_operand_cases as C
from tests import dnn_ref as R


@pytest.mark.parametrize("act", R.ACTS)
def test_gradients_match_central_differences(act):
    F, hidden, N = 5, [4, 3], 7
    rng = np.random.RandomState(11)
    _, P = R.layout(F, hidden)
    params = rng.normal(scale=0.5, size=P)
    lay, _ = R.layout(F, hidden)
    for (og, _, _, _), (k, _) in zip(lay, R.layer_dims(F, hidden)):  # LayerNorm weights around 1
        params[og:og + k] += 1.0
    x = rng.uniform(-1, 1, size=(N, F))
    dscore = rng.normal(size=N)
    if act == "relu":  # central differences need every pre-activation further than the step from its kink
        z = np.concatenate([a.reshape(-1) for a in R.forward(params, F, hidden, x, act)["z"]])
        assert np.abs(z).min() > 1e-4, float(np.abs(z).min())
    g, terms = R.backward(params, F, hidden, x, dscore, act)
    fd = R.central_differences(params, F, hidden, x, dscore, act, h=1e-6)
    assert (terms >= np.abs(g) * (1 - 1e-12)).all()
    rel = np.abs(g - fd).max() / np.abs(fd).max()
    assert rel <= 1e-6, rel


def test_restatement_agrees_with_the_oracles_own_walks():
    """The same layout, the same LayerNorm epsilon and the same sums of |terms| as oracle.ultr_oracle (abs_terms=True is float64 there)."""
    from oracle import ultr_oracle as O
    assert R.LN_EPS == O.LN_EPS
    d, ref = C.inputs(1), C.reference(1)
    assert R.layout(d["F"], d["hidden"])[1] == O.num_params(d["F"], d["hidden"])
    x32 = O.gather_rows(d["feats"], d["ids"]).numpy()
    np.testing.assert_array_equal(x32.astype(np.float64), ref["x"])
    dsc = (ref["dscores"].T.reshape(-1)).astype(np.float32)
    terms = O.dnn_backward_manual(d["params"], d["F"], d["hidden"], x32, dsc, d["act"], abs_terms=True)
    _, mine = R.backward(d["params"], d["F"], d["hidden"], ref["x"], dsc, d["act"], fwd=ref["fwd"])
    np.testing.assert_allclose(mine, terms, rtol=1e-12, atol=0)


@pytest.mark.parametrize("k", range(len(C.CASES)), ids=[C.case_id(c) for c in C.CASES])
def test_oracle_is_within_a_third_of_the_gpu_bars(k):
    from oracle import ultr_oracle as O
    d, ref = C.inputs(k), C.reference(k)
    F, hidden, act = d["F"], d["hidden"], d["act"]
    o = O.train_step_softmax(d["params"], np.zeros_like(d["params"]), F, hidden, d["feats"], d["ids"].astype(np.int64), d["y"], ipw_list=C.IPW,
                             act=act)
    rs, rl, rg = C.score_ratio(o["scores"], ref["scores"]), C.loss_ratio(o["loss"], ref["loss"]), C.grad_ratio(o["grads"], ref["grads"], ref["terms"])
    print("case %s: oracle / bar  scores %.3f  loss %.3f  grads %.3f  (rows redrawn %.1f%%)" % (C.case_id(C.CASES[k]), rs, rl, rg, 100 * d["redrawn"]))
    assert rs <= 1 / 3 and rl <= 1 / 3 and rg <= 1 / 3, (rs, rl, rg)
    # the closed-form backward in fp32 (the written-out spec of the kernels) at the reference's dscores, too
    x32 = O.gather_rows(d["feats"], d["ids"]).numpy()
    gm = O.dnn_backward_manual(d["params"], F, hidden, x32, ref["dscores"].T.reshape(-1).astype(np.float32), act)
    assert C.grad_ratio(gm, ref["grads"], ref["terms"]) <= 1 / 3


def test_relu_conditioning_leaves_no_unit_near_zero():
    k = [i for i, c in enumerate(C.CASES) if c[1] == "relu"][0]
    d, ref = C.inputs(k), C.reference(k)
    assert not R.near_zero_rows(d["params"], d["F"], d["hidden"], ref["x"], "relu").any()
    # and it does find them: a pre-activation put exactly on zero through the bias
    p = d["params"].astype(np.float64).copy()
    lay, _ = R.layout(d["F"], d["hidden"])
    p[lay[0][3]] -= ref["fwd"]["z"][0][3, 0]
    assert R.near_zero_rows(p, d["F"], d["hidden"], ref["x"], "relu")[3]


# ---- the route query with operand facts ------------------------------------------------------------------------------------------
def _shapes():
    from tests.test_gpu_planner_sweep import CASES as SWEEP
    out = [(F, tuple(h), B, L, "elu") for F, h, B, L in C.SHAPES]
    out += [(c["F"], tuple(c["hidden"]), c["B"], c["L"], c["act"]) for c in SWEEP]
    return out


def _route(shape, B, L, call, clear=()):
    from ultra_pytorch_amd import _lib
    r = shape.route(B, L, call=call, operands=[n for n in _lib.DNN_OPERANDS if n not in clear])
    return dict(r, fwd=_lib.DNN_FAMILIES[r["fwd"]], bwd=_lib.DNN_FAMILIES[r["bwd"]], loss=_lib.DNN_LOSS_PLACES[r["loss"]])


def test_route_operands_is_pinned():
    from ultra_pytorch_amd import _lib, hip_ops
    assert len(_shapes()) == len(C.SHAPES) + 75
    seen = {"fused_lost": 0, "wide_lost": 0, "prologue": 0}
    for F, hidden, B, L, act in _shapes():
        shape = hip_ops.DnnShape(F, list(hidden), act)
        for call in ("step_softmax", "step_dscores", "eval"):
            try:
                full = _route(shape, B, L, call)
            except _lib.UltrHipError:
                continue  # (a shape the call refuses with every operand aligned)
            # ultr_dnn_route is the all-bits case
            assert full == dict(shape.route(B, L, call=call), fwd=full["fwd"], bwd=full["bwd"], loss=full["loss"])
            assert shape.route(B, L, call=call, operands=_lib.DNN_OP_ALL) == shape.route(B, L, call=call)
            for bit in ("params16", "features16"):
                r = _route(shape, B, L, call, clear=(bit,))
                assert r["fused_waves"] == 0 and r["fwd"] == "tile" and r["wg_split_half"] == 0, (F, hidden, B, L, call, bit, r)
                assert r["bwd"] == ("none" if call == "eval" else "tile"), (F, hidden, B, L, call, bit, r)
            for bit in ("wt", "wt16"):
                r = _route(shape, B, L, call, clear=(bit,))
                if hidden:
                    assert r["fused_waves"] == 0 and r["fwd"] == "tile" and r["bwd"] != "wide", (F, hidden, B, L, call, bit, r)
                    seen["fused_lost"] += full["fused_waves"] != 0
                    seen["wide_lost"] += full["bwd"] == "wide"
                else:  # a one-Linear model has no copies to read: it keeps its aligned route
                    assert r == full, (F, hidden, B, L, call, bit, r, full)
            # a copy off a 16-byte boundary counts as absent: one route for the three ways to say so
            assert _route(shape, B, L, call, clear=("wt",)) == _route(shape, B, L, call, clear=("wt16",)) == _route(shape, B, L, call, clear=("wt", "wt16"))
            if call == "step_softmax":
                r = _route(shape, B, L, call, clear=("dscores",))
                if r["fused_waves"] == 0:  # (the fused launch keeps the loss to itself with or without a dscores buffer)
                    assert r["bwd"] in ("tile", "tile2") and r["loss"] == "prologue", (F, hidden, B, L, r)
                    seen["prologue"] += full["loss"] == "launch"
                else:
                    assert r == full
    assert all(v > 0 for v in seen.values()), seen  # every rule above changed some route


def test_route_operands_refuses_unknown_bits():
    import ctypes
    from ultra_pytorch_amd import _lib, hip_ops
    shape = hip_ops.DnnShape(24, [32], "elu")
    info = _lib.DnnRouteInfo()
    assert shape.lib.ultr_dnn_route_operands(ctypes.byref(shape.desc), 5, 7, 35, 1, 32, ctypes.byref(info)) == -1
    with pytest.raises(KeyError):
        shape.route(5, 7, operands=["wt32"])


def test_misaligned_weight_copy_is_refused_on_the_host():
    """ultr_apply_update and ultr_train_step must write the copies: one off a 16-byte boundary is ULTR_E_BADARG before anything is
    launched (the check precedes every other look at the arguments, so it is reachable without a device)."""
    import ctypes
    from ultra_pytorch_amd import _lib, hip_ops
    shape = hip_ops.DnnShape(24, [32], "elu")
    lib = shape.lib
    u = _lib.UpdateDesc()
    u.algo, u.optimizer, u.list_size, u.n_params, u.learning_rate = _lib.ALGO_SOFTMAX, _lib.OPT_ADAGRAD, 7, shape.n_params, 0.05
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    a = _lib.StepArgs()
    a.desc, a.upd, a.wt = ctypes.pointer(shape.desc), ctypes.pointer(u), base + 4
    assert lib.ultr_train_step(ctypes.byref(a), None) == -1
    assert lib.ultr_apply_update(ctypes.byref(u), ctypes.byref(shape.desc), base, base + 4, base, base, None, base, base, None) == -1
