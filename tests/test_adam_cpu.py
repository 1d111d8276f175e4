"""ULTR_OPT_ADAM without a GPU: the state query, the refusals (before anything is launched), the unchanged ABI, the optimizer
mappings, tests/adam_ref.py against torch.optim.Adam in float64, and the float32 rounding floor the GPU bar is derived from."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1


def _lib():
    from ultra_pytorch_amd import _lib as L, build
    build.build_library()
    return L, L.load()


def _udesc(L, algo, opt, list_size=10, n_params=100, t=1):
    u = L.UpdateDesc()
    u.algo, u.optimizer, u.list_size, u.n_params, u.adam_t = algo, opt, list_size, n_params, t
    u.learning_rate, u.max_gradient_norm, u.adagrad_eps = 0.05, 5.0, 1e-8
    return u


def test_state_query_gives_the_documented_sizes():
    L, lib = _lib()
    assert hasattr(lib, "ultr_opt_state_floats") and "ultr_opt_state_floats" in L.SIGNATURES
    assert (L.OPT_ADAGRAD, L.OPT_SGD, L.OPT_ADAM) == (0, 1, 2)
    q = lambda *a, **k: int(lib.ultr_opt_state_floats(ctypes.byref(_udesc(L, *a, **k))))  # noqa: E731
    for algo in range(8):
        assert q(algo, L.OPT_SGD) == 0
        assert q(algo, L.OPT_ADAGRAD) == 100
        assert q(algo, L.OPT_ADAM) == (200 + 2 * 11 if algo == L.ALGO_DLA else 200)
    assert q(L.ALGO_DLA, L.OPT_ADAM, list_size=1, n_params=1) == 2 + 4
    assert q(L.ALGO_SOFTMAX, L.OPT_ADAM, n_params=2 ** 33) == 2 ** 34  # 64-bit
    for bad in (dict(algo=8), dict(algo=-1), dict(opt=3), dict(opt=-1), dict(list_size=0), dict(n_params=0)):
        kw = dict(algo=L.ALGO_SOFTMAX, opt=L.OPT_ADAM)
        kw.update(bad)
        assert q(**kw) == -1, bad
    assert int(lib.ultr_opt_state_floats(None)) == -1
    from ultra_pytorch_amd import engine
    assert engine.opt_state_floats("dla", "adam", 10, 100) == 222
    assert engine.opt_state_floats("softmax", "adam", 10, 100) == 200
    assert engine.opt_state_floats("softmax", "ada", 10, 100) == engine.opt_state_floats("softmax", "anything", 10, 100) == 100
    assert engine.opt_state_floats("pdgd", "sgd", 10, 100) == 0


def test_abi_is_still_8_and_the_descriptor_keeps_its_layout():
    L, lib = _lib()
    assert int(lib.ultr_abi_version()) == L.ABI_VERSION == 8
    header = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    assert "#define ULTR_ABI_VERSION 8" in header
    assert "ULTR_OPT_ADAM = 2" in header and "#define ULTR_ADAM_BETA1 0.9" in header and "#define ULTR_ADAM_BETA2 0.999" in header
    assert "#define ULTR_ADAM_EPS 1e-8" in header
    assert (L.ADAM_BETA1, L.ADAM_BETA2, L.ADAM_EPS) == (A.B1, A.B2, A.EPS) == (0.9, 0.999, 1e-8)
    U = L.UpdateDesc
    assert ctypes.sizeof(U) == 88
    assert U.seq.offset == 72 and U.adam_t.offset == 76 and U.adam_t.size == 4 and U.range_flag.offset == 80  # t sits in the old pad


def _host_buffers(n=256):
    bufs = [np.full(n, 7.0, np.float32) for _ in range(6)]
    return bufs, [b.ctypes.data for b in bufs]


@pytest.mark.parametrize("what", ["adam-null-state", "adam-t0", "opt3", "opt-1"])
def test_update_refuses_before_anything_is_launched(what):
    """ultr_apply_update and ultr_train_step: Adam without state, Adam with t = 0 and an optimizer outside the enum are
    ULTR_E_BADARG from the host-side checks - the buffers here are plain host memory, which no launch could have taken."""
    L, lib = _lib()
    opt = {"opt3": 3, "opt-1": -1}.get(what, L.OPT_ADAM)
    u = _udesc(L, L.ALGO_SOFTMAX, opt, list_size=3, n_params=64, t=0 if what == "adam-t0" else 5)
    bufs, (params, state, grads, ws, scalars, other) = _host_buffers()
    st = None if what == "adam-null-state" else state
    rc = lib.ultr_apply_update(ctypes.byref(u), None, params, None, st, grads, None, ws, scalars, None)
    assert rc == BADARG, rc
    desc = L.make_desc(8, [4])
    a = L.StepArgs()
    a.desc, a.upd = ctypes.pointer(desc), ctypes.pointer(u)
    a.params, a.state, a.grads, a.bwd_ws, a.scalars = params, st, grads, ws, scalars
    a.features = a.docids = a.labels = a.scores = a.dscores = a.saved = a.loss_ws = other
    a.n_docs, a.batch, a.list_size = 4, 2, 3
    rc = lib.ultr_train_step(ctypes.byref(a), None)
    assert rc == BADARG, rc
    assert all((b == 7.0).all() for b in bufs)


def test_optimizer_mappings_know_adam():
    import inspect
    from ultra_pytorch_amd import _lib as L, engine
    from ultra_pytorch_amd.learning_algorithm import DBGD
    from ultra_pytorch_amd.learning_algorithm.base_algorithm import BaseAlgorithm
    assert engine.optimizer_id("adam") == L.OPT_ADAM == 2
    assert engine.optimizer_id("sgd") == L.OPT_SGD and engine.optimizer_id("ada") == L.OPT_ADAGRAD
    assert engine.optimizer_id("adagrad") == engine.optimizer_id("rmsprop") == L.OPT_ADAGRAD  # any other string: today's behaviour
    # the one-call engine and, through it, the staged engines (SetRank, DLCM, GSF) take their id and eps from it
    src = inspect.getsource(engine.StepEngine.__init__)
    assert "u.optimizer = optimizer_id(optimizer)" in src and "_lib.ADAM_EPS if u.optimizer == _lib.OPT_ADAM else 1e-10" in src
    for cls in (engine.StagedStepEngine, engine.SetRankStepEngine, engine.DlcmStepEngine, engine.GsfStepEngine):
        assert issubclass(cls, engine.StepEngine)
    # the algorithms hand grad_strategy through; DBGD / MGD / NSGD keep their two-way mapping
    algo = lambda gs: types.SimpleNamespace(hparams=types.SimpleNamespace(grad_strategy=gs))  # noqa: E731
    assert [BaseAlgorithm._optimizer(algo(g)) for g in ("adam", "sgd", "ada", "xyz")] == ["adam", "sgd", "ada", "ada"]
    assert [DBGD._optimizer(algo(g)) for g in ("adam", "sgd", "ada")] == ["ada", "sgd", "ada"]


def test_adam_ref_agrees_with_torch_adam_in_float64():
    """Five steps of adam64 against torch.optim.Adam(betas=(0.9, 0.999), eps=1e-8) on float64 tensors, from zero moments."""
    rng = np.random.RandomState(3)
    n, lr = 300, 0.05
    p = rng.uniform(-1, 1, size=n)
    tp = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
    opt = torch.optim.Adam([tp], lr=lr)
    assert opt.defaults["betas"] == (A.B1, A.B2) and opt.defaults["eps"] == A.EPS and not opt.defaults["amsgrad"]
    assert opt.defaults["weight_decay"] == 0
    m, v = np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = A.make_grad(rng, n)[0].astype(np.float64)
        tp.grad = torch.tensor(g)
        opt.step()
        p, m, v = A.adam64(p, g, m, v, t, lr, A.EPS)
        st = opt.state[tp]
        np.testing.assert_allclose(tp.detach().numpy(), p, rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(st["exp_avg"].numpy(), m, rtol=1e-13, atol=0)
        np.testing.assert_allclose(st["exp_avg_sq"].numpy(), v, rtol=1e-13, atol=0)


def test_step64_applies_adam_to_the_gradient_of_param_update():
    """step64 feeds Adam the gradient loss_ref.param_update feeds Adagrad / SGD (scale, l2 term, clip), and DLA's propensity
    gradient is the one loss_ref.tail_update steps with: both read back from an SGD step of rate 1."""
    for name in ("flat-dla-P257-clip0.05-l20.01", "flat-softmax-P1000-clip0.05-l20", "flat-pairdebias-P255-clip0-l20.01"):
        case = A.flat_cases()[name]
        algo, h = case["algo"], dict(case["hyper"])
        t, g, tail = case["fresh"][0]
        p, aux = case["p0"], case["aux0"]
        ss = float((g.astype(np.float64) ** 2).sum())
        sgd = dict(h, optimizer="sgd", learning_rate=1.0, propensity_learning_rate=1.0)
        g_ref = p.astype(np.float64) - R.param_update(p, g, None, ss, sgd, tail)[0]
        pn, st, an, _ = A.step64(p, g, np.zeros(A.state_floats(algo, case["P"], case["L"])), 1, h, tail, aux if algo == "dla" else None)
        np.testing.assert_allclose(st[:case["P"]], (1 - A.B1) * g_ref, rtol=1e-9, atol=1e-16)  # m after one step from 0
        if algo == "dla":
            a_ref = aux.astype(np.float64) - R.tail_update("dla", tail, aux, sgd, ss=ss, l2_sums=R.l2_sums_of(p, g))[0]
            np.testing.assert_allclose(st[2 * case["P"]:2 * case["P"] + case["L"] + 1], (1 - A.B1) * a_ref, rtol=1e-9, atol=1e-16)
            assert np.abs(a_ref).max() > 0


def _floor(cases):
    worst, worst_m, where = 0.0, 0.0, None
    for case in cases.values():
        lr, plr, P = case["hyper"]["learning_rate"], case["hyper"]["propensity_learning_rate"], case["P"]
        for t, got, ref, old in A.walk(case, A.step32):
            e = A.excess(got[0], ref[0], lr)
            if case["algo"] == "dla":
                e = max(e, A.excess(got[2], ref[2], plr))  # (one-signed sums: their condition number is 1)
            if e > worst:
                worst, where = e, (case["name"], t)
            worst_m = max(worst_m, A.moment_excess(got[1], ref[1], old, ref[3]))
    return worst, worst_m, where


def test_float32_floor_is_the_recorded_one():
    """The float32 restatement against the float64 one on the very inputs of the GPU tests: the largest deviation of a parameter,
    relative to max(|p|, lr), is the floor; the GPU bar is four times it and must stay under the project's 1e-5 parity bar."""
    flat, flat_m, w1 = _floor(A.flat_cases())
    tiled, tiled_m, w2 = _floor(A.tiled_cases())
    print("float32 floor: flat %.3e at %s, tiled %.3e at %s; moments %.3e / %.3e (relative)" % (flat, w1, tiled, w2, flat_m, tiled_m))
    floor = max(flat, tiled)
    assert floor <= A.FLOOR_MEASURED, (floor, A.FLOOR_MEASURED)
    assert floor >= 0.8 * A.FLOOR_MEASURED, "the recorded floor is stale: %.3e measured" % floor
    assert A.BAR == 4.0 * A.FLOOR_MEASURED and A.BAR <= 1e-5
    assert 0.8 * A.MOMENT_FLOOR_MEASURED <= max(flat_m, tiled_m) <= A.MOMENT_FLOOR_MEASURED
    assert A.MOMENT_RTOL == 4.0 * A.MOMENT_FLOOR_MEASURED <= 1e-5


def test_case_tables_cover_what_the_gpu_tests_claim():
    cases = A.flat_cases()
    assert len(cases) == 4 * 4 * 2 * 2 and {c["P"] for c in cases.values()} == {1, 255, 257, 1000}
    for c in list(cases.values()) + list(A.tiled_cases().values()):
        for t, g, tail in c["fresh"]:
            nz = np.abs(g[g != 0])
            assert (g[c["zero_mask"]] == 0).all() and (nz.size == 0 or (nz.min() >= 1e-3 and nz.max() <= 1.0))
        assert [w[0] for w in c["warm"]] == [1000, 10 ** 5, 2 ** 31]
        for _, g, _, st in c["warm"]:
            nz = np.abs(g[g != 0])
            assert nz.size == 0 or (nz.min() >= 1e-3 and nz.max() <= 1.0)
            assert np.abs(st).min() > 0
    assert any(c["zero_mask"].any() for c in cases.values())
    # the clip bites where it is on and the algorithm keeps it, and does not where it is off
    for name in ("flat-softmax-P1000-clip0.05-l20", "flat-dla-P257-clip0.05-l20.01", "flat-pdgd-P255-clip0.05-l20.01"):
        c = cases[name]
        t, g, tail = c["fresh"][0]
        assert A._scalars(c["p0"], g, tail, float((g.astype(np.float64) ** 2).sum()), c["hyper"])["coef"] < 1.0
    c = cases["flat-softmax-P1000-clip0.05-l20.01"]  # l2_loss > 0 switches the clip off for every algorithm but DLA and PDGD
    t, g, tail = c["fresh"][0]
    assert A._scalars(c["p0"], g, tail, float((g.astype(np.float64) ** 2).sum()), c["hyper"])["coef"] == 1.0
