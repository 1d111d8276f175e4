"""ULTR_OPT_ADAM in the update launch (csrc/ultr_update.hip) against float64 Adam (tests/adam_ref.py: step64, which
tests/test_adam_cpu.py holds to torch.optim.Adam), teacher-forced: every step starts from the GPU's own float32 parameters and
moments and is fed the float32 gradient, sum of squares and step tail the GPU itself used - synthetic gradients through
ultr_grad_sumsq + ultr_apply_update.  A sign flip of a tiny gradient therefore cannot pass for an optimizer error, nor hide one.

The bar: the float32 rounding floor was measured on these very inputs (adam_ref.step32 against step64, on the CPU:
test_adam_cpu.py::test_float32_floor_is_the_recorded_one) at 5.35e-7 of max(|p|, lr); the GPU gets four times the recorded 5.4e-7,
BAR = 2.16e-6, under the project's 1e-5 parity bar.  The moments are held at 4 x their own floor of 4.0e-7 (MOMENT_RTOL = 1.6e-6),
relative to max(|m'|, |m|, the terms the step adds).

flat-*: the flat kernel (d == NULL), P in {1, 255, 257, 1000}, t = 1, 2, 3 from zero moments and single steps at t = 1000, 10^5, 2^31
from non-zero ones, clip off / biting, l2_loss 0 / 0.01, algorithms softmax, DLA (aux and its moments), PairDebias (aux as with
Adagrad, bit for bit), PDGD.  tiled-*: the DNN kernel that keeps the weight copies, on the three models of
test_gpu_edges.py::test_update_kernel_keeps_every_weight_copy_current."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import adam_ref as A  # noqa: E402

ALGO_ID = {"softmax": 0, "dla": 1, "pairdebias": 2, "pdgd": 6}


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def make_udesc(hyper, P, L, optimizer):
    from ultra_pytorch_amd import _lib
    u = _lib.UpdateDesc()
    u.algo, u.optimizer, u.list_size, u.n_params = ALGO_ID[hyper["algo"]], optimizer, L, P
    u.learning_rate, u.max_gradient_norm = hyper["learning_rate"], hyper["max_gradient_norm"]
    u.adagrad_eps = hyper["adagrad_eps"] if optimizer == _lib.OPT_ADAM else 1e-10
    u.ranker_loss_weight, u.propensity_learning_rate = hyper["ranker_loss_weight"], hyper["propensity_learning_rate"]
    u.em_step_size, u.regulation_p, u.l2_loss = hyper["em_step_size"], hyper["regulation_p"], hyper["l2_loss"]
    return u


class Launch:
    """One update launch on synthetic gradients: grads [P | tail], the sum-of-squares partials of ultr_grad_sumsq, 16 scalars.
    shape = None: the flat kernel (d == NULL, wt == NULL); a DnnShape: the tiled kernel with the model's weight copies."""

    def __init__(self, P, L, shape=None, rows=0):
        from ultra_pytorch_amd import _lib, hip_ops
        self.P, self.L, self.shape, self.lib = P, L, shape, _lib.load()
        tail = hip_ops.tail_floats(L)
        self.grads = torch.zeros(P + tail, device="cuda")
        n_ws = (P + tail + 63) // 64 + P // 4096 + 16
        if shape is not None:
            n_ws = max(n_ws, shape.bwd_workspace_bytes(rows) // 4)
        self.ws = torch.zeros(n_ws, device="cuda")
        self.sc = torch.zeros(16, device="cuda")

    def __call__(self, u, p, st, g, tail, aux):
        from ultra_pytorch_amd import _lib, hip_ops
        self.grads[:self.P].copy_(dev(g))
        self.grads[self.P:].copy_(dev(tail))
        hip_ops.grad_sumsq(self.grads, self.P, self.L, self.ws)
        if self.shape is not None:
            hip_ops.apply_update(self.shape, u, p, st, self.grads, aux, self.ws, self.sc)
        else:
            vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
            _lib.check(self.lib.ultr_apply_update(ctypes.byref(u), None, vp(p), None, vp(st), vp(self.grads), vp(aux), vp(self.ws),
                                                  vp(self.sc), hip_ops.raw_stream()), "ultr_apply_update")
        torch.cuda.synchronize()
        return self.sc.cpu().numpy()


def hold_step(case, t, before, after, g, tail, sc):
    """The launch's results against step64 from the GPU's own inputs and its own sum of squares (scalars[7])."""
    h, algo, P = case["hyper"], case["algo"], case["P"]
    p0, st0, aux0 = before
    p1, st1, aux1 = after
    ref_p, ref_st, ref_aux, terms = A.step64(p0, g, st0, t, h, tail, aux0 if algo == "dla" else None, ss=float(sc[7]))
    e = A.excess(p1, ref_p, h["learning_rate"])
    em = A.moment_excess(st1, ref_st, st0, terms)
    print("%s t=%d: parameters %.3e of max(|p|, lr) (bar %.3e), moments %.3e (bar %.3e)" % (case["name"], t, e, A.BAR, em, A.MOMENT_RTOL))
    assert e <= A.BAR, ("parameters", t, e)
    assert em <= A.MOMENT_RTOL, ("moments", t, em)
    if algo == "dla":
        ea = A.excess(aux1, ref_aux, h["propensity_learning_rate"], A.aux_cond(tail, aux0, h))
        print("%s t=%d: propensity parameters %.3e (bar %.3e)" % (case["name"], t, ea, A.BAR))
        assert ea <= A.BAR, ("aux", t, ea)
    # the clip: the restated coefficient, and exactly 1 where the clip is off or (l2_loss > 0, not DLA or PDGD) dropped
    want = A._scalars(p0, g, tail, float(sc[7]), h)["coef"]
    assert abs(float(sc[2]) - want) <= 1e-5, ("clip coefficient", float(sc[2]), want)
    if h["max_gradient_norm"] == 0 or (h["l2_loss"] > 0 and algo not in ("dla", "pdgd")):
        assert sc[2] == 1.0


def run_case(case, launch, after_step=None):
    from ultra_pytorch_amd import _lib
    h, algo, P, L = case["hyper"], case["algo"], case["P"], case["L"]
    u = make_udesc(h, P, L, _lib.OPT_ADAM)
    assert int(launch.lib.ultr_opt_state_floats(ctypes.byref(u))) == A.state_floats(algo, P, L)
    p, st = dev(case["p0"]), torch.zeros(A.state_floats(algo, P, L), device="cuda")
    aux = None if case["aux0"] is None else dev(case["aux0"])
    runs = [(t, g, tail, None) for t, g, tail in case["fresh"]] + list(case["warm"])
    host = lambda: (p.cpu().numpy(), st.cpu().numpy(), None if aux is None else aux.cpu().numpy())  # noqa: E731
    for t, g, tail, st_in in runs:
        if st_in is not None:
            p.copy_(dev(case["p0"]))
            st.copy_(dev(st_in))
            if aux is not None:
                aux.copy_(dev(case["aux0"]))
        before = host()
        u.adam_t = t
        sc = launch(u, p, st, g, tail, aux)
        after = host()
        hold_step(case, t, before, after, g, tail, sc)
        if algo == "pairdebias":
            # the EM update of t_plus / t_minus does not pass through an optimizer: the same bits as an Adagrad launch gives
            ua = make_udesc(h, P, L, _lib.OPT_ADAGRAD)
            p2, s2, aux2 = dev(before[0]), torch.full((P,), 0.1, device="cuda"), dev(before[2])
            launch(ua, p2, s2, g, tail, aux2)
            assert np.array_equal(aux2.cpu().numpy().view(np.uint32), after[2].view(np.uint32))
            assert not np.array_equal(after[2], before[2])
        if after_step is not None:
            after_step(p)
        if st_in is None and t == 3 and h["l2_loss"] == 0:
            # an exact 0 gradient on v = 0, three steps running: the parameter keeps its bits, the moments stay 0
            zm = case["zero_mask"]
            assert np.isfinite(after[0]).all() and np.array_equal(after[0][zm].view(np.uint32), case["p0"][zm].view(np.uint32))
            assert not after[1][:P][zm].any() and not after[1][P:2 * P][zm].any()
            assert (after[0][~zm] != case["p0"][~zm]).all()


@pytest.mark.parametrize("name", list(A.flat_cases()))
def test_flat_kernel_holds_float64_adam(name):
    case = A.flat_cases()[name]
    run_case(case, Launch(case["P"], case["L"]))


@pytest.mark.parametrize("name", list(A.tiled_cases()))
def test_tiled_kernel_holds_float64_adam_and_keeps_every_weight_copy_current(name):
    """After every Adam update the k-major copy, the packed image, the fragment-major and the split-half copies equal a fresh
    ultr_dnn_build_wt of the new parameters, bitwise; the parameters and moments hold the bars."""
    from ultra_pytorch_amd import _lib, hip_ops
    case = A.tiled_cases()[name]
    shape = hip_ops.DnnShape(A.TILED_F, case["hidden"], "elu")
    assert shape.n_params == case["P"]

    def copies_are_current(p):
        kept = hip_ops.weight_copy(shape).wt
        fresh = torch.zeros_like(kept)
        _lib.check(shape.lib.ultr_dnn_build_wt(ctypes.byref(shape.desc), ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(fresh.data_ptr()),
                                               hip_ops.raw_stream()), "ultr_dnn_build_wt")
        torch.cuda.synchronize()
        assert kept.numel() > shape.n_params
        diff = (kept.view(torch.int32) != fresh.view(torch.int32)).nonzero().flatten()
        assert diff.numel() == 0, (diff[:8].tolist(), diff.numel(), kept.numel())

    run_case(case, Launch(case["P"], case["L"], shape=shape, rows=A.TILED_B * A.TILED_L), after_step=copies_are_current)


@pytest.mark.parametrize("tiled", [False, True])
def test_guard_word_leaves_parameters_moments_and_aux_untouched(tiled):
    """A non-zero guard word (a refused data-parallel step): parameters, m, v, DLA's aux and its moments keep their bits; the same
    launch with the word cleared moves all of them."""
    from ultra_pytorch_amd import _lib, hip_ops
    if tiled:
        case = dict(A.tiled_cases()["tiled-256x64"])
        shape = hip_ops.DnnShape(A.TILED_F, case["hidden"], "elu")
        case.update(algo="dla", hyper=A.adam_hyper("dla", max_gradient_norm=5.0), aux0=A.make_aux(np.random.RandomState(5), "dla", case["L"]))
        launch = Launch(case["P"], case["L"], shape=shape, rows=A.TILED_B * A.TILED_L)
    else:
        case = A.flat_cases()["flat-dla-P1000-clip0.05-l20"]
        launch = Launch(case["P"], case["L"])
    P, L = case["P"], case["L"]
    rng = np.random.RandomState(11)
    u = make_udesc(case["hyper"], P, L, _lib.OPT_ADAM)
    u.adam_t = 4
    n = A.state_floats("dla", P, L)
    st0 = np.concatenate([rng.uniform(-0.01, 0.01, size=P), rng.uniform(1e-6, 1e-3, size=P), rng.uniform(-0.01, 0.01, size=L + 1),
                          rng.uniform(1e-6, 1e-3, size=L + 1)]).astype(np.float32)
    assert len(st0) == n
    p, st, aux = dev(case["p0"]), dev(st0), dev(case["aux0"])
    g, tail = A.make_grad(rng, P)[0], A.make_tail(rng, "dla", L)
    guard = torch.ones(1, dtype=torch.int32, device="cuda")
    u.guard = guard.data_ptr()
    launch(u, p, st, g, tail, aux)
    for got, want in ((p, case["p0"]), (st, st0), (aux, case["aux0"])):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    guard.zero_()
    launch(u, p, st, g, tail, aux)
    moved = g != 0
    assert (p.cpu().numpy()[moved] != case["p0"][moved]).all()
    s1 = st.cpu().numpy()
    # (a moment may round back to its old bits where its increment is below half an ulp: most move, not all)
    assert (s1[:P][moved] != st0[:P][moved]).mean() > 0.9 and (s1[P:2 * P][moved] != st0[P:2 * P][moved]).mean() > 0.9
    assert (s1[2 * P:] != st0[2 * P:]).any() and (aux.cpu().numpy() != case["aux0"]).any()
