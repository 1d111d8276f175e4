"""TwoTower without a GPU: the float64 twin (tests/twotower_ref.py) against the textbook expression and autograd, the tail's
additivity, the kernel's formulas restated in float32 against the twin at the GPU bar, the hyper-parameters, the optimizer-state
sizes, the C entry and its binding, and the exported propensity table."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import loss_ref as R
from tests import twotower_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBINATIONS = ("product", "sum")


def _inputs(n, bound, seed, fractional=True):
    rng = np.random.RandomState(seed)
    s = rng.uniform(-bound, bound, size=(n, 1))
    th = rng.uniform(-bound, bound, size=n)
    c = rng.choice([0.0, 1.0, 0.25, 0.5] if fractional else [0.0, 1.0], size=(n, 1))
    return s, th, c


@pytest.mark.parametrize("comb", COMBINATIONS)
def test_stable_form_is_the_textbook_expression_where_that_is_exact(comb):
    """|s|, |theta| <= 15: 1 - p keeps its digits in float64 and the naive expression is exact to 1e-9 (the sum form at half the
    range each: its logit is s + theta)."""
    s, th, c = _inputs(20000, 15.0 if comb == "product" else 7.5, 1)
    s, th, c = torch.tensor(s).view(1, -1), torch.tensor(th), torch.tensor(c).view(1, -1)  # element i pairs s_i with theta_i
    a, b = T.element_loss(s, th, c, comb), T.naive_element_loss(s, th, c, comb)
    assert torch.isfinite(a).all()
    assert float(((a - b).abs() / (1.0 + b.abs())).max()) <= 1e-9


@pytest.mark.parametrize("comb", COMBINATIONS)
def test_closed_form_gradients_are_autograds(comb):
    rng = np.random.RandomState(3)
    B, L = 50, 40
    s = torch.tensor(rng.uniform(-40, 40, size=(B, L)), requires_grad=True)
    th = torch.tensor(rng.uniform(-40, 40, size=L), requires_grad=True)
    c = torch.tensor(rng.choice([0.0, 1.0, 0.25, 0.5], size=(B, L)))
    T.element_loss(s, th, c, comb).sum().backward()
    gs, gt, a_s, a_t = T.closed_form_grads(s.detach(), th.detach(), c, comb)
    assert R.terms_excess(gs.numpy(), s.grad.numpy(), a_s.numpy()) <= 1e-12
    assert R.terms_excess(gt.sum(0).numpy(), th.grad.numpy(), a_t.sum(0).numpy()) <= 1e-12


@pytest.mark.parametrize("comb", COMBINATIONS)
def test_tail_of_a_batch_is_the_sum_of_its_halves(comb):
    s, th, y = T.make_case(65, 8.0, "fractional", B=6)
    ids = np.arange(6 * 65, dtype=np.int32).reshape(65, 6)
    ids[60:, 2] = 6 * 65  # PADs at the tail of one list
    whole = T.loss_parts(s, y, th, comb, ids, 6 * 65)
    a = T.loss_parts(s[:2], y[:, :2], th, comb, ids[:, :2], 6 * 65)
    b = T.loss_parts(s[2:], y[:, 2:], th, comb, ids[:, 2:], 6 * 65)
    assert R.terms_excess(a["tail"] + b["tail"], whole["tail"], whole["tail_abs"]) <= 1e-13
    assert a["tail"][1] + b["tail"][1] == whole["tail"][1] == 6.0
    assert np.array_equal(np.concatenate([a["ds"], b["ds"]]), whole["ds"])
    assert not whole["ds"][2, 60:].any() and whole["ds"][2, :60].all()


@pytest.mark.parametrize("comb", COMBINATIONS)
@pytest.mark.parametrize("bound", [8.0, 40.0, 110.0])
def test_float32_restatement_of_the_kernel_holds_the_gpu_bar(comb, bound):
    """2 x 10^5 random (s, theta, c): the kernel's formulas in numpy float32 against the twin, loss and both gradients, at TERMS_RTOL.
    40 is the range the forms were chosen on; 110 is past the underflow of exp(-x) in float32, where the common factor taken out of
    1 - p (csrc/ultr_twotower.hip) keeps log(1 - p) and the gradients finite."""
    n = 200000
    rng = np.random.RandomState(int(bound))
    s = rng.uniform(-bound, bound, size=n).astype(np.float32)
    th = rng.uniform(-bound, bound, size=n).astype(np.float32)
    c = rng.choice(np.array([0.0, 1.0, 0.25, 0.5, 1.0, 0.0], np.float32), size=n)
    loss32, gs32, gt32 = T.kernel32(s, th, c, comb)
    s64, c64 = torch.tensor(s.astype(np.float64)).view(n, 1), torch.tensor(c.astype(np.float64)).view(n, 1)
    th64 = torch.tensor(th.astype(np.float64)).view(n, 1)
    # row i pairs s_i with theta_i: element_loss broadcasts theta over columns, so hand it one column per call
    s_r = s64.view(1, n).clone().requires_grad_(True)
    th_r = th64.view(n).clone().requires_grad_(True)
    el = T.element_loss(s_r, th_r, c64.view(1, n), comb)
    el.sum().backward()
    gs, gt, a_s, a_t = T.closed_form_grads(s_r.detach(), th_r.detach(), c64.view(1, n), comb)
    if comb == "sum":
        z = (s_r + th_r.view(1, -1)).detach()
        el_abs = (c64.view(1, n) * torch.nn.functional.logsigmoid(z)).abs() + ((1 - c64.view(1, n)) * torch.nn.functional.logsigmoid(-z)).abs()
    else:
        el_abs = el.detach().abs()
    e_loss = T.excess(loss32, el.detach().numpy().ravel(), el_abs.numpy().ravel())
    e_s = T.excess(gs32, s_r.grad.numpy().ravel(), a_s.numpy().ravel())
    e_t = T.excess(gt32, th_r.grad.numpy().ravel(), a_t.numpy().ravel())
    print("%s |x| <= %g: loss %.2e, d/ds %.2e, d/dtheta %.2e of the terms (bar %.0e)" % (comb, bound, e_loss, e_s, e_t, R.TERMS_RTOL))
    assert np.isfinite(loss32).all() and np.isfinite(gs32).all() and np.isfinite(gt32).all()
    assert max(e_loss, e_s, e_t) <= R.TERMS_RTOL


def test_careless_log_of_q_misses_where_p_is_small():
    """log q = log(sigmoid(-s) + sigmoid(s) sigmoid(-theta)) used also where p is small rounds q to 1: the saturating cases tell it
    from log1p(-p)."""
    f = np.float32
    s, th = f(-8.0), f(-8.0)
    p = (1.0 / (1.0 + np.exp(8.0))) ** 2  # 1.1e-7: two float32 spacings below 1
    sig = lambda x: f(1.0) / (f(1.0) + np.exp(-x, dtype=f))  # noqa: E731
    q32 = sig(-s) + sig(s) * sig(-th)
    careless, right = -np.log(q32, dtype=f), T.kernel32(s, th, f(0.0), "product")[0]
    ref = -np.log1p(-p)
    assert abs(float(right) - ref) <= R.TERMS_RTOL * ref and abs(float(careless) - ref) > 1000 * R.TERMS_RTOL * ref


def test_hparams_parse_and_refuse_an_unknown_combination():
    from ultra_pytorch_amd.learning_algorithm import TwoTower
    from ultra_pytorch_amd.utils import find_class
    assert find_class("ultra_pytorch_amd.learning_algorithm.TwoTower") is TwoTower and TwoTower.ENGINE_ALGO == "twotower"
    hp = TwoTower.parse_hparams("")
    assert (hp.learning_rate, hp.max_gradient_norm, hp.l2_loss, hp.grad_strategy) == (0.05, 5.0, 0.0, "ada")
    assert (hp.tower_combination, hp.propensity_learning_rate, hp.mask_padding) == ("product", -1.0, True)
    hp = TwoTower.parse_hparams("tower_combination=sum,propensity_learning_rate=0.01,mask_padding=False,grad_strategy=adam,l2_loss=0.01")
    assert (hp.tower_combination, hp.propensity_learning_rate, hp.mask_padding, hp.grad_strategy, hp.l2_loss) == ("sum", 0.01, False, "adam", 0.01)
    with pytest.raises(ValueError, match="tower_combination"):
        TwoTower.parse_hparams("tower_combination=ratio")


def test_optimizer_state_sizes():
    from ultra_pytorch_amd import _lib, engine
    P, L = 1234, 17
    assert engine.opt_state_floats("twotower", "sgd", L, P) == 0
    assert engine.opt_state_floats("twotower", "ada", L, P) == P + L
    assert engine.opt_state_floats("twotower", "adam", L, P) == 2 * P + 2 * L
    assert engine.opt_state_floats("regem", "ada", L, P) == P and engine.opt_state_floats("dla", "adam", L, P) == 2 * P + 2 * (L + 1)
    u = _lib.UpdateDesc()
    u.algo, u.optimizer, u.list_size, u.n_params = 8, _lib.OPT_ADAGRAD, L, P
    assert int(_lib.load().ultr_opt_state_floats(ctypes.byref(u))) == -1  # 8 stays no algorithm
    u.algo = 10
    assert int(_lib.load().ultr_opt_state_floats(ctypes.byref(u))) == -1
    for opt in ("sgd", "ada", "adam"):
        assert T.state_floats(opt, P, L) == engine.opt_state_floats("twotower", opt, L, P)


def test_entry_is_exported_bound_and_declared_at_abi_8():
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    assert int(lib.ultr_abi_version()) == _lib.ABI_VERSION == 8
    assert hasattr(lib, "ultr_twotower_loss") and _lib.ALGO_TWOTOWER == 9
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert _lib.SIGNATURES["ultr_twotower_loss"] == (i32, [vp, vp, vp, i32, vp, i64, i32, i32, vp, vp, vp])
    hdr = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    m = re.search(r"\bint ultr_twotower_loss\(([^)]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == 11
    assert re.search(r"ULTR_ALGO_TWOTOWER = 9\b", hdr) and re.search(r"#define\s+ULTR_ABI_VERSION\s+8\b", hdr)
    # bad arguments are refused on the host, with nothing launched (no GPU is needed to be told so)
    assert lib.ultr_twotower_loss(None, None, None, 0, None, 0, 3, 5, None, None, None) == -1
    # the layout: the tail alone, 64 KiB -> 8190 documents; one more is refused; the value 8 is no algorithm
    tail_bytes = lambda L: (4 + 2 * L) * 4  # noqa: E731
    assert hip_ops.loss_lds_bytes(_lib.ALGO_TWOTOWER, 10) == tail_bytes(10)
    longest = max(L for L in range(8000, 8400) if int(lib.ultr_loss_lds_bytes(_lib.ALGO_TWOTOWER, L)) >= 0)
    assert longest == 8190 and int(lib.ultr_loss_lds_bytes(_lib.ALGO_TWOTOWER, longest + 1)) == -2
    assert int(lib.ultr_loss_lds_bytes(8, 10)) == -1
    assert "list_size up to %d " % longest in hdr[hdr.index("---- TwoTower"):hdr.index("int ultr_twotower_loss(")]
    assert hip_ops.loss_route(_lib.ALGO_TWOTOWER, longest) == "short"
    with pytest.raises(_lib.UltrHipError):
        hip_ops.loss_route(_lib.ALGO_TWOTOWER, longest + 1)


@pytest.mark.parametrize("comb", COMBINATIONS)
def test_export_propensity_round_trips_through_the_estimator(comb, tmp_path):
    from ultra_pytorch_amd.learning_algorithm import TwoTower
    from ultra_pytorch_amd.utils.propensity_estimator import BasicPropensityEstimator
    algo = TwoTower.__new__(TwoTower)  # the table needs the learned logits and the hyper-parameters only, no GPU
    algo.hparams = TwoTower.parse_hparams("tower_combination=" + comb)
    theta = np.array([T.LN9, 1.0, 0.0, -1.5, -4.0], np.float32)
    algo.bias_logits = torch.tensor(theta)
    path = str(tmp_path / "learned.json")
    if comb == "sum":
        with pytest.raises(ValueError, match="examination"):
            algo.propensity
        with pytest.raises(ValueError):
            algo.export_propensity(path)
        return
    sig = 1.0 / (1.0 + np.exp(-theta.astype(np.float64)))
    assert tuple(algo.propensity.shape) == (1, 5) and np.allclose(algo.propensity.numpy().ravel(), sig, rtol=1e-6)
    table = algo.export_propensity(path)
    est = BasicPropensityEstimator(path)
    assert est.IPW_list == table and np.allclose(table, sig[0] / sig, rtol=1e-6) and table[0] == 1.0
    assert est.getPropensityForOneList([1, 0, 1, 0, 1]) == [table[0], 0.0, table[2], 0.0, table[4]]


@pytest.mark.parametrize("opt", ["ada", "sgd", "adam"])
def test_twin_state_travels_in_the_device_layout(opt):
    """Two persistent steps of one twin; a second twin put where the first stood after step 1 (load: parameters, theta, the state
    vector in ultr_opt_state_floats' layout, the steps taken) takes the same second step.  A forced gradient replaces autograd's."""
    from oracle import ultr_oracle as O
    rng = np.random.RandomState(4)
    B, L = 5, 7
    feats = rng.uniform(-1, 1, size=(B * L, R.TOY_F)).astype(np.float32)
    ids = rng.permutation(B * L).astype(np.int32).reshape(L, B)
    ids[L - 1, 0] = B * L  # a PAD
    y = rng.choice(np.array([0.0, 1.0, 0.5, 3.0], np.float32), size=(L, B))
    p0 = O.init_params(R.TOY_F, R.TOY_HIDDEN, seed=1)
    h = T.hyper_of(optimizer=opt, max_gradient_norm=0.05, l2_loss=0.01, propensity_learning_rate=0.2)
    a = T.dnn_twin(p0, T.theta_init("product", L), h, R.TOY_F, R.TOY_HIDDEN, feats, ids)
    r1 = a.step(y, ids, B * L)
    assert r1["coef"] < 1.0 and r1["pcoef"] < 1.0 and r1["D"] == B and r1["scores"].shape == (B, L)
    assert len(a.state()) == T.state_floats(opt, a.P, L)
    snap = (a.flat().copy(), a.theta.detach().numpy().copy(), a.state().copy())
    r2 = a.step(y, ids, B * L)
    b = T.dnn_twin(p0, T.theta_init("product", L), h, R.TOY_F, R.TOY_HIDDEN, feats, ids)
    b.load(snap[0], snap[1], snap[2], 1)
    r2b = b.step(y, ids, B * L, force_grad=r2["grad"], force_theta_grad=r2["theta_grad"])
    assert np.allclose(b.flat(), a.flat(), rtol=0, atol=1e-15) and np.allclose(b.theta.detach().numpy(), a.theta.detach().numpy(), atol=1e-15)
    assert np.allclose(b.state(), a.state(), rtol=1e-14, atol=0) and abs(r2b["loss"] - r2["loss"]) < 1e-14
    # the PAD position of list 0 reaches neither tower
    parts = T.loss_parts(r1["scores"], y, T.theta_init("product", L), "product", ids, B * L)
    assert parts["ds"][0, L - 1] == 0.0 and not parts["live"][0, L - 1]
    # the loss is the definition: mean over lists of the sum over positions
    assert abs(parts["loss"] + 0.5 * h["l2_loss"] * float((p0.astype(np.float64) ** 2).sum()) - r1["loss"]) < 1e-12
