"""tests/loss_ref.py (the float64 restatement of the list-loss kernels and of the step tail's duties) tied to the reference, on
the CPU: it reproduces the reference's recorded steps (tests/golden), and on every case of the shared tables the float32
oracle stays inside the bars tests/test_gpu_losses.py holds the kernels to - which is what makes those inputs fair."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from oracle import ultr_oracle as O
from tests import loss_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(f)[:-4] for pre in ("dla_", "pairdebias_", "lambdarank_", "regem_", "na_", "ipw_")
                  for f in glob.glob(os.path.join(GOLDEN, pre + "*.npz")))


def _load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return d, json.loads(str(d["meta"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference(name):
    """Every recorded step of the reference: its scores and labels through the restatement and tail_update(), against what it
    recorded - at the bars test_gpu_parity.py::test_golden_train_step uses for the same quantities."""
    d, m = _load(name)
    hp = dict(kv.split("=") for kv in m.get("algo_hparams", "").split(",") if kv)
    algo = {"na": "softmax", "ipw": "softmax"}.get(m["algo"], m["algo"])
    L = m["L"]
    hyper = R.hyper_of(algo, learning_rate=m["lr"], max_gradient_norm=m["max_gradient_norm"], l2_loss=float(hp.get("l2_loss", 0.0)),
                       ranker_loss_weight=float(hp.get("ranker_loss_weight", 1.0)),
                       propensity_learning_rate=float(hp.get("propensity_learning_rate", -1.0)))
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        s, y = d[p + "scores"], d[p + "labels"]
        if algo == "softmax":
            r, aux = R.softmax_ce(s, y, ipw=d["ipw_list"] if m["algo"] == "ipw" else None), None
        elif algo == "dla":
            aux = d[p + "pre_prop_params"]
            r = R.dla(s, y, aux, hp.get("logits_to_prob", "softmax"))
        elif algo in ("pairdebias", "lambdarank"):
            tp, tm = d[p + "pre_t_plus"].ravel(), d[p + "pre_t_minus"].ravel()
            aux = np.concatenate([tp, tm])
            r = R.pairdebias(s, y, tp, tm) if algo == "pairdebias" else R.lambdarank(s, y, tp, tm, float(m.get("sigma", 1.0)))
        else:
            aux = d[p + "pre_propensity"].ravel()
            r = R.regem(s, y, aux, d[p + "uniforms"])
            np.testing.assert_array_equal(r["pseudo"], d[p + "ranker_labels"])
        p0 = d[p + "pre_params"].astype(np.float64)
        aux2, sc = R.tail_update(algo, r["tail"], aux, hyper, l2_sums=(float((p0 * p0).sum()), 0.0))
        ref_loss = float(d[p + "loss"])
        assert abs(sc["loss"] - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (sc["loss"], ref_loss)
        if algo in ("pairdebias", "lambdarank"):
            np.testing.assert_allclose(aux2[:L], d[p + "post_t_plus"].ravel(), atol=1e-6)
            np.testing.assert_allclose(aux2[L:], d[p + "post_t_minus"].ravel(), atol=1e-6)
        if algo == "regem":
            np.testing.assert_allclose(aux2, d[p + "post_propensity"].ravel(), atol=1e-6)
        if algo == "dla":
            np.testing.assert_allclose(aux2, d[p + "post_prop_params"], atol=1e-6)
            assert abs(sc["pnorm"] - float(d[p + "prop_norm"])) < 1e-6
            assert abs(sc["rank_loss"] - float(d[p + "rank_loss"])) < 1e-5 and abs(sc["exam_loss"] - float(d[p + "exam_loss"])) < 1e-5


# ------------------------------------------------------------------------------------------------------------------------
# the float32 oracle on the shared cases
# ------------------------------------------------------------------------------------------------------------------------
def oracle_losses(case, scores=None):
    """The float32 oracle on a case: dict(loss [, exam], ds = d loss / d scores, pos = its per-position sums) - all NORMALISED as the
    reference has them (the kernels emit them x D; hold_loss_bars() divides the restatement's figures accordingly)."""
    a, L, B = case["algo"], case["L"], case["B"]
    s = torch.tensor(case["scores"] if scores is None else scores, requires_grad=True)
    y_LB = torch.tensor(case["labels"])
    y = y_LB.t().contiguous()
    out = dict(pos=None)
    if a == "softmax":
        pw = None if case["ipw"] is None else O.ipw_weights(case["labels"], case["ipw"])
        loss = O.softmax_loss(s, y, pw)
        out.update(loss=float(loss.detach()))
    elif a == "dla":
        l2p = case["kw"].get("logits_to_prob", "softmax")
        q = torch.tensor(case["aux"], requires_grad=True)
        prop = O.denoising_net(q, B, L)
        with torch.no_grad():
            pw = O.normalized_weights(O.logits_to_prob(prop, l2p))
            rw = O.normalized_weights(O.logits_to_prob(s, l2p))
        loss = O.softmax_loss(s, y, pw)
        exam = O.softmax_loss(prop, y, rw)
        gprop, gq = torch.autograd.grad(exam, (prop, q), retain_graph=True)
        out.update(loss=float(loss.detach()), exam=float(exam.detach()), pos=gprop.sum(0).numpy(), gq=gq, q=q.detach())
    elif a == "pairdebias":
        tp, tm = torch.tensor(case["aux"][:L]), torch.tensor(case["aux"][L:])
        loss, PL, tpl, tml = O.pairdebias_loss(s, y_LB, tp, tm)
        out.update(loss=float(loss.detach()), pos=np.concatenate([tpl.detach().numpy(), tml.detach().numpy()]), tpl=tpl.detach(), tml=tml.detach())
    elif a == "lambdarank":
        tp, tm = torch.tensor(case["aux"][:L]), torch.tensor(case["aux"][L:])
        loss, PL, tpl, tml = O.lambdarank_loss(s, y, tp, tm, float(case["kw"].get("sigma", 1.0)))
        out.update(loss=float(loss.detach()), pos=np.concatenate([tpl.detach().numpy(), tml.detach().numpy()]), tpl=tpl.detach(), tml=tml.detach())
    else:
        prop = torch.tensor(case["aux"]).reshape(1, -1)
        with torch.no_grad():
            p_e1_r0, p_r1 = O.regression_em_estimation(s.detach(), y, prop)
            pseudo = torch.ceil(p_r1 - torch.tensor(case["uniforms"]))
            m = y + (1 - y) * p_e1_r0
        loss = torch.nn.functional.binary_cross_entropy_with_logits(s, pseudo)
        out.update(loss=float(loss.detach()), pos=m.sum(0).numpy(), pseudo=pseudo.numpy(), mstep=torch.mean(m, dim=0), prop=prop)
    (g,) = torch.autograd.grad(loss, s)
    out["ds"] = g.numpy()
    return out


def hold_loss_bars(case, o, ref, rtol=R.TERMS_RTOL, srtol=R.SCALAR_RTOL):
    """The oracle's (normalised) figures against the restatement's tail and dscores x D at the GPU bars."""
    a, L, t = case["algo"], case["L"], ref["tail"]
    D = 1.0 if a == "pairdebias" else t[1]
    want = t[0] / D
    assert abs(o["loss"] - want) <= srtol * max(1.0, abs(want)), ("loss", o["loss"], want)
    ex = R.terms_excess(o["ds"], ref["ds"] / D, ref["ds_abs"] / D)
    assert ex <= rtol, ("dscores", ex)
    F = R.TAIL_FIXED
    if a == "dla":
        want = t[2] / t[3]
        assert abs(o["exam"] - want) <= srtol * max(1.0, abs(want)), ("exam_loss", o["exam"], want)
        ex = R.terms_excess(o["pos"], t[F:F + L] / t[3], ref["tail_abs"][F:F + L] / t[3])
    elif a in ("pairdebias", "lambdarank"):
        ex = R.terms_excess(o["pos"], t[F:] / D, ref["tail_abs"][F:] / D)
    elif a == "regem":
        np.testing.assert_array_equal(o["pseudo"], ref["pseudo"])
        ex = R.terms_excess(o["pos"], t[F:F + L], ref["tail_abs"][F:F + L])
    else:
        ex = 0.0
    assert ex <= rtol, ("per-position sums", ex)


def _all_cases():
    cases = dict(R.loss_cases())
    cases.update(R.hyper_cases())
    return cases


@pytest.mark.parametrize("name", [n for n, c in _all_cases().items() if not (c["tie"] and c["algo"] == "lambdarank")])
def test_oracle_losses_hold_the_gpu_bars(name):
    case = _all_cases()[name]
    hold_loss_bars(case, oracle_losses(case), R.reference(case))


@pytest.mark.parametrize("algo,B", R.MANY)
def test_oracle_losses_hold_the_gpu_bars_on_many_lists(algo, B):
    case = R.many_case(algo, B)
    hold_loss_bars(case, oracle_losses(case), R.reference(case))


@pytest.mark.parametrize("name", [n for n, c in R.loss_cases().items() if c["tie"] and c["algo"] == "lambdarank"])
def test_lambdarank_ties_follow_the_stable_order(name):
    """torch.sort leaves the order inside a tie unspecified, so the oracle runs on scores whose ties are broken the way the kernel
    documents (earlier index first): s - 1e-3 x index inside the tie.  That moves z = sigma (s_r - s_c) of a pair by up to
    1e-3 (k - 1); every term of the loss and of the gradient is a product of delta (unchanged: same order), x (1 - x) and
    sigmoid(x) - target, whose logarithmic derivatives in z are at most 1 in magnitude where the term matters, so each sum moves
    by at most ~2e-3 (k - 1) of the sum of its absolute terms.  The bar is that plus the usual 1e-5; a REVERSED tie order swaps
    the labels inside the tie (they differ by construction) and moves the tied documents' gradients by their own size."""
    case = R.loss_cases()[name]
    k, L = case["tie"], case["L"]
    broken = case["scores"].copy()
    broken[:, L - k:] -= (1e-3 * np.arange(k)).astype(np.float32)[None, :]
    ref = R.reference(case)
    assert np.array_equal(R.stable_order(broken), ref["order"])
    bar = 1e-5 + 2e-3 * (k - 1)
    hold_loss_bars(case, oracle_losses(case, scores=broken), ref, rtol=bar, srtol=bar)


@pytest.mark.parametrize("labels", ["graded", "fractional"])
def test_pairdebias_restatement_equals_the_reference_loop_structure(labels):
    """pairdebias_loss_loops - the reference's own two-level Python loop with its [B] x [B, 1] broadcast - at L = 5, with graded
    labels (the mask min(1, c_i - c_j) clamps) and fractional ones (it does not)."""
    case = R.make_case("loops-" + labels, "pairdebias", 3, 5, labels=labels)
    L = 5
    s = torch.tensor(case["scores"], requires_grad=True)
    loss, PL, tpl, tml = O.pairdebias_loss_loops(s, torch.tensor(case["labels"]), torch.tensor(case["aux"][:L]), torch.tensor(case["aux"][L:]))
    (g,) = torch.autograd.grad(loss, s)
    o = dict(loss=float(loss.detach()), ds=g.numpy(), pos=np.concatenate([tpl.detach().numpy(), tml.detach().numpy()]))
    hold_loss_bars(case, o, R.pairdebias(case["scores"], case["labels"], case["aux"][:L], case["aux"][L:]))


# ------------------------------------------------------------------------------------------------------------------------
# the step tail and the elementwise update
# ------------------------------------------------------------------------------------------------------------------------
def oracle_aux(case, o, hyper):
    """The float32 oracle's per-position state after the step."""
    a, L = case["algo"], case["L"]
    alpha, p = hyper["em_step_size"], hyper["regulation_p"]
    with torch.no_grad():
        if a in ("pairdebias", "lambdarank"):
            tp, tm = torch.tensor(case["aux"][:L]), torch.tensor(case["aux"][L:])
            safe = a == "lambdarank"
            return torch.cat([O.em_update(tp, o["tpl"], alpha, p, safe), O.em_update(tm, o["tml"], alpha, p, safe)]).numpy(), None
        if a == "regem":
            return ((1 - alpha) * o["prop"] + alpha * o["mstep"].reshape(1, -1)).numpy().ravel(), None
        if a == "dla":
            q2, _, nq, _ = O.apply_update(o["q"], o["gq"], torch.zeros_like(o["gq"]), hyper["propensity_learning_rate"],
                                          hyper["max_gradient_norm"], hyper["optimizer"], stateless=True)
            return q2.numpy(), float(nq)
    return None, None


STEP_CASES = dict(R.hyper_cases())
STEP_CASES.update({R.many_case(a, B)["name"]: R.many_case(a, B) for a, B in R.MANY})


@pytest.mark.parametrize("name", [n for n, c in STEP_CASES.items() if c["algo"] != "softmax"])
def test_oracle_step_tail_holds_the_gpu_bars(name):
    """The oracle's own t_plus / t_minus, propensity and DenoisingNet parameters after the step against tail_update() on the
    restatement's tail: inside the bar the GPU gets.  With regulation_p = 0 the figure is the measured one loss_ref.py carries."""
    case = STEP_CASES[name]
    hyper = R.hyper_of(case["algo"], **case["kw"])
    o = oracle_losses(case)
    got, pnorm = oracle_aux(case, o, hyper)
    want, sc = R.tail_update(case["algo"], R.reference(case)["tail"], case["aux"], hyper, l2_sums=(0.0, 0.0))  # (no part in aux)
    err = float(np.abs(got - want).max())
    print("aux error of the float32 oracle: %s %.3e" % (name, err))
    if float(case["kw"].get("regulation_p", 1.0)) == 0.0:
        assert err <= R.AUX_P0_ERR_MEASURED[case["algo"]], err
    assert err <= R.aux_atol(case), err
    if pnorm is not None:
        assert abs(pnorm - sc["pnorm"]) <= R.SCALAR_RTOL * max(1.0, sc["pnorm"])
        if name.endswith("-pc"):
            assert sc["pnorm"] > hyper["max_gradient_norm"]  # the case is about pc < 1


def toy_gradient(case):
    """The toy net's RAW gradient (x D) in float32 from the restatement's dscores x D: (g_raw, ss = its float64 sum of squares)."""
    x = O.gather_rows(case["feats"], case["ids"]).numpy()
    ds = R.reference(case)["ds"].astype(np.float32)
    g = O.dnn_backward_manual(case["params"], R.TOY_F, R.TOY_HIDDEN, x, ds.T.reshape(-1))
    return g, float((g.astype(np.float64) ** 2).sum())


def oracle_param_error(case):
    """apply_update (float32) against param_update (float64) on the same raw float32 gradient: (max |p' - ref|, max relative
    accumulator error)."""
    hyper = R.hyper_of(case["algo"], **case["kw"])
    tail = R.reference(case)["tail"]
    g_raw, ss = toy_gradient(case)
    p, st = case["params"], case["state"]
    want_p, want_s = R.param_update(p, g_raw, st, ss, hyper, tail)
    sc = R.step_scalars(tail, ss, hyper, R.l2_sums_of(p, g_raw))
    g = torch.tensor(g_raw) * np.float32(sc["gs"])
    if sc["lam"] != 0.0:
        g = g + np.float32(sc["lam"]) * torch.tensor(p)
    clip = hyper["max_gradient_norm"] if (hyper["l2_loss"] == 0 or case["algo"] == "dla") else 0.0
    p2, s2, n, _ = O.apply_update(torch.tensor(p), g, torch.tensor(st), hyper["learning_rate"], clip, hyper["optimizer"],
                                  stateless=case["algo"] == "dla")
    assert abs(float(n) - sc["norm"]) <= R.SCALAR_RTOL * max(1.0, sc["norm"])
    perr = float(np.abs(p2.numpy() - want_p).max())
    serr = 0.0
    if hyper["optimizer"] != "sgd" and case["algo"] != "dla":
        serr = float((np.abs(s2.numpy() - want_s) / np.maximum(want_s, 1e-30)).max())
    return perr, serr


def test_oracle_update_error_is_inside_the_measured_figures():
    """The figures loss_ref.py's PARAM_ATOL / STATE_RTOL are four times of: the float32 oracle's parameter and accumulator error
    against param_update() over every step case."""
    worst_p = worst_s = 0.0
    for name, case in R.hyper_cases().items():
        perr, serr = oracle_param_error(case)
        worst_p, worst_s = max(worst_p, perr), max(worst_s, serr)
    print("float32 oracle against param_update: parameters %.3e, accumulators (relative) %.3e" % (worst_p, worst_s))
    assert worst_p <= R.PARAM_ERR_MEASURED and worst_s <= R.STATE_ERR_MEASURED
    assert worst_p >= 0.25 * R.PARAM_ERR_MEASURED and worst_s >= 0.25 * R.STATE_ERR_MEASURED  # the figures are measurements
