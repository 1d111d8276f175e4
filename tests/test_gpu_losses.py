"""The five list-loss kernels (softmax_ce_kernel, dla_loss_kernel, pairdebias_kernel, lambdarank_kernel, regem_kernel), the
two-level fold of their step tails and block 0's duties in the update launch against the float64 restatement tests/loss_ref.py,
at the settings the oracle-parity tests leave at their defaults: list lengths at the lane and slice boundaries, saturating
scores, graded / fractional / missing clicks, tied scores, every hyper-parameter of the step tail off its default, and EVERY
updated parameter and accumulator.  The inputs are the shared tables of loss_ref.py; tests/test_loss_ref_cpu.py shows that the
float32 oracle holds the same bars on them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import loss_ref as R  # noqa: E402
from tests import margins  # noqa: E402
from tests.hipref import HipRun  # noqa: E402

F = R.TAIL_FIXED


def make_run(case, net=False):
    B, L = case["B"], case["L"]
    run = HipRun(R.TOY_F, R.TOY_HIDDEN, B, L, algo=case["algo"], **case["kw"])
    if net:
        run.set_inputs(case["feats"], case["ids"], case["labels"])
        run.forward(case["params"])
    else:
        run.set_inputs(np.zeros((1, R.TOY_F), np.float32), np.zeros((L, B), np.int32), case["labels"])
    return run


def run_loss(run, case):
    return run.loss(aux=case["aux"], ipw_table=case["ipw"], uniforms=case["uniforms"], scores=case["scores"])


def group_of(case):
    return "losses/%s/%s" % (case["algo"], case["name"].split("-")[0])


def hold_tail(case, tail, what="tail"):
    """Head and per-position sums of a step tail against the restatement: |got - ref| <= 1e-5 (|ref| + sum |terms|) per word, and
    the losses the head stands for at 1e-5 max(1, |ref|)."""
    ref = R.reference(case)
    ex = R.terms_excess(tail, ref["tail"], ref["tail_abs"])
    print("%s %s: max excess over (|ref| + terms) %.3e" % (case["name"], what, ex))
    margins.check(group_of(case), "%s/%s" % (case["name"], what), ex)
    assert ex <= R.TERMS_RTOL, (what, ex)
    for k in ((0, 2) if case["algo"] == "dla" else (0,)):
        den = 1.0 if case["algo"] == "pairdebias" else ref["tail"][k + 1]
        got_den = 1.0 if case["algo"] == "pairdebias" else float(tail[k + 1])
        want = ref["tail"][k] / den if den != 0 else 0.0
        got = float(tail[k]) / got_den if got_den != 0 else 0.0
        assert abs(got - want) <= R.SCALAR_RTOL * max(1.0, abs(want)), ("loss", k, got, want)


def hold_dscores(case, ds):
    ref = R.reference(case)
    ex = R.terms_excess(ds, ref["ds"], ref["ds_abs"])
    print("%s dscores: max excess over (|ref| + terms) %.3e" % (case["name"], ex))
    margins.check(group_of(case), "%s/dscores" % case["name"], ex)
    assert ex <= R.TERMS_RTOL, ("dscores", ex)
    if case["algo"] == "regem":  # the pseudo-labels, the only discrete quantity: dscores x D = sigmoid(s) - y
        y = np.rint(1.0 / (1.0 + np.exp(-case["scores"].astype(np.float64))) - ds)
        np.testing.assert_array_equal(y, ref["pseudo"])


@pytest.mark.parametrize("name", list(R.loss_cases()))
def test_loss_kernels(name):
    """len-*: L in {1, 2, 15, 16, 17, 63, 64, 65, 129, 255, 256} (waves whose slice of the list is empty, one lane short of / past a
    wavefront, the cap), B = 3; DLA also with logits_to_prob = sigmoid beyond 64 positions; RegressionEM's `l += 64` loops take up
    to four trips.  scale-*: scores x 8 (LambdaRank x 4, loss_ref.SCORE_SCALE).  labels-*: graded and fractional clicks through
    PairDebias' mask min(1, |c_i - c_j|), a list without a click and one with a single click, a LambdaRank list of all-equal
    labels (gradients exactly 0).  tie-*: the last 1, 5, L - 1 documents share one score and differ in label - the stable order.
    edge-*: PairDebias at L = 585 and LambdaRank at L = 531, the longest lists their 160 KiB of LDS hold (B = 2)."""
    case = R.loss_cases()[name]
    run = make_run(case)
    ds, tail = run_loss(run, case)
    hold_tail(case, tail)
    hold_dscores(case, ds)
    if name == "labels-lambdarank-flat":
        assert (ds[0] == 0.0).all()
        assert np.abs(ds[1:]).max() > 0 and tail[1] > 0


def test_pair_walk_kernels_refuse_lists_beyond_the_lds_budget():
    """One document past the longest accepted list (edge-pairdebias-L585, edge-lambdarank-L531 above): a host refusal, nothing is
    launched."""
    import torch
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    for fn, L in (("ultr_pairdebias_loss", 586), ("ultr_lambdarank_loss", 532)):
        s = torch.zeros(1, L, device="cuda")
        ds = torch.full((1, L), 7.0, device="cuda")
        ws = torch.zeros(hip_ops.loss_workspace_bytes(1, L) // 4, device="cuda")
        t = torch.ones(L, device="cuda")
        if fn == "ultr_pairdebias_loss":
            rc = lib.ultr_pairdebias_loss(s.data_ptr(), s.data_ptr(), t.data_ptr(), t.data_ptr(), 1, L, 1, ds.data_ptr(), ws.data_ptr(),
                                          hip_ops.raw_stream())
        else:
            rc = lib.ultr_lambdarank_loss(s.data_ptr(), s.data_ptr(), t.data_ptr(), t.data_ptr(), 1.0, 1, L, ds.data_ptr(), ws.data_ptr(),
                                          hip_ops.raw_stream())
        assert rc == -2, (fn, rc)  # ULTR_E_UNSUPPORTED
        torch.cuda.synchronize()
        assert (ds == 7.0).all() and not ws.any()


def hold_step(case, run, g, tail2, out):
    """After loss -> backward -> update: the new per-position state, the eight step scalars, every parameter and accumulator."""
    p_new, s_new, aux_new, sc = out
    algo = case["algo"]
    hyper = R.hyper_of(algo, **case["kw"])
    ref = R.reference(case)
    ss = float((g.astype(np.float64) ** 2).sum())
    aux_ref, want = R.tail_update(algo, ref["tail"], case["aux"], hyper, ss=ss, l2_sums=R.l2_sums_of(case["params"], g))
    # --- the per-position state
    if aux_ref is not None:
        err = float(np.abs(aux_new - aux_ref).max()) if np.isfinite(aux_new).all() else float("inf")
        print("%s aux: max error %.3e" % (case["name"], err))
        margins.check(group_of(case), "%s/aux" % case["name"], err)
        assert err <= R.aux_atol(case), ("aux", err)
    # --- the eight scalars: loss, norm, coef, D, rank_loss, exam_loss, pnorm, sum g^2
    got = dict(zip(("loss", "norm", "coef", "D", "rank_loss", "exam_loss", "pnorm"), [float(v) for v in sc[:7]]))
    for k, w in want.items():
        assert abs(got[k] - w) <= R.SCALAR_RTOL * max(1.0, abs(w)), (k, got[k], w)
    assert abs(float(sc[7]) - ss) <= R.SCALAR_RTOL * max(1.0, ss), ("sum g^2", float(sc[7]), ss)
    mg = hyper["max_gradient_norm"]
    if mg == 0.0 or (hyper["l2_loss"] > 0 and algo != "dla"):
        assert got["coef"] == 1.0
    elif "clip0.01" in case["name"] or case["name"].endswith("-pc"):
        assert got["coef"] < 1.0 and want["coef"] < 1.0
    if case["name"].endswith("-pc") or (algo == "dla" and "clip0.01" in case["name"]):
        assert want["pnorm"] > mg  # DLA's own clip bites
    # --- every parameter and accumulator against the restated step on the GPU's OWN gradient, sum of squares and tail
    want_p, want_s = R.param_update(case["params"], g, case["state"], float(sc[7]), hyper, tail2)
    perr = float(np.abs(p_new - want_p).max()) if np.isfinite(p_new).all() else float("inf")
    print("%s parameters: max error %.3e" % (case["name"], perr))
    margins.check(group_of(case), "%s/params" % case["name"], perr)
    assert perr <= R.PARAM_ATOL, ("params", perr, int(np.abs(p_new - want_p).argmax()))
    if hyper["optimizer"] == "sgd" or algo == "dla":
        assert np.array_equal(s_new, case["state"])  # no accumulator: untouched
    else:
        serr = float((np.abs(s_new - want_s) / np.maximum(want_s, 1e-30)).max()) if np.isfinite(s_new).all() else float("inf")
        print("%s accumulators: max relative error %.3e" % (case["name"], serr))
        margins.check(group_of(case), "%s/state" % case["name"], serr)
        assert serr <= R.STATE_RTOL, ("state", serr)


@pytest.mark.parametrize("name", list(R.hyper_cases()))
def test_step_tail_and_update(name):
    """loss -> backward -> update on the toy net (F = 8, hidden [4]) with one hyper-parameter off its default: sigma,
    regulation_p (powf and sqrtf), em_step_size, ranker_loss_weight / propensity_learning_rate, max_gradient_norm 0 / biting /
    default, DLA's own clip, SGD, a non-zero Adagrad accumulator, l2_loss.  Parameters: 4 x the float32 oracle's own error
    against param_update (loss_ref.PARAM_ERR_MEASURED = 6.2e-8, STATE_ERR_MEASURED = 2.8e-7 relative)."""
    case = R.hyper_cases()[name]
    run = make_run(case, net=True)
    ds, tail = run_loss(run, case)
    hold_tail(case, tail)
    hold_dscores(case, ds)
    g, tail2 = run.backward()
    hold_step(case, run, g, tail2, run.update(case["state"].copy()))


@pytest.mark.parametrize("algo,B", R.MANY)
def test_many_lists_fold_the_tail_in_two_levels(algo, B):
    """More than 1024 lists (one loss partial each) and a 70-word tail (L = 33): the weight-gradient launch folds chunks of 1024
    partials, the reduction launch folds the chunk rows, 64 words per pass - two passes.  The folded tail (head and per-position
    sums) against the float64 sum over the lists, then the update that reads it.  B = 1024 / 1025: either side of the switch."""
    case = R.many_case(algo, B)
    run = make_run(case, net=True)
    ds, tail = run_loss(run, case)
    hold_dscores(case, ds)
    g, tail2 = run.backward()
    hold_tail(case, tail2, what="folded-tail")
    hold_step(case, run, g, tail2, run.update(case["state"].copy()))
