"""The long-list kernels of the pair-walk losses (csrc/ultr_loss_long.hip: pairdebias_long_kernel, lambdarank_long_kernel,
prs_loss_long_kernel) and their routing, against the float64 restatements tests/loss_ref.py and tests/prs_ref.py (evaluated list by
list, tests/loss_long_ref.py) at the bars those files carry:

    dscores and per-position sums   |got - ref| <= TERMS_RTOL (|ref| + sum |terms|) per word
    losses and step scalars         |got - ref| <= SCALAR_RTOL max(1, |ref|)
    PRSrank                         loss 1e-5 |ref|; dscores rtol 1e-4, atol 1e-5 max |ref|  (tests/test_gpu_prs.py)

Lengths: 1, 2, the lane boundary (63, 64, 65), the 1024-thread boundary where a thread starts owning two positions (1023, 1024,
1025), the first length the short kernel refuses, MSLR-WEB30K's 1251 and the entry's own longest list.  (PairDebias at 6823 documents
spends its seconds in the float64 reference of 2 x 6823^2 pairs, not on the GPU.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import loss_long_ref as LR  # noqa: E402
from tests import loss_ref as R  # noqa: E402
from tests import margins  # noqa: E402
from tests.hipref import HipRun, dev  # noqa: E402

F = R.TAIL_FIXED
DS_FILL, WS_FILL = 7.0, 3.0
FORMS = ("pairdebias", "lambdarank", "prs", "prs_pw")
ALGO_OF = {"pairdebias": "pairdebias", "lambdarank": "lambdarank", "prs": "prs", "prs_pw": "prs"}


def lengths(form):
    a = ALGO_OF[form]
    return [1, 2, 63, 64, 65, 1023, 1024, 1025, LR.SHORT_MAX[a] + 1, LR.MSLR, LR.MAX_LIST[a]]


def batch_of(L):
    return 3 if L <= 1025 else 2


def entry(form, long):
    from ultra_pytorch_amd import hip_ops
    return getattr(hip_ops, {"pairdebias": "pairdebias_loss", "lambdarank": "lambdarank_loss", "prs": "prs_loss",
                             "prs_pw": "prs_loss_pw"}[form] + ("_long" if long else ""))


def launch(form, long, B, L, scores, labels_LB, extra, sigma=1.0, batch_total=None):
    """One direct call of an entry on poisoned outputs: (dscores [B, L], the workgroups' tails [B, 4 + 2L]) as device tensors."""
    from ultra_pytorch_amd import hip_ops
    s, y = dev(np.asarray(scores, np.float32)), dev(np.asarray(labels_LB, np.float32))
    ds = torch.full((B, L), DS_FILL, dtype=torch.float32, device="cuda")
    ws = torch.full((hip_ops.loss_workspace_bytes(B, L) // 4,), WS_FILL, dtype=torch.float32, device="cuda")
    x = dev(np.asarray(extra, np.float32))
    fn = entry(form, long)
    if form == "pairdebias":
        fn(s, y, x[:L], x[L:], B, L, B if batch_total is None else batch_total, ds, ws)
    elif form == "lambdarank":
        fn(s, y, x[:L], x[L:], sigma, B, L, ds, ws)
    else:
        fn(s, y, x, sigma, B, L, ds, ws)
    torch.cuda.synchronize()
    tail = hip_ops.tail_floats(L)
    assert hip_ops.loss_part_count(B) == B
    assert bool((ws[B * tail:] == WS_FILL).all())  # one partial per list, nothing behind them
    return ds, ws[: B * tail].view(B, tail).clone()


def as_np(ds, parts):
    return ds.double().cpu().numpy(), parts.double().cpu().numpy().sum(0)


# ---- the bars ------------------------------------------------------------------------------------------------------------------------
def hold_pair(case, ds, tail, what, ref=None, key=None):
    """PairDebias / LambdaRank: the tail (head, t_plus and t_minus sums) and dscores against the float64 restatement."""
    ref = LR.reference(case) if ref is None else ref
    L, algo = case["L"], case["algo"]
    group, key = "losses_long/%s" % algo, key or "%s/%s" % (case["name"], what)
    figs = {"tail": R.terms_excess(tail, ref["tail"], ref["tail_abs"]),
            "t_plus": R.terms_excess(tail[F:F + L], ref["tail"][F:F + L], ref["tail_abs"][F:F + L]),
            "t_minus": R.terms_excess(tail[F + L:], ref["tail"][F + L:], ref["tail_abs"][F + L:]),
            "dscores": R.terms_excess(ds, ref["ds"], ref["ds_abs"])}
    print("%s %s: excess over (|ref| + terms): %s" % (case["name"], what, ", ".join("%s %.3e" % kv for kv in figs.items())))
    for k, v in figs.items():
        margins.check(group, "%s/%s" % (key, k), v)
    for k, v in figs.items():
        assert v <= R.TERMS_RTOL, (k, v)
    den = 1.0 if algo == "pairdebias" else ref["tail"][1]
    got_den = 1.0 if algo == "pairdebias" else float(tail[1])
    want = ref["tail"][0] / den if den != 0 else 0.0
    got = float(tail[0]) / got_den if got_den != 0 else 0.0
    assert abs(got - want) <= R.SCALAR_RTOL * max(1.0, abs(want)), ("loss", got, want)
    assert not tail[2:4].any()


def prs_normalised(ds, tail):
    assert not tail[2:].any()
    return tail[0] / tail[1], ds / tail[1]


def hold_prs(name, ds, tail, ref, what):
    """PRSrank: the x D convention undone with the tail's D, at the bars of tests/test_gpu_prs.py."""
    rl, rg, D = ref
    loss, g = prs_normalised(ds, tail)
    gmax = float(np.abs(rg).max())
    lerr = abs(loss - rl) / abs(rl) if rl != 0 else abs(loss)
    gerr = float((np.abs(g - rg) / (1e-5 * gmax + 1e-4 * np.abs(rg))).max()) if gmax > 0 else float(np.abs(g).max())
    print("%s %s: loss relative error %.3e, dscores error over (1e-5 max + 1e-4 |ref|) %.3e" % (name, what, lerr, gerr))
    margins.check("losses_long/prs", "%s/%s/loss" % (name, what), lerr)
    margins.check("losses_long/prs", "%s/%s/dscores_over_bar" % (name, what), gerr)
    assert abs(loss - rl) <= 1e-5 * abs(rl), (loss, rl)
    np.testing.assert_allclose(g, rg, rtol=1e-4, atol=1e-5 * gmax)
    assert abs(tail[1] - D) <= 1e-5 * D


def prs_inputs(form, B, L):
    return LR.prs_batch(B, L, seed=1000 * B + L, per_entry=(form == "prs_pw"))


# ---- 1. the long entries against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,L", [(f, L) for f in FORMS for L in lengths(f)])
def test_long_entries_against_float64(form, L):
    B = batch_of(L)
    if form in ("pairdebias", "lambdarank"):
        case = LR.make_case("long-%s-L%d" % (form, L), form, B, L)
        ds, tail = as_np(*launch(form, True, B, L, case["scores"], case["labels"], case["aux"]))
        hold_pair(case, ds, tail, "long")
    else:
        s, y, ipw = prs_inputs(form, B, L)
        for sigma in (1.0, 0.7):
            ds, tail = as_np(*launch(form, True, B, L, s, y, ipw, sigma=sigma))
            hold_prs("long-%s-L%d-sigma%g" % (form, L, sigma), ds, tail, LR.prs_reference(s, y, ipw, sigma), "long")
            if L > 1025:
                break  # (the longest lists once: their float64 reference is what takes the time)


@pytest.mark.parametrize("form", FORMS)
def test_one_document_past_the_bound_is_refused_with_nothing_launched(form):
    from ultra_pytorch_amd import _lib
    L = LR.MAX_LIST[ALGO_OF[form]] + 1
    extra = np.ones((1, L) if form == "prs_pw" else (2 * L if form != "prs" else 8), np.float32)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        launch(form, True, 1, L, np.zeros((1, L), np.float32), np.zeros((L, 1), np.float32), extra)
    # (launch() raised before its own reads: the same call by hand, on buffers this test keeps)
    from ultra_pytorch_amd import hip_ops
    s = torch.zeros(1, L, device="cuda")
    ds = torch.full((1, L), DS_FILL, device="cuda")
    ws = torch.full((hip_ops.loss_workspace_bytes(1, L) // 4,), WS_FILL, device="cuda")
    x = dev(extra)
    lib, st = _lib.load(), hip_ops.raw_stream()
    if form == "pairdebias":
        rc = lib.ultr_pairdebias_loss_long(s.data_ptr(), s.data_ptr(), x.data_ptr(), x.data_ptr(), 1, L, 1, ds.data_ptr(), ws.data_ptr(), st)
        bad = lib.ultr_pairdebias_loss_long(s.data_ptr(), s.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 8, 0, ds.data_ptr(), ws.data_ptr(), st)
    elif form == "lambdarank":
        rc = lib.ultr_lambdarank_loss_long(s.data_ptr(), s.data_ptr(), x.data_ptr(), x.data_ptr(), 1.0, 1, L, ds.data_ptr(), ws.data_ptr(), st)
        bad = lib.ultr_lambdarank_loss_long(s.data_ptr(), s.data_ptr(), None, x.data_ptr(), 1.0, 1, 8, ds.data_ptr(), ws.data_ptr(), st)
    elif form == "prs":
        rc = lib.ultr_prs_loss_long(s.data_ptr(), s.data_ptr(), x.data_ptr(), 8, 1.0, 1, L, ds.data_ptr(), ws.data_ptr(), st)
        bad = lib.ultr_prs_loss_long(s.data_ptr(), s.data_ptr(), None, 0, 1.0, 1, 8, ds.data_ptr(), ws.data_ptr(), st)
    else:
        rc = lib.ultr_prs_loss_pw_long(s.data_ptr(), s.data_ptr(), x.data_ptr(), 1.0, 1, L, ds.data_ptr(), ws.data_ptr(), st)
        bad = lib.ultr_prs_loss_pw_long(s.data_ptr(), s.data_ptr(), x.data_ptr(), 1.0, 0, 8, ds.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == -2 and bad == -1  # ULTR_E_UNSUPPORTED; ULTR_E_BADARG by the short entry's rules
    assert bool((ds == DS_FILL).all()) and bool((ws == WS_FILL).all())


@pytest.mark.parametrize("form", FORMS)
def test_ties_follow_the_stable_order(form):
    """L = 1100: the last 5 documents share one score and differ in label - rank by counting over 16 waves keeps the stable order
    (ties by original index), which the restatement's stable sort defines."""
    B, L = 2, 1100
    if form in ("pairdebias", "lambdarank"):
        case = LR.make_case("long-tie-%s" % form, form, B, L, tie=5)
        assert len(set(case["scores"][0, L - 5:])) == 1 and len(set(case["labels"][L - 5:, 0])) > 1
        ds, tail = as_np(*launch(form, True, B, L, case["scores"], case["labels"], case["aux"]))
        hold_pair(case, ds, tail, "long")
    else:
        s, y, ipw = prs_inputs(form, B, L)
        s[:, L - 5:] = np.float32(0.125)
        y[L - 5:, :] = np.asarray([0, 1, 0, 1, 1], np.float32)[:, None]
        ds, tail = as_np(*launch(form, True, B, L, s, y, ipw))
        hold_prs("long-tie-%s" % form, ds, tail, LR.prs_reference(s, y, ipw), "long")


def test_lists_that_carry_no_gradient():
    """L = 700: a PairDebias list without a click and a LambdaRank list of equal labels have gradients of exactly 0; a PRSrank batch
    without any click leaves exact zeros everywhere."""
    B, L = 3, 700
    case = LR.make_case("long-sparse-pairdebias", "pairdebias", B, L, labels="sparse")
    ds, tail = as_np(*launch("pairdebias", True, B, L, case["scores"], case["labels"], case["aux"]))
    hold_pair(case, ds, tail, "long")
    assert not case["labels"][:, 0].any() and not ds[0].any() and np.abs(ds[1:]).max() > 0
    case = LR.make_case("long-flat-lambdarank", "lambdarank", B, L, labels="flat")
    ds, tail = as_np(*launch("lambdarank", True, B, L, case["scores"], case["labels"], case["aux"]))
    hold_pair(case, ds, tail, "long")
    assert not ds[0].any() and np.abs(ds[1:]).max() > 0 and tail[1] > 0
    s, _, ipw = prs_inputs("prs", B, L)
    ds, parts = launch("prs", True, B, L, s, np.zeros((L, B), np.float32), ipw)
    assert not ds.any() and not parts.any()


def test_pairdebias_global_batch_factor():
    """batch_total != batch (a data-parallel shard): the reference's x B is the GLOBAL batch."""
    B, L = 2, 586
    case = LR.make_case("long-pairdebias-bt5", "pairdebias", B, L)
    ds, tail = as_np(*launch("pairdebias", True, B, L, case["scores"], case["labels"], case["aux"], batch_total=5))
    hold_pair(case, ds, tail, "long", ref=LR.reference(case, batch_total=5))
    own = LR.reference(case)
    assert abs(tail[0] / own["tail"][0] - 2.5) <= 1e-4


# ---- 2. long against short -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,L", [(f, L) for f in FORMS for L in (64, LR.SHORT_MAX[ALGO_OF[f]])])
def test_long_and_short_kernels_agree_where_both_run(form, L):
    """Each within the bars of float64; within twice the bar of each other (a position's sum is one ascending chain in the long
    kernel, a fold of 16 slice sums in the short one).  The short kernel twice: the same bits."""
    B = 2
    if form in ("pairdebias", "lambdarank"):
        case = LR.make_case("both-%s-L%d" % (form, L), form, B, L)
        args = (case["scores"], case["labels"], case["aux"])
    else:
        args = prs_inputs(form, B, L)
    short1, short2, long1 = launch(form, False, B, L, *args), launch(form, False, B, L, *args), launch(form, True, B, L, *args)
    for a, b in zip(short1, short2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    (ds_s, tail_s), (ds_l, tail_l) = as_np(*short1), as_np(*long1)
    if form in ("pairdebias", "lambdarank"):
        ref = LR.reference(case)
        hold_pair(case, ds_s, tail_s, "short")
        hold_pair(case, ds_l, tail_l, "long")
        assert (np.abs(ds_l - ds_s) <= 2.0 * R.TERMS_RTOL * (np.abs(ref["ds"]) + ref["ds_abs"])).all()
        assert (np.abs(tail_l - tail_s) <= 2.0 * R.TERMS_RTOL * (np.abs(ref["tail"]) + ref["tail_abs"])).all()
    else:
        ref = LR.prs_reference(*args)
        name = "both-%s-L%d" % (form, L)
        hold_prs(name, ds_s, tail_s, ref, "short")
        hold_prs(name, ds_l, tail_l, ref, "long")
        (loss_s, g_s), (loss_l, g_l) = prs_normalised(ds_s, tail_s), prs_normalised(ds_l, tail_l)
        assert abs(loss_l - loss_s) <= 2.0 * 1e-5 * abs(ref[0])
        assert (np.abs(g_l - g_s) <= 2.0 * (1e-5 * np.abs(ref[1]).max() + 1e-4 * np.abs(ref[1]))).all()


# ---- 3. engine routing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ("pairdebias", "lambdarank", "prs"))
def test_engine_loss_takes_the_first_list_the_short_kernel_refuses(algo):
    """engine.StepEngine.loss() at 586 / 532 / 953 documents (the stage StagedStepEngine calls for SetRank, DLCM and GSF)."""
    B, L = 2, LR.SHORT_MAX[algo] + 1
    run = HipRun(R.TOY_F, R.TOY_HIDDEN, B, L, algo=algo)
    if algo == "prs":
        s, y, ipw = prs_inputs("prs", B, L)
        run.set_inputs(np.zeros((1, R.TOY_F), np.float32), np.zeros((L, B), np.int32), y)
        ds, tail = run.loss(ipw_table=ipw, scores=s)
        hold_prs("engine-prs-L%d" % L, ds.astype(np.float64), tail.astype(np.float64), LR.prs_reference(s, y, ipw), "engine")
        s, y, ipw = prs_inputs("prs_pw", B, L)
        run.set_inputs(np.zeros((1, R.TOY_F), np.float32), np.zeros((L, B), np.int32), y)
        ds, tail = run.loss(pw=ipw, scores=s)
        hold_prs("engine-prs_pw-L%d" % L, ds.astype(np.float64), tail.astype(np.float64), LR.prs_reference(s, y, ipw), "engine")
    else:
        case = LR.make_case("engine-%s-L%d" % (algo, L), algo, B, L)
        run.set_inputs(np.zeros((1, R.TOY_F), np.float32), np.zeros((L, B), np.int32), case["labels"])
        ds, tail = run.loss(aux=case["aux"], scores=case["scores"])
        hold_pair(case, ds.astype(np.float64), tail.astype(np.float64), "engine")
    run.eng.close()


@pytest.mark.parametrize("algo", ("pairdebias", "lambdarank", "prs"))
def test_engine_loss_still_refuses_20000_documents(algo):
    from ultra_pytorch_amd import _lib, engine, hip_ops
    d = torch.device("cuda")
    B, L = 1, 20000
    eng = engine.StepEngine(hip_ops.DnnShape(8, [4]), B, L, d, algo=algo)
    eng.dscores.fill_(DS_FILL)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        eng.loss(torch.ones(L, B, device=d), aux=torch.ones(2 * L, device=d), ipw_table=torch.ones(8, device=d))
    torch.cuda.synchronize()
    assert bool((eng.dscores == DS_FILL).all()) and not bool(eng.loss_ws.any())
    eng.close()


# ---- 4. whole steps --------------------------------------------------------------------------------------------------------------------
STEP_F, STEP_HIDDEN, STEP_B = LR.STEP_F, LR.STEP_HIDDEN, LR.STEP_B
step_inputs = LR.step_inputs  # (the seeds: loss_long_ref.STEP_SEED, where the float32 oracle itself keeps to a quarter of the bar)


def one_call_step(d):
    """One ultr_train_step from d's state on a fresh engine: everything the step leaves, as numpy."""
    from ultra_pytorch_amd import engine, hip_ops
    shape = hip_ops.DnnShape(d["F"], d["hidden"], d["act"])
    eng = engine.StepEngine(shape, d["B"], d["L"], torch.device("cuda"), algo=d["algo"])
    p, st = dev(d["params"].copy()), dev(d["state"].copy())
    aux = None if d["aux"] is None else dev(d["aux"].copy())
    tab = None if d["ipw"] is None else dev(d["ipw"])
    sc = eng.train_step(p, st, dev(d["feats"]), d["feats"].shape[0], dev(d["ids"], torch.int32), dev(d["y"], torch.float32), aux=aux,
                        ipw_table=tab)
    torch.cuda.synchronize()
    out = dict(scores=eng.scores.cpu().numpy(), dscores=eng.dscores.cpu().numpy(), sc=sc.cpu().numpy(), grads=eng.grads[: shape.n_params].cpu().numpy(),
               tail=eng.grads[shape.n_params:].cpu().numpy(), params=p.cpu().numpy(), state=st.cpu().numpy(),
               aux=None if aux is None else aux.cpu().numpy())
    eng.close()
    return out


@pytest.mark.parametrize("algo", ("pairdebias", "lambdarank", "prs"))
def test_one_call_step_at_1251_documents(algo):
    """DNN [16, 8] on 12 features, B = 2, L = 1251 through ONE ultr_train_step against the float32 oracle's step (PRSrank: the
    restatement's), at the bars tests/test_gpu_parity.py holds the same quantities to; twice from the same state: the same bits."""
    from oracle import ultr_oracle as O
    from tests import prs_ref
    from tests.test_gpu_parity import gtol
    d = step_inputs(algo)
    L, ids = d["L"], d["ids"].astype(np.int64)
    if algo == "pairdebias":
        ref = O.pairdebias_step(d["params"], d["state"], d["aux"][:L], d["aux"][L:], d["F"], d["hidden"], d["feats"], ids, d["y"], lr=0.05)
    elif algo == "lambdarank":
        ref = O.lambdarank_step(d["params"], d["state"], d["aux"][:L], d["aux"][L:], d["F"], d["hidden"], d["feats"], ids, d["y"], lr=0.05)
    else:
        ref = prs_ref.prs_step(d["params"], d["state"], prs_ref.dnn_forward(d["F"], d["hidden"], d["feats"], ids), d["y"], d["ipw"])
    got, again = one_call_step(d), one_call_step(d)
    for k, v in got.items():
        assert v is None or np.array_equal(v.view(np.int32), again[k].view(np.int32)), k
    sc = got["sc"]
    gs = 1.0 if algo == "pairdebias" else 1.0 / float(sc[3])
    gref = ref["grads"]
    figs = {"scores": float(np.abs(got["scores"] - ref["scores"]).max()),
            "loss": abs(float(sc[0]) - ref["loss"]) / max(1.0, abs(ref["loss"])),
            "norm": abs(float(sc[1]) - ref["norm"]) / max(1.0, ref["norm"]),
            "grads_over_max": float(np.abs(got["grads"] * gs - gref).max()) / max(1.0, float(np.abs(gref).max()))}
    print("step %s L%d: %s" % (algo, L, ", ".join("%s %.3e" % kv for kv in figs.items())))
    for k, v in figs.items():
        margins.check("losses_long/step", "%s/%s" % (algo, k), v)
    np.testing.assert_allclose(got["scores"], ref["scores"], atol=1e-5, rtol=0, err_msg="scores")
    assert figs["loss"] <= 1e-5 and figs["norm"] <= 1e-5
    np.testing.assert_allclose(got["grads"] * gs, gref, err_msg="grads", **gtol(gref))
    sel = np.abs(gref) > 1e-6 * max(1.0, float(np.abs(gref).max()))
    np.testing.assert_allclose(got["params"][sel], ref["params"][sel], atol=5e-6, rtol=1e-5, err_msg="params")
    np.testing.assert_allclose(got["state"], ref["state"], rtol=2e-5, atol=2e-6 * float(ref["state"].max()), err_msg="state")
    if algo != "prs":
        np.testing.assert_allclose(got["aux"][:L], ref["t_plus"].ravel(), atol=1e-6, err_msg="t_plus")
        np.testing.assert_allclose(got["aux"][L:], ref["t_minus"].ravel(), atol=1e-6, err_msg="t_minus")


@pytest.mark.parametrize("algo", ("pairdebias", "lambdarank", "prs"))
def test_one_call_step_refuses_before_the_forward(algo):
    """A list neither kernel takes: ultr_train_step returns ULTR_E_UNSUPPORTED with nothing launched - the scores are untouched."""
    from ultra_pytorch_amd import _lib, engine, hip_ops
    d = torch.device("cuda")
    B, L = 1, LR.MAX_LIST[algo] + 1
    shape = hip_ops.DnnShape(STEP_F, STEP_HIDDEN)
    eng = engine.StepEngine(shape, B, L, d, algo=algo)
    eng.scores.fill_(DS_FILL)
    p = torch.zeros(shape.n_params, device=d)
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        eng.train_step(p, torch.zeros_like(p), torch.zeros(1, STEP_F, device=d), 1, torch.zeros(L, B, dtype=torch.int32, device=d),
                       torch.ones(L, B, device=d), aux=torch.ones(2 * L, device=d), ipw_table=torch.ones(8, device=d))
    torch.cuda.synchronize()
    assert bool((eng.scores == DS_FILL).all())
    eng.close()


# ---- 5. a staged engine ----------------------------------------------------------------------------------------------------------------
def test_dlcm_trains_with_lambdarank_at_600_documents():
    """DlcmStepEngine (hidden 8, 12 features), B = 2, L = 600: scores against the float64 twin of tests/dlcm_ref.py, dscores and the
    tail against loss_ref.lambdarank on the engine's scores, the gradient against the twin's backward of those dscores - the bars of
    tests/test_gpu_dlcm.py (1e-5 of the tensor's largest entry) and of tests/loss_ref.py."""
    from tests import dlcm_ref as D
    from ultra_pytorch_amd import engine
    from ultra_pytorch_amd.ranking_model import DLCM
    B, L, Fd, H, heads = 2, 600, 12, 8, 3
    torch.manual_seed(31)
    model = DLCM("hidden_size=%d,num_heads=%d" % (H, heads), Fd)
    rng = np.random.RandomState(32)
    feats = torch.from_numpy(rng.normal(size=(B * L, Fd)).astype(np.float32))
    ids = np.ascontiguousarray(np.arange(B * L, dtype=np.int32).reshape(B, L).T)
    y = rng.randint(0, 5, size=(L, B)).astype(np.float32)
    aux0 = rng.uniform(0.8, 1.2, size=2 * L).astype(np.float32)
    d = torch.device("cuda")
    eng = engine.DlcmStepEngine(model.shape, B, L, d, algo="lambdarank")
    params = model.flat_params.detach().to(d).clone()
    eng.train_step(params, torch.zeros_like(params), feats.to(d), B * L, torch.as_tensor(ids).to(d), dev(y), aux=dev(aux0))
    torch.cuda.synchronize()
    scores = eng.scores.cpu()
    twin = D.twin_from(model.state_dict(), Fd, H, heads)
    with torch.no_grad():
        ref_scores = twin(D.gather(feats, ids))
    e = D.rel_err(scores, ref_scores)
    margins.check("losses_long/dlcm", "scores", e)
    assert e <= D.BAR, ("scores", e)
    case = dict(name="dlcm-lambdarank-L600", algo="lambdarank", B=B, L=L, scores=scores.numpy(), labels=y, aux=aux0, kw={})
    ref = LR.reference(case)
    P = model.shape.n_params
    hold_pair(case, eng.dscores.double().cpu().numpy(), eng.grads[P:].double().cpu().numpy(), "dlcm", ref=ref)
    _, ref_grads = D.reference(model.state_dict(), Fd, H, heads, feats, ids, torch.from_numpy(ref["ds"]))
    grads = eng.grads[:P].cpu()
    for name, shp, off in model.shape.layout():
        n = ref_grads[name].numel()
        e = D.rel_err(grads[off:off + n].view(*shp), ref_grads[name])
        margins.check("losses_long/dlcm", "grad/" + name, e)
        assert e <= D.BAR, (name, e)
    eng.close()


# ---- 6. the plugins --------------------------------------------------------------------------------------------------------------------
class FullLists:
    """A Raw_data look-alike of n_queries full lists of M documents (no PADs): graded labels 0 .. 4, or click-like 0 / 1 labels in
    which every batch of three queries has position 0 both clicked and unclicked (PairDebias' EM ratios divide by the position-0 sums)."""

    def __init__(self, n_queries, M, F_, seed, clicks=False):
        rng = np.random.RandomState(seed)
        self.feature_size, self.rank_list_size = F_, M
        self.features = rng.uniform(-1, 1, size=(n_queries * M, F_)).astype(np.float32).tolist() + [[0.0] * F_]
        self.initial_list = [list(range(q * M, (q + 1) * M)) for q in range(n_queries)]
        self.labels, self.qids, self.dids = [], ["q%d" % q for q in range(n_queries)], ["d%d" % i for i in range(n_queries * M)]
        for q in range(n_queries):
            lab = (rng.uniform(size=M) < 0.3).astype(int) if clicks else rng.randint(0, 5, size=M)
            if clicks:
                lab[0], lab[1] = (0, 1) if q % 3 == 0 else (1, 0)
            self.labels.append([int(v) for v in lab])


@pytest.mark.parametrize("algo", ("lambdarank", "pairdebias"))
def test_plugin_trains_and_validates_on_700_documents(algo, monkeypatch):
    """learning_algorithm.LambdaRank / PairDebias + ranking_model.DNN + the host DirectLabelFeed on 6 queries of 700 documents: two
    train() calls, each the engine-level step on the same batch bit for bit, then validation()."""
    from tests.test_gpu_plugins import build
    from ultra_pytorch_amd import engine, input_layer
    from ultra_pytorch_amd.utils import metrics
    monkeypatch.setattr(metrics.RankingMetricKey, "MAX_LABEL", 4.0 if algo == "lambdarank" else 1.0)
    L, B, Fp = 700, 3, 12
    ds = FullLists(6, L, Fp, seed=41, clicks=(algo == "pairdebias"))
    alg = build(dict(algo=algo, hidden=[16, 8], L=L, F=Fp))
    feed = input_layer.DirectLabelFeed(alg, B, "")
    kw = dict(learning_rate=alg.learning_rate, max_gradient_norm=float(alg.hparams.max_gradient_norm), optimizer="ada",
              l2_loss=float(getattr(alg.hparams, "l2_loss", 0.0)))
    kw.update(alg._engine_kwargs())
    eng = engine.StepEngine(alg.model.shape, B, L, torch.device("cuda"), algo=algo, **kw)
    p, st, t = alg.model.flat_params.detach().clone(), alg.state_sum.clone(), alg.t_state.clone()
    for step in range(2):
        input_feed, _ = feed.get_next_batch(step * B, ds, check_validation=False)
        loss, out, summary = alg.train(input_feed)
        assert out is None and np.isfinite(loss)
        x, ids, y = alg.letor_features.clone(), alg.docid_inputs.clone(), alg.labels_LB.clone()
        assert tuple(ids.shape) == (L, B)
        eng.train_step(p, st, x, alg.n_docs, ids, y, aux=t)
        assert eng.read_loss() == loss
        torch.cuda.synchronize()
        for a, b in ((p, alg.model.flat_params), (st, alg.state_sum), (t, alg.t_state)):
            assert torch.equal(a.view(torch.int32), b.detach().view(torch.int32))
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(t).all())
    assert alg.global_step == 2
    input_feed, _ = feed.get_next_batch(0, ds, check_validation=False)
    _, scores, summary = alg.validation(input_feed)
    assert scores.numel() >= B * L and bool(torch.isfinite(scores).all())
    for n in (1, 3, 5, 10):
        assert 0.0 <= summary["ndcg_%d" % n] <= 1.0
    assert summary["ndcg_10"] > 0.0
    eng.close()


# ---- 7. the workspace contract -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ("pairdebias", "lambdarank", "prs"))
def test_long_kernels_stay_inside_the_loss_workspace(algo):
    """B = 2, L = 1251 on the guarded arena of tests/guarded.py (exact lengths, NaN bands), two steps bit for bit against a plain
    run: the long kernels write ultr_loss_part_count partials of ultr_loss_workspace_bytes and nothing else."""
    from tests.test_gpu_workspace_bounds import hold_dnn
    hold_dnn(step_inputs(algo), "%s B%d L%d long list" % (algo, STEP_B, LR.MSLR))
