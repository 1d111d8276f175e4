"""twotower_kernel (csrc/ultr_twotower.hip) and the ULTR_ALGO_TWOTOWER branch of the update launch (csrc/ultr_update.hip) against the
float64 twin tests/twotower_ref.py, at the project's own bars (tests/loss_ref.py; Adam: tests/adam_ref.py).

Kernel: both combinations at B = 3 and L in {1, 2, 63, 64, 65, 129, 256}; scores and theta at unit scale, x 8 and x 30 (both towers
saturate, with both signs); binary, graded (2, 4 clamp to 1) and fractional clicks, a list without a click and an all-clicked one;
PADs masked and not; 1100 lists (the two-level fold); the longest list the layout takes and one document past it; additivity and
determinism on the device.  Steps: loss -> backward -> update on loss_ref's toy DNN through the one-call path, three consecutive
steps from one state, every optimizer x max_gradient_norm {5, 0.01, 0} x l2_loss {0, 0.01} x propensity_learning_rate set / unset.

Every step is checked from the inputs the GPU itself had (the twin is put where the device stands and is fed the device's float32
gradient): what separates the two is then the float32 rounding of this step's own operations - the design of tests/test_gpu_adam.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import adam_ref as A  # noqa: E402
from tests import loss_ref as R  # noqa: E402
from tests import twotower_ref as T  # noqa: E402

F0 = R.TAIL_FIXED
COMBINATIONS = ("product", "sum")


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def run_kernel(s, th, y, comb, ids=None, n_docs=0):
    """(dscores [B, L], the per-list partial tails summed in float64 [4 + 2L], the raw return code) of one ultr_twotower_loss."""
    from ultra_pytorch_amd import hip_ops
    B, L = s.shape
    tail = hip_ops.tail_floats(L)
    ds = torch.full((B, L), 7.0, device="cuda")
    ws = torch.zeros(hip_ops.loss_workspace_bytes(B, L) // 4, device="cuda")
    hip_ops.twotower_loss(dev(s), dev(y), dev(th), B, L, ds, ws, combination=comb, docids=None if ids is None else dev(ids, torch.int32),
                          n_docs=n_docs)
    torch.cuda.synchronize()
    parts = ws[:hip_ops.loss_part_count(B) * tail].view(-1, tail).cpu().numpy().astype(np.float64)
    return ds.cpu().numpy(), parts.sum(0)


def hold_parts(tag, ds, tail, ref):
    e_ds = T.excess(ds, ref["ds"], ref["ds_abs"])
    e_tail = T.excess(tail, ref["tail"], ref["tail_abs"])
    print("%s: dscores %.3e, tail %.3e of (|ref| + terms) (bar %.0e)" % (tag, e_ds, e_tail, R.TERMS_RTOL))
    assert e_ds <= R.TERMS_RTOL, (tag, "dscores", e_ds)
    assert e_tail <= R.TERMS_RTOL, (tag, "tail", e_tail)
    assert tail[1] == ref["tail"][1] and not tail[2:F0].any()
    B = ref["tail"][1]
    assert abs(tail[0] / B - ref["loss"]) <= R.SCALAR_RTOL * max(1.0, abs(ref["loss"])), (tag, "loss")


@pytest.mark.parametrize("comb", COMBINATIONS)
@pytest.mark.parametrize("L", T.LENGTHS)
def test_kernel_against_the_twin(comb, L):
    for scale in T.SCALES:
        for labels in T.LABEL_KINDS:
            s, th, y = T.make_case(L, scale, labels)
            ds, tail = run_kernel(s, th, y, comb)
            hold_parts("%s L%d x%g %s" % (comb, L, scale, labels), ds, tail, T.loss_parts(s, y, th, comb))
            assert not tail[F0 + L:].any()  # the second half of the per-position words is not this algorithm's


def padded_case(L=70):
    """Four lists: a full one, PADs at the tail of two (ids n_docs, beyond n_docs and negative) and an all-PAD one."""
    B = 4
    s, th, y = T.make_case(L, 8.0, "fractional", B=B, seed=5)
    y[:, 1] = (np.arange(L) % 2).astype(np.float32)  # (make_case's all-clicked list: click some PADs too)
    n_docs = B * L
    ids = np.arange(B * L, dtype=np.int32).reshape(L, B)
    ids[L - 7:, 1] = n_docs
    ids[L - 1, 1] = n_docs + 5
    ids[L - 30:, 2] = n_docs
    ids[L - 2, 2] = -1
    ids[:, 3] = n_docs
    return s, th, y, ids, n_docs


@pytest.mark.parametrize("comb", COMBINATIONS)
def test_masked_padding_is_exactly_absent_and_unmasked_padding_counts(comb):
    s, th, y, ids, n_docs = padded_case()
    L = s.shape[1]
    ds, tail = run_kernel(s, th, y, comb, ids, n_docs)
    ref = T.loss_parts(s, y, th, comb, ids, n_docs)
    hold_parts(comb + " masked", ds, tail, ref)
    live = ref["live"]
    assert not live[3].any() and live[0].all() and live[1].sum() == L - 7 and live[2].sum() == L - 30
    assert (ds[~live] == 0.0).all() and (ds[live] != 0.0).mean() > 0.5  # (a saturated sigmoid may round a live entry to 0)
    # theta's gradient holds the live entries only: the same kernel on the live entries alone, PAD rows cut away list by list
    only = np.zeros(L)
    for b in range(3):
        n = int(live[b].sum())
        _, t1 = run_kernel(s[b:b + 1, :n], th[:n], y[:n, b:b + 1], comb)
        only[:n] += t1[F0:F0 + n]
    assert T.excess(tail[F0:F0 + L], only, ref["tail_abs"][F0:F0 + L]) <= R.TERMS_RTOL
    assert tail[1] == 4.0  # D counts lists, the all-PAD one too
    # mask_padding off: every position is an unclicked or clicked document
    ds2, tail2 = run_kernel(s, th, y, comb)
    hold_parts(comb + " unmasked", ds2, tail2, T.loss_parts(s, y, th, comb))
    assert ds2[~live].any() and np.array_equal(ds2[live], ds[live])


def test_longest_list_and_one_document_past_it():
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    lo, hi = 1, 1 << 20  # the bound by asking: the largest L ultr_loss_lds_bytes accepts
    assert int(lib.ultr_loss_lds_bytes(_lib.ALGO_TWOTOWER, lo)) > 0 and int(lib.ultr_loss_lds_bytes(_lib.ALGO_TWOTOWER, hi)) == -2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if int(lib.ultr_loss_lds_bytes(_lib.ALGO_TWOTOWER, mid)) >= 0 else (lo, mid)
    longest = lo
    for comb in COMBINATIONS:
        s, th, y = T.make_case(longest, 8.0, "binary", B=2)
        ds, tail = run_kernel(s, th, y, comb)
        hold_parts("%s L%d" % (comb, longest), ds, tail, T.loss_parts(s, y, th, comb))
    L = longest + 1
    s = torch.zeros(1, L, device="cuda")
    ds = torch.full((1, L), 7.0, device="cuda")
    ws = torch.zeros(hip_ops.loss_workspace_bytes(1, L) // 4, device="cuda")
    rc = lib.ultr_twotower_loss(s.data_ptr(), s.data_ptr(), s.data_ptr(), 0, None, 0, 1, L, ds.data_ptr(), ws.data_ptr(), hip_ops.raw_stream())
    assert rc == -2  # ULTR_E_UNSUPPORTED, on the host
    torch.cuda.synchronize()
    assert (ds == 7.0).all() and not ws.any()
    # bad arguments: nothing launched either
    for bad in (dict(comb=2), dict(B=0), dict(ndocs=-1)):
        ids = torch.zeros(1, L - 1, dtype=torch.int32, device="cuda")
        rc = lib.ultr_twotower_loss(s.data_ptr(), s.data_ptr(), s.data_ptr(), bad.get("comb", 0), ids.data_ptr(), bad.get("ndocs", 5),
                                    bad.get("B", 1), L - 1, ds.data_ptr(), ws.data_ptr(), hip_ops.raw_stream())
        assert rc == -1, bad
    torch.cuda.synchronize()
    assert (ds == 7.0).all() and not ws.any()


# ---- whole steps on the toy DNN ------------------------------------------------------------------------------------------------
class Step:
    """An engine of the one-call path (ultr_train_step) on loss_ref's toy DNN with its state on the device."""

    def __init__(self, B, L, hyper, seed=0, state="rand"):
        from oracle import ultr_oracle as O
        from ultra_pytorch_amd import engine, hip_ops
        self.B, self.L, self.h = B, L, hyper
        rng = np.random.RandomState(seed)
        self.n_docs = B * L - 3
        self.feats = rng.uniform(-1, 1, size=(self.n_docs, R.TOY_F)).astype(np.float32)
        ids = rng.permutation(B * L)
        self.ids = np.where(ids >= self.n_docs, self.n_docs, ids).astype(np.int32).reshape(L, B)
        y = rng.choice(np.array([0.0, 0.0, 1.0, 1.0, 0.5, 3.0], np.float32), size=(L, B))
        self.labels = y
        params = O.init_params(R.TOY_F, R.TOY_HIDDEN, seed=seed % 1000) + rng.uniform(-0.2, 0.2, size=O.num_params(R.TOY_F, R.TOY_HIDDEN))
        self.shape = hip_ops.DnnShape(R.TOY_F, R.TOY_HIDDEN, "elu")
        self.P = self.shape.n_params
        self.eng = engine.StepEngine(self.shape, B, L, torch.device("cuda"), algo="twotower", optimizer=hyper["optimizer"],
                                     learning_rate=hyper["learning_rate"], max_gradient_norm=hyper["max_gradient_norm"],
                                     propensity_learning_rate=hyper["plr_given"], l2_loss=hyper["l2_loss"],
                                     tower_combination=hyper["tower_combination"], mask_padding=hyper["mask_padding"])
        n = engine.opt_state_floats("twotower", hyper["optimizer"], L, self.P)
        assert n == T.state_floats(hyper["optimizer"], self.P, L)
        st = np.zeros(max(n, 1), np.float32)
        if state == "rand" and hyper["optimizer"] == "ada":
            st = (0.01 * rng.uniform(size=n)).astype(np.float32)
        self.p, self.st = dev(params.astype(np.float32)), dev(st)
        self.theta = dev(rng.normal(size=L).astype(np.float32))
        self.d_feats, self.d_ids, self.d_labels = dev(self.feats), dev(self.ids, torch.int32), dev(self.labels)
        self.t = 0
        self.twin = T.dnn_twin(params, self.theta.cpu().numpy(), hyper, R.TOY_F, R.TOY_HIDDEN, self.feats, self.ids)

    def host(self):
        return self.p.cpu().numpy(), self.st.cpu().numpy(), self.theta.cpu().numpy()

    def step(self):
        self.t += 1
        self.eng.set_opt_step(self.t)
        self.eng.train_step(self.p, self.st, self.d_feats, self.n_docs, self.d_ids, self.d_labels, aux=self.theta)
        torch.cuda.synchronize()
        e = self.eng
        g = e.grads.cpu().numpy()
        return dict(g=g[:self.P], tail=g[self.P:], sc=e.scalars.cpu().numpy(), scores=e.scores.cpu().numpy(), ds=e.dscores.cpu().numpy(),
                    loss=e.read_loss())


def hold_step(tag, run, before, out, after):
    """One step of `run` against the twin put at `before` and fed the device's float32 gradients."""
    h, P, L, B, t = run.h, run.P, run.L, run.B, run.t
    p0, st0, th0 = before
    p1, st1, th1 = after
    masked = h["mask_padding"]
    # the loss kernel, on the device's own scores
    ref = T.loss_parts(out["scores"], run.labels, th0, h["tower_combination"], run.ids if masked else None, run.n_docs)
    hold_parts(tag + " kernel", out["ds"], out["tail"].astype(np.float64), ref)
    # the step
    D = float(out["tail"][1])
    assert D == B
    n_state = T.state_floats(h["optimizer"], P, L)
    tw = run.twin
    tw.load(p0, th0, st0[:n_state], t - 1)
    g64, tg64 = out["g"].astype(np.float64) / D, out["tail"][F0:F0 + L].astype(np.float64) / D
    r = tw.step(run.labels, run.ids, run.n_docs, force_grad=g64, force_theta_grad=tg64)
    # the ranker's gradient itself against autograd through the oracle's DNN: smoke()'s bar for it (rtol 1e-4, atol 1e-6) - the DNN
    # backward is not what this file tests
    np.testing.assert_allclose(out["scores"], r["scores"], atol=1e-5)
    np.testing.assert_allclose(g64, r["grad"], rtol=1e-4, atol=1e-6)
    # the eight scalars
    sc = out["sc"]
    ss = float((out["g"].astype(np.float64) ** 2).sum())
    want = dict(loss=r["loss"], norm=r["norm"], coef=r["coef"], D=float(B), rank_loss=0.0, exam_loss=0.0, pnorm=r["pnorm"], ss=ss)
    for k, name in enumerate(("loss", "norm", "coef", "D", "rank_loss", "exam_loss", "pnorm", "ss")):
        assert abs(float(sc[k]) - want[name]) <= R.SCALAR_RTOL * max(1.0, abs(want[name])), (tag, name, float(sc[k]), want[name])
    assert float(sc[3]) == B and sc[4] == 0.0 and sc[5] == 0.0
    assert out["loss"] == float(sc[0])  # what the host reads (the early report included) is scalars[0]
    # parameters, theta, state
    ref_p, ref_th, ref_st = tw.flat(), tw.theta.detach().numpy(), tw.state()
    e_th = float(np.abs(th1 - ref_th).max())
    assert np.isfinite(th1).all() and e_th <= R.AUX_ATOL, (tag, "theta", e_th)
    if h["optimizer"] == "adam":
        e_p = A.excess(p1, ref_p, h["learning_rate"])
        terms = np.concatenate([(1 - A.B1) * r["g_terms"], (1 - A.B2) * r["g_terms"] ** 2, (1 - A.B1) * np.abs(r["theta_final"]),
                                (1 - A.B2) * r["theta_final"] ** 2])
        e_s = A.moment_excess(st1, ref_st, st0, terms)  # (all four in the device layout: m | v | m_theta | v_theta)
        print("%s t=%d: parameters %.3e (bar %.3e), moments %.3e (bar %.3e), theta %.3e" % (tag, t, e_p, A.BAR, e_s, A.MOMENT_RTOL, e_th))
        assert e_p <= A.BAR and e_s <= A.MOMENT_RTOL, (tag, e_p, e_s)
        assert A.excess(th1, ref_th, h["propensity_learning_rate"]) <= A.BAR
    else:
        e_p = float(np.abs(p1 - ref_p).max())
        print("%s t=%d: parameters %.3e (bar %.3e), theta %.3e (bar %.0e)" % (tag, t, e_p, R.PARAM_ATOL, e_th, R.AUX_ATOL))
        assert np.isfinite(p1).all() and e_p <= R.PARAM_ATOL, (tag, "params", e_p)
        if h["optimizer"] == "ada":
            e_s = float((np.abs(st1 - ref_st) / np.maximum(ref_st, 1e-30)).max())  # relative to the accumulator, as tests/test_gpu_losses.py
            print("%s t=%d: accumulators %.3e (bar %.3e)" % (tag, t, e_s, R.STATE_RTOL))
            assert e_s <= R.STATE_RTOL, (tag, "state", e_s)
        else:
            assert np.array_equal(st1, st0)  # SGD keeps no state
    return r, sc


def hyper(opt, mg, l2, plr, comb="product", mask=True):
    h = T.hyper_of(optimizer=opt, max_gradient_norm=mg, l2_loss=l2, propensity_learning_rate=plr, tower_combination=comb, mask_padding=mask)
    h["plr_given"] = plr
    return h


@pytest.mark.parametrize("l2", [0.0, 0.01])
@pytest.mark.parametrize("mg", [5.0, 0.01, 0.0])
@pytest.mark.parametrize("opt", ["ada", "sgd", "adam"])
def test_three_steps_hold_every_parameter_state_word_theta_and_scalar(opt, mg, l2):
    """propensity_learning_rate unset (-1: the learning rate) with the product, set (0.2) with the sum and unmasked PADs.  SGD runs at
    a clip that bites for the observation tower too (its gradient norm is of order 0.1)."""
    for plr, comb, mask in ((-1.0, "product", True), (0.2, "sum", False)):
        h = hyper(opt, mg, l2, plr, comb, mask)
        run = Step(R.HB, R.HL, h, seed=17 + int(100 * l2))
        th_start = run.theta.cpu().numpy()
        for _ in range(3):
            before = run.host()
            out = run.step()
            r, sc = hold_step("%s mg%g l2%g %s" % (opt, mg, l2, comb), run, before, out, run.host())
            if mg == 0.0:
                assert sc[2] == 1.0 and r["pcoef"] == 1.0
            if mg == 0.01:  # the clip bites, for both towers - with l2_loss > 0 too (this algorithm keeps its clip)
                assert sc[2] < 1.0 and r["coef"] < 1.0 and r["pcoef"] < 1.0 and sc[1] > mg and sc[6] > mg
            if l2 > 0:
                assert r["norm"] != pytest.approx(float(np.sqrt(sc[7])) / run.B, rel=1e-9)  # the norm covers the L2 term
        assert (run.theta.cpu().numpy() != th_start).all()
        assert run.eng.udesc.propensity_learning_rate == np.float32(0.2 if plr > 0 else h["learning_rate"])


@pytest.mark.parametrize("opt", ["ada", "adam"])
def test_many_lists_fold_in_two_levels(opt):
    """1100 lists at L = 33: more than 1024 partials and a 70-word tail (loss_ref.MANY)."""
    h = hyper(opt, 5.0, 0.0, -1.0)
    run = Step(1100, R.MANY_L, h, seed=3)
    before = run.host()
    out = run.step()
    hold_step("many " + opt, run, before, out, run.host())


@pytest.mark.parametrize("comb", COMBINATIONS)
def test_halves_add_up_on_the_device_and_runs_repeat_bitwise(comb):
    """The folded tail of a batch against the folded tails of its two halves (D adds exactly), and two runs from one state."""
    h = hyper("ada", 5.0, 0.0, -1.0, comb)
    whole = Step(6, R.HL, h, seed=9)
    folded = {}
    for name, lo, hi in (("whole", 0, 6), ("a", 0, 2), ("b", 2, 6)):
        run = whole if name == "whole" else Step(hi - lo, R.HL, h, seed=9)
        ids, y = dev(whole.ids[:, lo:hi], torch.int32), dev(whole.labels[:, lo:hi])
        run.eng.forward(run.p, whole.d_feats, whole.n_docs, ids, train=True)  # (the backward wants a record of a forward)
        run.eng.scores.copy_(dev(T.make_case(R.HL, 8.0, "fractional", B=6, seed=1)[0][lo:hi]))  # saturating scores for the loss
        run.eng.loss(y, aux=whole.theta, docids=ids, n_docs=whole.n_docs)
        run.eng.backward(run.p, whole.d_feats, whole.n_docs, ids)
        torch.cuda.synchronize()
        folded[name] = run.eng.grads[run.P:].cpu().numpy().astype(np.float64)
    s = T.make_case(R.HL, 8.0, "fractional", B=6, seed=1)[0]
    ref = T.loss_parts(s, whole.labels, whole.theta.cpu().numpy(), comb, whole.ids, whole.n_docs)
    assert T.excess(folded["a"] + folded["b"], folded["whole"], ref["tail_abs"]) <= R.TERMS_RTOL
    assert folded["a"][1] + folded["b"][1] == folded["whole"][1] == 6.0
    assert T.excess(folded["whole"], ref["tail"], ref["tail_abs"]) <= R.TERMS_RTOL
    # two runs from the same state: the same bits everywhere
    ends = []
    for _ in range(2):
        run = Step(R.HB, R.HL, h, seed=21)
        outs = [run.step() for _ in range(2)]
        ends.append([a.view(np.uint32) for a in run.host()] + [outs[-1]["sc"][:8].view(np.uint32), outs[-1]["ds"].view(np.uint32)])
    assert all(np.array_equal(a, b) for a, b in zip(*ends))
