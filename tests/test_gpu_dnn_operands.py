"""The DNN entry points off the aligned operand route, against the float64 restatement (tests/dnn_ref.py).

dnn_route (csrc/ultr_dnn.hip) picks every DNN kernel from the shape AND from what the call knows of its operands: params / features
on a 16-byte boundary, the weight copies present (and aligned), a dscores buffer.  The rest of the suite moves the shape only.  Here
each operand fact is cleared, alone (params and features also together), on the smallest shapes at which each decision exists
(tests/dnn_operand_cases.py), and every public DNN call is held to the project's bars against float64:

    scores   atol = rtol = 1e-5        loss   1e-5 max(1, |loss|)        gradients, per entry   1e-5 (|g| + sum |terms|)
    updated parameters / state: as tests/test_gpu_planner_sweep.py holds them against the oracle (rtol 1e-4, atol 1e-5 where the
    gradient is not ~0 - a fresh Adagrad step is sign-like; DLA's propensity parameters atol 2e-5)

Misaligned inputs are slices of a larger buffer whose other words hold the NaN pattern of tests/guarded.py (read: NaN results; written:
the pattern check fails); outputs are views of a guarded arena exactly as long as the size queries say, checked after every call.
Every call runs twice and must give the same bits.  Each case first asks ultr_dnn_route_operands what the call takes and asserts
that clearing the operand moved the route where it was meant to.

The operand contract (include/ultr_hip.h, ultr_dnn_forward): params / features at any 4-byte aligned address; a weight copy off a
16-byte boundary counts as absent where it is read and is refused (ULTR_E_BADARG, nothing launched) where it must be written.

One thing the ABI cannot express: a backward WITH the copies behind a forward WITHOUT them - only ultr_train_step hands the copies to
the backward, and it runs its own forward with the same ones.  test_forward_and_backward_on_different_routes covers the pairs there
are: forward without / with the copies in front of the public backward (which never sees them), and whole steps with / without."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import dnn_operand_cases as C
from tests import guarded as G
from tests import margins

pytestmark = pytest.mark.gpu

RATIOS = {}   # variant -> (largest error-to-bar ratio, where)
ROUTES = {}   # variant -> set of route descriptions reached
CASE_IDS = [C.case_id(c) for c in C.CASES]
PAD_WORDS = 64

# default plan (mfma_mode split_half): the (shape index, operand group) pairs whose route MUST differ from the aligned one
DIFFERS = {"pointer": {0, 1, 2, 3, 5}, "wt": {1, 2, 3, 5}, "dscores": {5}}


def note(variant, what, ratio, mode="split_half"):
    print("%-22s %-60s error / bar = %.3f" % (variant, what, ratio))
    margins.check("dnn_operands/%s" % variant, "%s/%s" % (what, mode), ratio)
    if ratio > RATIOS.get(variant, (-1.0, ""))[0]:
        RATIOS[variant] = (ratio, what)
    assert ratio <= 1.0, (variant, what, ratio)


def sliced(arr, byte_off):
    """arr as a slice, byte_off bytes past a 16-byte boundary, of a larger device buffer filled with the NaN pattern."""
    a = np.ascontiguousarray(arr).reshape(-1)
    assert a.dtype == np.float32 and byte_off % 4 == 0
    buf = torch.full((a.size + 2 * PAD_WORDS,), G._PATTERN_I32, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    start = PAD_WORDS + byte_off // 4
    view = buf[start:start + a.size].view(torch.float32)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == byte_off and view.is_contiguous()
    return buf, view


def around_is_untouched(buf, view):
    start = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:start] == G._PATTERN_I32).all()) and bool((buf[start + view.numel():] == G._PATTERN_I32).all())


class Operands:
    """The inputs of case k on the device under an operand variant."""

    def __init__(self, k, variant):
        from ultra_pytorch_amd import hip_ops
        d, v = C.inputs(k), C.VARIANTS[variant]
        self.k, self.variant, self.d, self.v = k, variant, d, v
        self.F, self.hidden, self.B, self.L, self.act = d["F"], d["hidden"], d["B"], d["L"], d["act"]
        self.shape = hip_ops.DnnShape(self.F, self.hidden, self.act)
        self.lib = self.shape.lib
        self.lib.ultr_config_reload()  # (the knobs of the mfma_mode fixture)
        self.P, self.N, self.n_docs = self.shape.n_params, self.B * self.L, d["feats"].shape[0]
        assert self.P == d["params"].size
        self.params_buf, self.params = sliced(d["params"], v.get("params", 0))
        self.feats_buf, self.feats = sliced(d["feats"], v.get("features", 0))
        self.ids = torch.from_numpy(d["ids"].astype(np.int32)).cuda()
        self.labels = torch.from_numpy(d["y"].astype(np.float32)).cuda()
        self.ipw = torch.from_numpy(C.IPW).cuda()
        self.wt_buf = self.wt = None
        if v.get("wt", 0) is not None:
            n = int(self.lib.ultr_dnn_wt_floats(ctypes.byref(self.shape.desc)))
            self.wt_buf, self.wt = sliced(np.zeros(n, np.float32), v.get("wt", 0))  # (alignment gaps of the copies stay zero)
            self.build_wt(self.wt)
        self.has_dscores = v.get("dscores", True)

    def build_wt(self, into):
        from ultra_pytorch_amd import _lib, hip_ops
        _lib.check(self.lib.ultr_dnn_build_wt(ctypes.byref(self.shape.desc), self.params.data_ptr(), into.data_ptr(), hip_ops.raw_stream()),
                   "ultr_dnn_build_wt")

    def inputs_untouched(self, params_too=True):
        ok = around_is_untouched(self.feats_buf, self.feats) and around_is_untouched(self.params_buf, self.params)
        ok = ok and torch.equal(self.feats.cpu(), torch.from_numpy(self.d["feats"]).reshape(-1))
        if params_too:
            ok = ok and torch.equal(self.params.cpu(), torch.from_numpy(self.d["params"]))
        if self.wt_buf is not None:
            ok = ok and around_is_untouched(self.wt_buf, self.wt)
        return ok

    def outputs(self):
        """Arena views of every buffer the library writes: poisoned where the engines allocate with torch.empty, zeroed where they zero."""
        from ultra_pytorch_amd import hip_ops
        tail = hip_ops.tail_floats(self.L)
        sizes = dict(saved=max(self.shape.saved_bytes(self.N) // 4, 1), bwd_ws=max(self.shape.bwd_workspace_bytes(self.N) // 4, 1),
                     scores=self.N, dscores=self.N, loss_ws=max(hip_ops.loss_workspace_bytes(self.B, self.L) // 4, 1),
                     grads=self.P + tail, scalars=16)
        arena = G.Arena(torch.device("cuda"), G.bytes_for([4 * n for n in sizes.values()]))
        out = {name: arena.view(n, zero=name in ("loss_ws", "grads", "scalars"), name=name) for name, n in sizes.items()}
        out["arena"] = arena
        return out

    # ---- routes ----------------------------------------------------------------------------------------------------------
    def route(self, call, variant=None, without=()):
        from ultra_pytorch_amd import _lib
        bits = [b for b in C.operand_bits(self.variant if variant is None else variant) if b not in without]
        r = self.shape.route(self.B, self.L, n_docs=self.n_docs, call=call, operands=bits)
        return dict(r, fwd=_lib.DNN_FAMILIES[r["fwd"]], bwd=_lib.DNN_FAMILIES[r["bwd"]], loss=_lib.DNN_LOSS_PLACES[r["loss"]])

    def hold_route(self, call, mode, without=()):
        """The route of `call` under this variant moved from the aligned one as meant; returns a description of it."""
        full, r = self.route(call, "aligned", without), self.route(call, without=without)
        v, si = self.v, C.CASES[self.k][0]
        if "params" in v or "features" in v:
            assert r["fused_waves"] == 0 and r["fwd"] == "tile" and r["bwd"] in ("none", "tile") and r["wg_split_half"] == 0, r
            group = "pointer"
        elif "wt" in v:
            if self.hidden:
                assert r["fused_waves"] == 0 and r["fwd"] == "tile" and r["bwd"] != "wide", r
            group = "wt"
        elif "dscores" in v:
            if call == "step_softmax" and r["fused_waves"] == 0:
                assert r["bwd"] in ("tile", "tile2") and r["loss"] == "prologue", r
            group = "dscores"
        else:
            group = None
        if group is not None and mode == "split_half" and call == "step_softmax" and not without:
            assert (r != full) == (si in DIFFERS[group]), (self.variant, call, full, r)
        text = "%s: fwd %s%d, bwd %s%d, loss %s%s" % (call, r["fwd"], r["fwd_rows"], r["bwd"], r["bwd_rows"], r["loss"],
                                                      ", fused on %d waves" % r["fused_waves"] if r["fused_waves"] else "")
        ROUTES.setdefault(self.variant, set()).add("%s [%s] %s" % (C.case_id(C.CASES[self.k]), mode, text))
        return r

    # ---- calls -----------------------------------------------------------------------------------------------------------
    def forward(self, out, train):
        from ultra_pytorch_amd import _lib, hip_ops
        rc = self.lib.ultr_dnn_forward(ctypes.byref(self.shape.desc), self.params.data_ptr(), self.wt.data_ptr() if self.wt is not None else None,
                                       self.feats.data_ptr(), self.n_docs, self.ids.data_ptr(), self.B, self.L, out["scores"].data_ptr(),
                                       out["saved"].data_ptr() if train else None, hip_ops.raw_stream())
        _lib.check(rc, "ultr_dnn_forward")
        torch.cuda.synchronize()
        out["arena"].check()
        return out["scores"].view(self.B, self.L).cpu().numpy()

    def backward(self, out, fused_loss):
        """ultr_softmax_ce + ultr_dnn_backward, or ultr_dnn_backward_softmax (dscores_out NULL under the dscores_null variant), behind a
        training forward into out; returns (loss, gradient of the loss [P])."""
        from ultra_pytorch_amd import hip_ops
        feats = self.feats.view(self.n_docs, self.F)
        sc = out["scores"].view(self.B, self.L)
        if fused_loss:
            hip_ops.dnn_backward_softmax(self.shape, self.params, feats, self.n_docs, self.ids, self.B, self.L, out["saved"], sc, self.labels,
                                         out["loss_ws"], out["bwd_ws"], out["grads"], ipw_table=self.ipw,
                                         dscores_out=out["dscores"] if self.has_dscores else None)
        else:
            hip_ops.softmax_ce(sc, self.labels, self.B, self.L, out["dscores"], out["loss_ws"], ipw_table=self.ipw)
            hip_ops.dnn_backward(self.shape, self.params, feats, self.n_docs, self.ids, self.B, self.L, out["saved"], out["dscores"],
                                 out["loss_ws"], out["bwd_ws"], out["grads"])
        torch.cuda.synchronize()
        out["arena"].check()
        g = out["grads"].cpu().numpy().astype(np.float64)
        D = g[self.P + 1]
        return g[self.P] / D, g[:self.P] / D

    def step_args(self, out, algo, aux=None, state=None, skip_update=0):
        from ultra_pytorch_amd import _lib
        u = _lib.UpdateDesc()
        u.algo = {"softmax": _lib.ALGO_SOFTMAX, "dla": _lib.ALGO_DLA}[algo]
        u.optimizer, u.list_size, u.logits_to_prob, u.n_params = _lib.OPT_ADAGRAD, self.L, 0, self.P
        u.learning_rate, u.max_gradient_norm, u.adagrad_eps, u.ranker_loss_weight = 0.05, 5.0, 1e-10, 1.0
        u.propensity_learning_rate, u.em_step_size, u.regulation_p, u.l2_loss = 0.05, 0.05, 1.0, 0.0
        u.guard = u.range_flag = u.host_scalars = None
        u.seq, u.adam_t = 1, 0
        a = _lib.StepArgs()
        a.desc, a.upd = ctypes.pointer(self.shape.desc), ctypes.pointer(u)
        a.params, a.wt = self.params.data_ptr(), self.wt.data_ptr() if self.wt is not None else None
        a.state = state.data_ptr() if state is not None else None
        a.aux = aux.data_ptr() if aux is not None else None
        a.features, a.n_docs, a.docids, a.labels = self.feats.data_ptr(), self.n_docs, self.ids.data_ptr(), self.labels.data_ptr()
        if algo == "softmax":
            a.ipw_table, a.n_ipw = self.ipw.data_ptr(), int(self.ipw.numel())
        a.scores, a.dscores = out["scores"].data_ptr(), out["dscores"].data_ptr() if (self.has_dscores or algo != "softmax") else None
        a.saved, a.loss_ws, a.bwd_ws = out["saved"].data_ptr(), out["loss_ws"].data_ptr(), out["bwd_ws"].data_ptr()
        a.grads, a.scalars = out["grads"].data_ptr(), out["scalars"].data_ptr()
        a.batch, a.list_size, a.batch_total, a.skip_update, a.sigma = self.B, self.L, self.B, skip_update, 1.0
        a._keep = (u, out, aux, state)
        return a

    def step(self, a):
        from ultra_pytorch_amd import hip_ops
        rc = self.lib.ultr_train_step(ctypes.byref(a), hip_ops.raw_stream())
        torch.cuda.synchronize()
        return rc


def bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int32).clone()


VAR_FWD = ["aligned", "params+4", "params+8", "params+12", "features+4", "params+4_features+4", "wt_null", "wt+4"]
VAR_BWD = VAR_FWD + ["dscores_null"]
VAR_STEP = ["params+4", "features+4", "params+4_features+4", "wt_null", "dscores_null"]


# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VAR_FWD)
@pytest.mark.parametrize("k", range(len(C.CASES)), ids=CASE_IDS)
def test_forward(k, variant, mfma_mode):
    """ultr_dnn_forward, evaluation and training."""
    op, ref = Operands(k, variant), C.reference(k)
    op.hold_route("eval", mfma_mode)
    op.hold_route("step_dscores", mfma_mode)  # (its forward half is the training forward)
    out = op.outputs()
    for train in (False, True):
        s1 = op.forward(out, train)
        b1 = (bits_of(out["scores"]), bits_of(out["saved"]) if train else None)
        note(variant, "forward_%s/%s" % ("train" if train else "eval", CASE_IDS[k]), C.score_ratio(s1, ref["scores"]), mfma_mode)
        out["scores"].view(torch.int32).fill_(G._PATTERN_I32)
        op.forward(out, train)
        assert torch.equal(bits_of(out["scores"]), b1[0]), "the second run gave other scores"
        if train:
            assert torch.equal(bits_of(out["saved"]), b1[1]), "the second run left other activations in `saved`"
    assert op.inputs_untouched()


@pytest.mark.parametrize("variant", VAR_BWD)
@pytest.mark.parametrize("k", range(len(C.CASES)), ids=CASE_IDS)
def test_backward(k, variant, mfma_mode):
    """ultr_dnn_backward (behind ultr_softmax_ce) and ultr_dnn_backward_softmax behind a training forward under the same variant.  The
    public backward calls never see the weight copies: under the aligned and the wt+4 / wt_null variants the forward and the backward
    route differently and must still agree on `saved`."""
    op, ref = Operands(k, variant), C.reference(k)
    op.hold_route("step_softmax", mfma_mode, without=("wt",))  # what ultr_dnn_backward_softmax takes
    out = op.outputs()
    op.forward(out, True)
    for fused_loss in ((True,) if variant == "dscores_null" else (False, True)):
        name = "backward_softmax" if fused_loss else "softmax_ce+backward"
        loss, g = op.backward(out, fused_loss)
        b1 = bits_of(out["grads"])
        note(variant, "%s_loss/%s" % (name, CASE_IDS[k]), C.loss_ratio(loss, ref["loss"]), mfma_mode)
        note(variant, "%s_grads/%s" % (name, CASE_IDS[k]), C.grad_ratio(g, ref["grads"], ref["terms"]), mfma_mode)
        out["grads"].zero_()
        op.backward(out, fused_loss)
        assert torch.equal(bits_of(out["grads"]), b1), "the second run gave other gradients"
    assert op.inputs_untouched()


@functools.lru_cache(maxsize=None)
def oracle_step(k, algo):
    from oracle import ultr_oracle as O
    d = C.inputs(k)
    if algo == "softmax":
        return O.train_step_softmax(d["params"], np.zeros_like(d["params"]), d["F"], d["hidden"], d["feats"], d["ids"].astype(np.int64), d["y"],
                                    ipw_list=C.IPW, act=d["act"])
    return O.dla_step(d["params"], prop_of(k), d["F"], d["hidden"], d["feats"], d["ids"].astype(np.int64), d["y"], act=d["act"])


def prop_of(k):
    """DLA's propensity parameters [W (L) | bias].  The bias is set so that W_l + bias changes sign along the list: where all are
    positive the ELU of the DenoisingNet is linear, the softmax's shift invariance makes the bias gradient exactly zero, and the
    fresh Adagrad step of the bias - lr g / |g| - is +lr or -lr by rounding alone, on the GPU and in the oracle alike."""
    w = 0.1 * np.random.RandomState(900 + k).randn(C.inputs(k)["L"])
    return np.concatenate((w, [-np.median(w)])).astype(np.float32)


def run_step(k, variant, algo, mode, hold):
    """One ultr_train_step from the case's initial state; returns the bits of everything it wrote (and holds it to the bars)."""
    op, ref = Operands(k, variant), C.reference(k)
    out = op.outputs()
    state = torch.zeros(op.P, dtype=torch.float32, device="cuda") if algo == "softmax" else None
    aux = torch.from_numpy(prop_of(k)).cuda() if algo == "dla" else None
    rc = op.step(op.step_args(out, algo, aux=aux, state=state))
    assert rc == 0, rc
    out["arena"].check()
    assert op.inputs_untouched(params_too=False), "the step wrote around its inputs"
    scal = out["scalars"].cpu().numpy()
    scores = out["scores"].view(op.B, op.L).cpu().numpy()
    p_new = op.params.cpu().numpy()
    if hold:
        o = oracle_step(k, algo)
        op.hold_route("step_softmax" if algo == "softmax" else "step_dscores", mode)
        what = "step_%s" % algo
        note(variant, "%s_scores/%s" % (what, CASE_IDS[k]), C.score_ratio(scores, ref["scores"]), mode)
        if algo == "softmax":
            note(variant, "%s_loss/%s" % (what, CASE_IDS[k]), C.loss_ratio(scal[0], ref["loss"]), mode)
            g = out["grads"][:op.P].cpu().numpy().astype(np.float64) / float(scal[3])
            note(variant, "%s_grads/%s" % (what, CASE_IDS[k]), C.grad_ratio(g, ref["grads"], ref["terms"]), mode)
        else:
            # (DLA's losses have no float64 restatement: the fp32 oracle's, as the sweep holds them)
            note(variant, "%s_loss/%s" % (what, CASE_IDS[k]), C.loss_ratio(scal[0], o["loss"]), mode)
            gq = np.abs(o["prop_grads"])
            assert gq.min() > 1e-3 * gq.max(), "an ill-conditioned case: a propensity gradient of ~0 under a sign-like update"
            np.testing.assert_allclose(aux.cpu().numpy(), o["prop_params"], atol=2e-5)
        # a fresh Adagrad step is sign-like: the updated parameters (and the accumulator) where the gradient is not ~0
        sel = np.abs(o["grads"]) > 1e-3 * np.abs(o["grads"]).max()
        np.testing.assert_allclose(p_new[sel], o["params"][sel], rtol=1e-4, atol=1e-5)
        assert np.isfinite(p_new).all()
        if state is not None:
            np.testing.assert_allclose(state.cpu().numpy()[sel], o["state"][sel], rtol=1e-4, atol=1e-5)
        if op.wt is not None and op.hidden:  # the update kept the copies current
            fresh = torch.zeros_like(op.wt)
            op.build_wt(fresh)
            torch.cuda.synchronize()
            assert torch.equal(bits_of(fresh), bits_of(op.wt)), "the weight copies are not those of the updated parameters"
    return [bits_of(out[n]) for n in ("scores", "grads", "scalars")] + [bits_of(op.params)] + ([bits_of(state)] if state is not None else []) + \
           ([bits_of(aux)] if aux is not None else [])


# (DLA's loss kernel writes dscores: there is no DLA step without the buffer)
STEPS = [(v, a) for v in VAR_STEP for a in ("softmax", "dla") if not (v == "dscores_null" and a == "dla")]


@pytest.mark.parametrize("variant,algo", STEPS, ids=["%s-%s" % s for s in STEPS])
@pytest.mark.parametrize("k", range(len(C.CASES)), ids=CASE_IDS)
def test_train_step(k, variant, algo, mfma_mode):
    """ultr_train_step for SOFTMAX and DLA, the arguments filled as engine.StepEngine fills them; wt NULL or aligned."""
    first = run_step(k, variant, algo, mfma_mode, hold=True)
    again = run_step(k, variant, algo, mfma_mode, hold=False)
    for a, b in zip(first, again):
        assert torch.equal(a, b), "the second run of the step gave other bits"


@pytest.mark.parametrize("algo", ["softmax", "dla"])
@pytest.mark.parametrize("k", [1, 3, 5], ids=[CASE_IDS[1], CASE_IDS[3], CASE_IDS[5]])
def test_step_refuses_a_misaligned_weight_copy(k, algo):
    """ultr_train_step (and ultr_apply_update) must write the copies: ULTR_E_BADARG, and nothing was launched - no output changed."""
    from ultra_pytorch_amd import _lib
    op = Operands(k, "wt+4")
    out = op.outputs()
    state = torch.zeros(op.P, dtype=torch.float32, device="cuda")
    aux = torch.from_numpy(prop_of(k)).cuda() if algo == "dla" else None
    before = {n: bits_of(out[n]) for n in out if n != "arena"}
    wt_before = bits_of(op.wt)
    for skip in (0, 1):
        assert op.step(op.step_args(out, algo, aux=aux, state=state, skip_update=skip)) == -1  # ULTR_E_BADARG
    a = op.step_args(out, algo, aux=aux, state=state)
    rc = op.lib.ultr_apply_update(a.upd, a.desc, op.params.data_ptr(), op.wt.data_ptr(), state.data_ptr(), out["grads"].data_ptr(),
                                  aux.data_ptr() if aux is not None else None, out["bwd_ws"].data_ptr(), out["scalars"].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1
    out["arena"].check()
    for n, b in before.items():
        assert torch.equal(bits_of(out[n]), b), n
    assert op.inputs_untouched() and torch.equal(bits_of(op.wt), wt_before) and not bool(state.any())
    assert _lib.DNN_OPERANDS["wt16"] == 8


@pytest.mark.parametrize("k", [2, 3, 5, 7], ids=[CASE_IDS[2], CASE_IDS[3], CASE_IDS[5], CASE_IDS[7]])
def test_forward_and_backward_on_different_routes(k, mfma_mode):
    """The same gradients whichever side had the weight copies: (a) forward without, public backward; (b) forward with them - the fused
    shapes' stand-alone forward, the wide-tile forward - and the public backward, which never has them; (c) a whole step with the copies
    (fused, or wide forward and backward); (d) a whole step without.  All within the bar of float64, and of each other."""
    ref = C.reference(k)
    got = {}
    for name, variant in (("fwd_null+bwd", "wt_null"), ("fwd_wt+bwd", "aligned")):
        op = Operands(k, variant)
        out = op.outputs()
        op.forward(out, True)
        got[name] = op.backward(out, True)[1]
    for name, variant in (("step_wt", "aligned"), ("step_null", "wt_null")):
        op = Operands(k, variant)
        out = op.outputs()
        state = torch.zeros(op.P, dtype=torch.float32, device="cuda")
        assert op.step(op.step_args(out, "softmax", state=state, skip_update=1)) == 0
        out["arena"].check()
        g = out["grads"].cpu().numpy().astype(np.float64)
        got[name] = g[:op.P] / g[op.P + 1]
        assert op.inputs_untouched()  # (skip_update: the parameters stay)
    bar = 1e-5 * (np.abs(ref["grads"]) + ref["terms"]) + 1e-12
    for name, g in got.items():
        note("wt_null" if "null" in name else "aligned", "pair_%s/%s" % (name, CASE_IDS[k]), float((np.abs(g - ref["grads"]) / bar).max()), mfma_mode)
    names = sorted(got)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert (np.abs(got[a] - got[b]) <= bar).all(), (a, b, float((np.abs(got[a] - got[b]) / bar).max()))


@pytest.mark.parametrize("k", [1, 5], ids=[CASE_IDS[1], CASE_IDS[5]])
def test_eval_engine_with_misaligned_features_and_params(k):
    """EvalEngine.run (ultr_dnn_forward_ndcg): scores to the bar, and the NDCG of the aligned run."""
    from ultra_pytorch_amd import engine
    ref, ndcg = C.reference(k), {}
    for variant in ("aligned", "params+4_features+4"):
        op = Operands(k, variant)
        ev = engine.EvalEngine(op.shape, op.B, op.L, torch.device("cuda"))
        scores, nd = ev.run(op.params, op.feats.view(op.n_docs, op.F), op.n_docs, op.ids, op.labels)
        torch.cuda.synchronize()
        note(variant, "eval_engine/%s" % CASE_IDS[k], C.score_ratio(scores.cpu().numpy(), ref["scores"]))
        ndcg[variant] = nd.cpu().numpy()
        assert op.inputs_untouched()
    np.testing.assert_allclose(ndcg["params+4_features+4"], ndcg["aligned"], atol=1e-6)


def test_every_variant_was_reached():
    """(runs after the cases above: pytest keeps file order)  The largest error-to-bar ratio and the routes per operand variant."""
    missing = [v for v in C.VARIANTS if v not in RATIOS]
    for v in C.VARIANTS:
        if v in RATIOS:
            print("dnn_operands/%-22s largest error / bar %.3f at %s" % (v, RATIOS[v][0], RATIOS[v][1]))
            for r in sorted(ROUTES.get(v, ())):
                print("    " + r)
    assert not missing, missing
