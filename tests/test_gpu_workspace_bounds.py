"""The step kernels held to their declared workspace sizes (testing: the workspace contract).

Every scratch buffer of a training step is sized by the library itself (ultr_dnn_saved_bytes, ultr_dnn_bwd_workspace_bytes,
ultr_dnn_wt_floats, ultr_loss_workspace_bytes, ultr_step_tail_floats, ultr_setrank_saved_bytes, ultr_setrank_workspace_bytes,
ultr_nsgd_workspace_bytes, and two hand-written formulas in engine.py).  torch's caching allocator rounds every request up and packs
tensors into shared blocks, so neither a write past a declared size nor a read of a word the step never wrote shows in any comparison
with the oracle.  Here the buffers of an engine are re-seated on a guarded arena (tests/guarded.py: exact lengths, 512-byte aligned
starts, 1 MiB NaN-pattern bands in front and behind; buffers the engine allocates with torch.empty are poisoned with the same pattern,
buffers it zeroes are zeroed) and every case runs the same two steps on a plain and on a guarded engine:

  (a) the bands are intact after every step: no write outside any declared size;
  (b) scores, step scalars, gradients + step tail, updated parameters, optimizer state, aux and the weight copy are bit for bit those
      of the plain run (int32 compare, NaNs included): a consumed poison word would turn them into NaN or other bits;
  (c) the second step, over the first one's leftovers, matches the plain engine's second step as well.

No tolerance anywhere: the reference is the unguarded run of the same library, which the rest of the suite pins to the oracle at these
shapes (test_gpu_planner_sweep, test_gpu_knobs, test_gpu_losses, test_gpu_setrank, test_gpu_dbgd, test_gpu_nsgd)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import guarded as G  # noqa: E402
from tests import loss_ref  # noqa: E402
from tests.hipref import dev  # noqa: E402
from tests.test_gpu_knobs import KNOB_SETS  # noqa: E402
from tests.test_gpu_planner_sweep import CASES as SWEEP_CASES, families  # noqa: E402

# device tensors of an engine that guard_engine leaves where they are, and why
LEFT = {"_counter": "EvalEngine's 4-byte launch counter: zeroed once, reset by every launch, no size to declare",
        "_exam": "DbgdEngine keeps the caller's click-model table alive: an input",
        "_cprob": "DbgdEngine keeps the caller's click-probability table alive: an input"}

STEP_BUFFERS = [("saved", False), ("bwd_ws", False), ("scores", False), ("dscores", False), ("loss_ws", True), ("grads", True),
                ("scalars", True)]
EVAL_BUFFERS = [("scores", False), ("masked", False), ("order", False), ("ndcg", False), ("ndcg_ws", False)]
DBGD_BUFFERS = [("noise", True), ("scores", True), ("winners", True), ("loss_scores", True), ("ndcg", True), ("ndcg_ws", False),
                ("grads", True), ("bwd_ws", True), ("scalars", True)]

SLACK = {}  # buffer -> (largest untouched share of a poisoned buffer seen, case): reported, not asserted


# ------------------------------------------------------------------------------------------------------------------------------
# the helper
# ------------------------------------------------------------------------------------------------------------------------------
def _device_tensors(eng):
    for name, v in vars(eng).items():
        if isinstance(v, torch.Tensor) and v.is_cuda:
            yield name, v
        elif isinstance(v, (list, tuple)) and v and all(isinstance(t, torch.Tensor) and t.is_cuda for t in v):
            for k, t in enumerate(v):
                yield "%s[%d]" % (name, k), t


def _weight_copy(eng):
    from ultra_pytorch_amd import hip_ops
    return hip_ops.weight_copy(eng.shape) if isinstance(eng.shape, hip_ops.DnnShape) else None


def arena_for(eng):
    """An arena large enough for every buffer guard_engine re-seats."""
    sizes = [t.numel() * t.element_size() for _, t in _device_tensors(eng)]
    if hasattr(eng, "cand_stride"):
        sizes.append(4 * eng.R * eng.cand_stride)
    wc = _weight_copy(eng)
    if wc is not None:
        sizes.append(4 * wc.n)
    return G.Arena(torch.device("cuda"), G.bytes_for(sizes))


def _swap(eng, arena, name, zero):
    old = getattr(eng, name)
    assert old.is_contiguous(), name
    if old.dtype == torch.float64:
        new = arena.view64(old.numel(), zero=zero, name=name)
    else:
        assert old.element_size() == 4, (name, old.dtype)
        new = arena.view(old.numel(), zero=zero, name=name)  # the engine's own sizing is what is under test
        if old.dtype != torch.float32:
            new = new.view(old.dtype)
    setattr(eng, name, new.view(old.shape))


def guard_engine(eng, arena):
    """Re-seat the workspace attributes of a freshly built engine (before its first step) with arena views of the same length:
    poisoned where the engine allocates with torch.empty, zeroed where it allocates zeroed.  Asserts that no device tensor of the
    engine escapes: each is swapped, or named in LEFT."""
    from ultra_pytorch_amd import engine as E
    swapped = set()
    if isinstance(eng, E.DbgdEngine):
        plan = list(DBGD_BUFFERS)
    elif isinstance(eng, E.EvalEngine):
        assert not eng._all
        plan = list(EVAL_BUFFERS)
    else:
        assert isinstance(eng, E.StepEngine) and eng._args is None, "guard_engine runs before the first step"
        plan = list(STEP_BUFFERS)
        if isinstance(eng, E.SetRankStepEngine):
            plan.append(("sr_ws", False))
    if isinstance(eng, E.NsgdEngine):
        plan += [("memory", True), ("nsgd_ws", True)]  # (nsgd_ws is torch.zeros today: it stays zeroed)
    for name, zero in plan:
        _swap(eng, arena, name, zero)
        swapped.add(name)
    if isinstance(eng, E.SetRankStepEngine):
        eng.saved[eng._flag_off].zero_()  # as _alloc does: the range word of a report before the first forward
    wc = _weight_copy(eng)
    if wc is not None and wc.n > 0:
        assert wc.wt is None, "the weight copy of this shape is already in use"
        wc.wt, wc.key = arena.view(wc.n, zero=True, name="wt"), None  # WeightCopy.get allocates only when wt is None
    if isinstance(eng, E.DbgdEngine):
        R, P, stride = eng.R, eng.P, eng.cand_stride
        eng.cand = arena.view(R * stride, zero=True, name="cand").view(R, stride)[:, :P]
        eng.cand_wt = [arena.view(t.numel(), zero=True, name="cand_wt[%d]" % r) for r, t in enumerate(eng.cand_wt)]
        swapped |= {"cand"} | {"cand_wt[%d]" % r for r in range(R)}
        a = eng.args  # DbgdEngine fills its argument block when it is built: the pointers follow the buffers
        a.noise, a.cand_params = eng.noise.data_ptr(), eng.cand.data_ptr()
        a.scores, a.winners, a.loss_scores = eng.scores.data_ptr(), eng.winners.data_ptr(), eng.loss_scores.data_ptr()
        a.ndcg, a.grads, a.bwd_ws = eng.ndcg.data_ptr(), eng.grads.data_ptr(), eng.bwd_ws.data_ptr()
        if isinstance(eng, E.NsgdEngine):
            eng.nargs.memory, eng.nargs.ws = eng.memory.data_ptr(), eng.nsgd_ws.data_ptr()
    lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + 4 * arena.buf.numel()
    for name, t in _device_tensors(eng):
        if name in LEFT:
            continue
        assert name in swapped, "device tensor %r of %s is neither guarded nor named in LEFT" % (name, type(eng).__name__)
        assert lo <= t.data_ptr() < hi and t.data_ptr() % 512 == 0, name
    return eng


def reseat_host_report(eng):
    """The 16-float step report in the middle of a larger pinned buffer filled with the pattern."""
    pad = 1024
    big = torch.empty(16 + 2 * pad, dtype=torch.float32).pin_memory()
    big.view(torch.int32).fill_(G._PATTERN_I32)
    eng._hs = big[pad:pad + 16]
    eng._hs.zero_()
    eng._hs_f = eng._hs.numpy()
    eng._hs_u = eng._hs_f.view(np.uint32)
    eng.udesc.host_scalars = eng._hs.data_ptr()
    return big, pad


def hold_host_report(big, pad):
    w = big.numpy().view(np.int32)
    assert (w[:pad] == G._PATTERN_I32).all() and (w[pad + 16:] == G._PATTERN_I32).all(), "the step report wrote outside its 16 floats"
    assert (w[pad + 11:pad + 16] == 0).all(), ("words 11..15 of the step report changed", w[pad + 11:pad + 16])
    assert w[pad + 9] != 0, "no report arrived"


# ------------------------------------------------------------------------------------------------------------------------------
# comparing
# ------------------------------------------------------------------------------------------------------------------------------
def bits(t):
    if t is None:
        return None
    a = t.detach().contiguous().cpu().numpy()
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).reshape(-1).copy()


def hold_equal(plain, guarded, what):
    assert plain.keys() == guarded.keys()
    for k in plain:
        a, b = plain[k], guarded[k]
        if a is None and b is None:
            continue
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0]
            poison = int((b[bad] == G._PATTERN_I32).sum()) if b.dtype == np.int32 else 0
            nan = int(np.isnan(b.view(np.float32 if b.dtype == np.int32 else np.float64)[bad]).sum())
            raise AssertionError("%s: '%s' of the guarded run differs from the plain run in %d of %d words (first at %d, last at %d; "
                                 "%d of them NaN, %d the poison pattern itself): a word the step never wrote was consumed"
                                 % (what, k, bad.size, a.size, int(bad[0]), int(bad[-1]), nan, poison))


def note_slack(arena, eng, case):
    for name in ("saved", "bwd_ws", "sr_ws", "ndcg_ws", "masked", "order"):
        t = getattr(eng, name, None)
        if t is None or t.numel() == 0 or (name, False) not in (DBGD_BUFFERS if hasattr(eng, "cand") else EVAL_BUFFERS + STEP_BUFFERS + [("sr_ws", False)]):
            continue  # (only buffers that start poisoned)
        share = arena.untouched(t) / float(t.numel())
        key = "%s.%s" % (type(eng).__name__, name)
        if share > SLACK.get(key, (-1.0, ""))[0]:
            SLACK[key] = (share, case)


def test_the_arena_reports_a_breach_on_the_device():
    """tests/test_guarded_cpu.py on a device arena, in short: a torch write one word past a view and one word in front of one."""
    arena = G.Arena(torch.device("cuda"), G.bytes_for([4 * 1000, 4 * 33]))
    a, b = arena.view(1000, name="a"), arena.view(33, zero=True, name="b")
    assert a.data_ptr() % 512 == 0 and b.data_ptr() % 512 == 0 and torch.isnan(a).all() and (b == 0).all()
    a.fill_(1.0)
    arena.check()
    _, start, n, _, _ = arena._record(a)
    arena.buf[start + n] = 0
    with pytest.raises(G.GuardBreach) as e:
        arena.check()
    assert (e.value.name, e.value.side, e.value.first, e.value.count) == ("a", "behind", 1000, 1)
    arena.buf[start + n] = G._PATTERN_I32
    arena.check()
    arena.buf[arena._record(b)[1] - 1] = 0
    with pytest.raises(G.GuardBreach) as e:
        arena.check()
    assert (e.value.name, e.value.side, e.value.first) == ("b", "front", -1)


# ------------------------------------------------------------------------------------------------------------------------------
# DNN steps
# ------------------------------------------------------------------------------------------------------------------------------
def dnn_inputs(F, hidden, B, L, algo, seed, n_pad=None, act="elu"):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import synthetic
    rng = np.random.RandomState(seed)
    n_pad = (2 if L >= 4 else 0) if n_pad is None else n_pad
    feats, ids, y = synthetic.make_batch(rng, B, L, F, clicks=(algo != "lambdarank"), n_pad=n_pad)
    if algo == "pairdebias" and L > 1:  # position 0 must lose a pair somewhere (the EM ratio divides by t_minus_loss[0]: loss_ref.make_case)
        y[0, 0], y[1, 0] = 0.0, 1.0
    params = O.init_params(F, hidden, seed=seed % 1000)
    params = params + rng.uniform(-0.1, 0.1, size=params.shape).astype(np.float32)  # LayerNorm affine parameters away from (1, 0)
    d = dict(F=F, hidden=list(hidden), B=B, L=L, algo=algo, act=act, feats=feats, ids=ids, y=y, params=params,
             state=None if algo == "dla" else (0.01 * rng.uniform(size=params.shape)).astype(np.float32), aux=None, ipw=None)
    if algo in ("softmax", "prs"):
        d["ipw"] = np.linspace(1.0, 6.0, 12).astype(np.float32)
    elif algo == "dla":
        d["aux"] = (0.1 * rng.randn(L + 1)).astype(np.float32)
    elif algo in ("pairdebias", "lambdarank"):
        d["aux"] = rng.uniform(0.8, 1.2, size=2 * L).astype(np.float32)
    elif algo == "regem":
        d["aux"] = rng.uniform(0.1, 0.9, size=L).astype(np.float32)
    return d


def from_loss_case(case):
    return dict(F=loss_ref.TOY_F, hidden=list(loss_ref.TOY_HIDDEN), B=case["B"], L=case["L"], algo=case["algo"], act="elu",
                feats=case["feats"], ids=case["ids"], y=case["labels"], params=case["params"],
                state=None if case["algo"] == "dla" else case["state"], aux=case["aux"], ipw=case["ipw"])


def snapshot(eng, p, st, aux):
    wc = _weight_copy(eng)
    return dict(scores=bits(eng.scores), scalars=bits(eng.scalars), grads=bits(eng.grads), params=bits(p), state=bits(st), aux=bits(aux),
                wt=bits(wc.wt) if wc is not None and wc.wt is not None else None)


def run_dnn(d, guarded, mode="train_step", host_report=False, n_steps=2, **kw):
    """n_steps steps from d's inputs on a fresh engine; mode: "train_step" (ONE C call), "stages" (forward / loss / backward / update) or
    "stages_fused_softmax" (forward / ultr_dnn_backward_softmax / update).  Returns the per-step snapshots."""
    from ultra_pytorch_amd import engine, hip_ops
    shape = hip_ops.DnnShape(d["F"], d["hidden"], d["act"])
    B, L = d["B"], d["L"]
    eng = engine.StepEngine(shape, B, L, torch.device("cuda"), algo=d["algo"], **kw)
    arena = None
    if guarded:
        arena = arena_for(eng)
        guard_engine(eng, arena)
    big = reseat_host_report(eng) if host_report else None
    p = dev(d["params"].copy())
    st = None if d["state"] is None else dev(d["state"].copy())
    aux = None if d["aux"] is None else dev(d["aux"].copy())
    tab = None if d["ipw"] is None else dev(d["ipw"])
    f, ids, y = dev(d["feats"]), dev(d["ids"], torch.int32), dev(d["y"], torch.float32)
    n_docs = d["feats"].shape[0]
    outs = []
    for k in range(n_steps):
        if mode == "train_step":
            eng.train_step(p, st, f, n_docs, ids, y, aux=aux, ipw_table=tab)
        else:
            eng.forward(p, f, n_docs, ids, train=True)
            if mode == "stages":
                eng.loss(y, aux=aux, ipw_table=tab, docids=ids, n_docs=n_docs)
                eng.backward(p, f, n_docs, ids)
            else:
                hip_ops.dnn_backward_softmax(shape, p, f, n_docs, ids, B, L, eng.saved, eng.scores, y, eng.loss_ws, eng.bwd_ws, eng.grads,
                                             ipw_table=tab, dscores_out=eng.dscores)
            eng.update(p, st, aux)
        torch.cuda.synchronize()
        if arena is not None:
            arena.check()
            assert arena.untouched(eng.scores) == 0  # (the step did run on the arena's views)
        if big is not None:
            hold_host_report(*big)
        outs.append(snapshot(eng, p, st, aux))
    if arena is not None:
        note_slack(arena, eng, "F%d_%s_B%dxL%d_%s" % (d["F"], "x".join(map(str, d["hidden"])) or "linear", B, L, d["algo"]))
    eng.close()
    return outs


def hold_dnn(d, what, **kw):
    plain = run_dnn(d, False, **kw)
    guarded = run_dnn(d, True, **kw)
    for k, (a, b) in enumerate(zip(plain, guarded)):
        hold_equal(a, b, "%s, step %d" % (what, k + 1))


# ---- the planner sweep ---------------------------------------------------------------------------------------------------------
SEEN = {}


def sweep_id(c):
    return "%02d_F%d_%s_B%dxL%d_%s_%s" % (c["k"], c["F"], "x".join(map(str, c["hidden"])) or "linear", c["B"], c["L"], c["algo"],
                                          "train" if c["train"] else "eval")


def run_eval(d, guarded):
    """EvalEngine.run, then StepEngine.forward(train=False), on the same inputs."""
    from ultra_pytorch_amd import engine, hip_ops
    B, L = d["B"], d["L"]
    cuda = torch.device("cuda")
    # (a shape object each: the weight copy belongs to the shape, and each engine's arena guards its own)
    ev = engine.EvalEngine(hip_ops.DnnShape(d["F"], d["hidden"], d["act"]), B, L, cuda)
    st = engine.StepEngine(hip_ops.DnnShape(d["F"], d["hidden"], d["act"]), B, L, cuda, algo="softmax")
    arenas = []
    if guarded:
        arenas = [arena_for(ev), arena_for(st)]
        guard_engine(ev, arenas[0])
        guard_engine(st, arenas[1])
    p = dev(d["params"].copy())
    f, ids, y = dev(d["feats"]), dev(d["ids"], torch.int32), dev(d["y"], torch.float32)
    n_docs = d["feats"].shape[0]
    scores, ndcg = ev.run(p, f, n_docs, ids, y)
    host = ev.read_ndcg()
    torch.cuda.synchronize()
    for a in arenas:
        a.check()
    # (masked and order are written whole by the metric launch: outputs as well)
    out = dict(scores=bits(scores), ndcg=bits(ndcg), host=host.view(np.int32).copy(), masked=bits(ev.masked), order=bits(ev.order))
    st.forward(p, f, n_docs, ids, train=False)
    torch.cuda.synchronize()
    for a in arenas:
        a.check()
    out["forward_scores"] = bits(st.scores)
    if guarded:
        note_slack(arenas[0], ev, "eval")
    st.close()
    return out


@pytest.mark.parametrize("c", SWEEP_CASES, ids=sweep_id)
def test_planner_sweep_stays_inside_its_workspaces(c):
    """Every case of tests.test_gpu_planner_sweep.CASES: the three forward kernels, the four backward kernels, the two weight-gradient
    kernels and the fused launch at the planner's rule boundaries."""
    d = dnn_inputs(c["F"], c["hidden"], c["B"], c["L"], c["algo"], 1000 + c["k"], n_pad=c["n_pad"], act=c["act"])
    for fam in families(c):
        SEEN[fam] = SEEN.get(fam, 0) + 1
    if c["train"]:
        hold_dnn(d, sweep_id(c))
    else:
        hold_equal(run_eval(d, False), run_eval(d, True), sweep_id(c))


def test_the_sweep_reached_every_kernel_family():
    """(runs after the cases above: pytest keeps file order)  The same set as test_gpu_planner_sweep asserts."""
    need = ["fwd_tile16", "fwd_wide", "bwd_wide", "eval_fwd_tile16", "eval_fwd_wide"]
    missing = [f for f in need if SEEN.get(f, 0) == 0]
    assert not missing, (missing, SEEN)
    assert any(k.startswith("bwd_tile") for k in SEEN), SEEN
    print("kernel families reached:", dict(sorted(SEEN.items())))


# ---- the knob sets -------------------------------------------------------------------------------------------------------------
KNOB_SHAPES = [(136, [256, 256], 33, 10), (137, [513, 255], 261, 17), (24, [32, 16], 7, 6)]
KNOB_IDS = [k[0].replace(" ", ",") + "-" + k[1] for k in KNOB_SETS]
REFUSED = []


@pytest.fixture(params=KNOB_SETS, ids=KNOB_IDS)
def knobs(request, monkeypatch):
    """tests.test_gpu_knobs' reload pattern: set the environment, ultr_config_reload, build the engine."""
    from ultra_pytorch_amd import _lib
    for kv in request.param[0].split():
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)
    _lib.load().ultr_config_reload()
    yield request.param
    monkeypatch.undo()
    _lib.load().ultr_config_reload()


@pytest.mark.parametrize("algo", ["softmax", "config"])
@pytest.mark.parametrize("F,hidden,B,L", KNOB_SHAPES, ids=["F136_256x256_B33xL10", "F137_513x255_B261xL17", "F24_32x16_B7xL6"])
def test_knob_sets_stay_inside_their_workspaces(knobs, F, hidden, B, L, algo):
    """Every entry of tests.test_gpu_knobs.KNOB_SETS at three small shapes, under NA / IPW (the fused forward + loss + backward launch) and
    under the algorithm of the full-size config the knob set names: the declared sizes claim to cover the env-tunable geometry."""
    from ultra_pytorch_amd import _lib
    algo = ("dla" if knobs[1].endswith("dla") else "pairdebias") if algo == "config" else algo
    d = dnn_inputs(F, hidden, B, L, algo, 77 + B)
    what = "%s at F%d %r B%d L%d %s" % (knobs[0], F, hidden, B, L, algo)
    try:
        plain = run_dnn(d, False)
    except _lib.UltrHipError as e:
        if "unsupported shape" not in str(e):
            raise
        REFUSED.append(what)
        pytest.skip("the library refuses %s (ULTR_E_UNSUPPORTED) on the plain engine as well: %s" % (what, e))
    guarded = run_dnn(d, True)  # (a refusal here, where the plain engine ran, is a failure)
    for k, (a, b) in enumerate(zip(plain, guarded)):
        hold_equal(a, b, "%s, step %d" % (what, k + 1))


# ---- every algorithm -----------------------------------------------------------------------------------------------------------
ALGOS = ["softmax", "dla", "pairdebias", "lambdarank", "regem", "prs", "pdgd"]
GEOM_L, GEOM_B = [1, 10, 33, 100, 256], [1, 37, 261]
VARIANTS = [dict(optimizer="ada"), dict(optimizer="sgd"), dict(optimizer="ada", l2_loss=0.01)]


@pytest.mark.parametrize("B", GEOM_B)
@pytest.mark.parametrize("L", GEOM_L)
@pytest.mark.parametrize("algo", ALGOS)
def test_every_algorithm_stays_inside_its_workspaces(algo, L, B):
    """The loss workspace, the step tail and the partial counts depend on (algo, B, L) only: F 24, hidden [32, 16].  The optimizer and
    l2_loss > 0 (l2_sums_kernel writes scalars[8:]) rotate over the geometries, so every algorithm meets Adagrad, SGD and the L2 term
    five times each (LambdaRank and PRSrank: Adagrad and SGD)."""
    # (LambdaRank and PRSrank have no l2_loss hyper-parameter: ultr_apply_update refuses it for them - they alternate the optimizers)
    kw = VARIANTS[(GEOM_L.index(L) + GEOM_B.index(B)) % (2 if algo in ("lambdarank", "prs") else 3)]
    d = dnn_inputs(24, [32, 16], B, L, algo, 31 * L + B)
    hold_dnn(d, "%s B%d L%d %r" % (algo, B, L, kw), **kw)


@pytest.mark.parametrize("algo,B", loss_ref.MANY)
def test_many_lists_stay_inside_their_workspaces(algo, B):
    """More than 1024 lists: the two-level fold of the step tail (tests.loss_ref.MANY at MANY_L)."""
    hold_dnn(from_loss_case(loss_ref.many_case(algo, B)), "many-%s-B%d" % (algo, B))


# ---- the stage calls -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["stages", "stages_fused_softmax"])
@pytest.mark.parametrize("F,hidden,B,L", [(136, [256, 256], 33, 10), (20, [32], 9, 13)], ids=["F136_256x256_B33xL10", "F20_32_B9xL13"])
def test_stage_calls_stay_inside_their_workspaces(F, hidden, B, L, mode):
    """forward(train=True) / loss / backward / update, and ultr_dnn_backward_softmax in place of loss + backward: the path of the
    plug-ins and of the process-group mode."""
    hold_dnn(dnn_inputs(F, hidden, B, L, "softmax", 5 + B), "%s F%d B%d L%d" % (mode, F, B, L), mode=mode)


def test_dnn_step_report_stays_inside_its_16_floats():
    """The host-mapped step report re-seated into the middle of a pinned buffer full of the pattern: only words 0 .. 10 may change."""
    hold_dnn(dnn_inputs(136, [256, 256], 33, 10, "softmax", 9), "host report", host_report=True)


# ------------------------------------------------------------------------------------------------------------------------------
# SetRank
# ------------------------------------------------------------------------------------------------------------------------------
def _setrank_shapes():
    from tests import test_gpu_setrank as T
    oracle_shapes = [m for m in T.test_setrank_oracle.pytestmark if m.name == "parametrize"][0].args[1]
    assert len(oracle_shapes) == 7
    return list(oracle_shapes) + [T.FUSED_SHAPES[0], T.BWD_FUSED_SHAPES[0], T.BWD_FUSED_SHAPES[2]]


SR_SHAPES = _setrank_shapes()
SR_RAGGED, SR_PADDED = (3, 37, 20, 48, 6, 1, 20), SR_SHAPES[7]  # a ragged last token block; (37, 30, ...) with PAD documents
SR_SETTINGS = ([("ULTR_SR_BLOCK", v) for v in "023"] + [("ULTR_SR_BWD_FUSED", v) for v in ("0", "6", "7")]
               + [("ULTR_SR_ATTN_H3", v) for v in "01"] + [("attention_dtype", "fp16")])


def run_setrank(B, L, F, dm, H, nl, dff, guarded, dtype="fp32", host_report=False, n_steps=2):
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    shape = hip_ops.SetRankShape(F, dm, H, nl, dff, attention_dtype=dtype)
    rng = np.random.RandomState(11)
    feats, ids, y = synthetic.make_batch(rng, B, L, F, n_pad=3 if L > 8 else 0)
    ipw = np.asarray(synthetic.load_ipw(), np.float32)
    p0 = init_setrank_params(shape, seed=9).numpy()
    p0 = p0 + rng.normal(scale=0.02, size=p0.shape).astype(np.float32)
    eng = engine.SetRankStepEngine(shape, B, L, torch.device("cuda"), algo="softmax", learning_rate=0.05, max_gradient_norm=5.0)
    arena = None
    if guarded:
        arena = arena_for(eng)
        guard_engine(eng, arena)
    big = reseat_host_report(eng) if host_report else None
    p, st = dev(p0.copy()), dev(np.zeros_like(p0))
    f, i, yy, tab = dev(feats), dev(ids, torch.int32), dev(y, torch.float32), dev(ipw)
    outs = []
    for k in range(n_steps):
        eng.train_step(p, st, f, feats.shape[0], i, yy, ipw_table=tab)
        torch.cuda.synchronize()
        if arena is not None:
            arena.check()
            assert arena.untouched(eng.scores) == 0  # (the step did run on the arena's views)
        if big is not None:
            hold_host_report(*big)
        outs.append(snapshot(eng, p, st, None))
    if arena is not None:
        note_slack(arena, eng, "B%d_L%d_F%d_d%d_H%d_nl%d_dff%d" % (B, L, F, dm, H, nl, dff))
    eng.close()
    return outs


def hold_setrank(shape, what, **kw):
    plain = run_setrank(*shape, False, **kw)
    guarded = run_setrank(*shape, True, **kw)
    for k, (a, b) in enumerate(zip(plain, guarded)):
        hold_equal(a, b, "%s, step %d" % (what, k + 1))


@pytest.mark.parametrize("shape", SR_SHAPES, ids=lambda s: "B%d_L%d_F%d_d%d_H%d_nl%d_dff%d" % tuple(s))
def test_setrank_stays_inside_its_workspaces(shape):
    """The seven shapes of test_setrank_oracle, FUSED_SHAPES[0], BWD_FUSED_SHAPES[0] and [2] under the default knobs: `saved` and
    `sr_ws` against ultr_setrank_saved_bytes / ultr_setrank_workspace_bytes, `bwd_ws` against engine.py's own formula."""
    hold_setrank(tuple(shape), "SetRank %r" % (tuple(shape),))


@pytest.mark.parametrize("shape", [SR_RAGGED, SR_PADDED], ids=["ragged_B3_L37", "padded_B37_L30"])
@pytest.mark.parametrize("setting", SR_SETTINGS, ids=["%s=%s" % s for s in SR_SETTINGS])
def test_setrank_knobs_stay_inside_their_workspaces(setting, shape, monkeypatch):
    from ultra_pytorch_amd import _lib
    kw = {}
    try:
        if setting[0] == "attention_dtype":
            kw["dtype"] = setting[1]
        else:
            monkeypatch.setenv(*setting)
            _lib.load().ultr_config_reload()
        hold_setrank(tuple(shape), "SetRank %s=%s %r" % (setting[0], setting[1], tuple(shape)), **kw)
    finally:
        monkeypatch.undo()
        _lib.load().ultr_config_reload()


def test_setrank_step_report_stays_inside_its_16_floats():
    hold_setrank(SR_PADDED, "SetRank host report", host_report=True)


# ------------------------------------------------------------------------------------------------------------------------------
# DBGD / MGD / NSGD
# ------------------------------------------------------------------------------------------------------------------------------
def run_online(kind, R, need_interleave, guarded, n_steps=2):
    """The smallest step shape of tests/test_gpu_dbgd.py and tests/test_gpu_nsgd.py: F 24, hidden [32, 16], 16 lists of 12 candidates,
    rank list 8 (P = 1489: cand_stride = 1536 != P)."""
    from ultra_pytorch_amd import engine, hip_ops
    from ultra_pytorch_amd.ranking_model.dnn import init_flat_params
    from tests.test_gpu_dbgd import _batch, _click_model, _cuda
    from tests.test_gpu_nsgd import _memory
    F, hidden, B, M, rls = 24, [32, 16], 16, 12, 8
    shape = hip_ops.DnnShape(F, hidden, "elu")
    model, ex, n_exam, cprob = _click_model("pbm")
    cls = engine.NsgdEngine if kind == "nsgd" else engine.DbgdEngine
    eng = cls(shape, B, M, rls, R, torch.device("cuda"), click_model=model, exam=ex, n_exam=n_exam, cprob=_cuda(cprob),
              need_interleave=need_interleave, stochastic=True, optimizer="ada", learning_rate=0.1, noise_rate=0.1, seed=77)
    assert eng.cand_stride != eng.P
    arena = None
    if guarded:
        arena = arena_for(eng)
        guard_engine(eng, arena)
    rng = np.random.RandomState(5)
    if kind == "nsgd":
        eng.memory.copy_(_cuda(_memory(rng, F, hidden, R, shape.n_params)))
    feats, ids, y, n_docs = _batch(rng, F, B, M)
    f, i_, yy = _cuda(feats), _cuda(ids), _cuda(y)
    p = init_flat_params(shape, seed=3).cuda()
    st = torch.full_like(p, 0.1)
    outs = []
    for k in range(n_steps):
        eng.train_step(p, st, f, n_docs, i_, yy, step=3 + k)
        eng.read_loss()
        torch.cuda.synchronize()
        if arena is not None:
            arena.check()
        wc = _weight_copy(eng)
        out = dict(params=bits(p), state=bits(st), wt=bits(wc.wt), cand=bits(torch.as_strided(eng.cand, (R, eng.cand_stride), (eng.cand_stride, 1))),
                   host=eng._hs_f.view(np.int32).copy())
        for name in ("noise", "scores", "winners", "loss_scores", "ndcg", "grads", "scalars", "memory", "nsgd_ws"):
            out[name] = bits(getattr(eng, name, None))
        for r, t in enumerate(eng.cand_wt):
            out["cand_wt[%d]" % r] = bits(t)
        outs.append(out)
    if arena is not None:
        note_slack(arena, eng, "%s_R%d" % (kind, R))
    return outs


@pytest.mark.parametrize("kind,R,need_interleave", [("dbgd", 1, True), ("mgd", 4, True), ("mgd", 4, False), ("nsgd", 1, False),
                                                    ("nsgd", 4, True)])
def test_online_learners_stay_inside_their_workspaces(kind, R, need_interleave):
    """One DBGD, MGD and NSGD step (and a second one over its leftovers) with one and with four candidate rankers: every buffer of
    DbgdEngine / NsgdEngine.__init__, `cand` on its 64-float stride, each cand_wt[r], nsgd_ws through the 64-bit view."""
    plain = run_online(kind, R, need_interleave, False)
    guarded = run_online(kind, R, need_interleave, True)
    for k, (a, b) in enumerate(zip(plain, guarded)):
        hold_equal(a, b, "%s R=%d interleave=%s, step %d" % (kind, R, need_interleave, k + 1))


def test_report_of_the_run():
    """(last in file order)  What was reached, what was refused, and how loose the declared sizes are: printed, not asserted."""
    print("kernel families reached:", dict(sorted(SEEN.items())))
    print("knob sets refused by the library (skipped):", REFUSED or "none")
    for key, (share, case) in sorted(SLACK.items()):
        print("largest never-written share of %s: %.1f %% (%s)" % (key, 100.0 * share, case))
