"""The heads of the step's tail kernels (weight gradients, slab reduction, update) look their work up in a copy of the plans that
the workgroup stages into LDS with one load per thread (csrc/ultr_dnn_wgrad.hip: wg_stage / wg_head, red_stage / red_lookup;
csrc/ultr_update.hip: upd_at) instead of walking the by-value plan arguments entry by entry.  One training step through
ultr_train_step (engine.StepEngine, the plugin for the device feed) against the oracle at the shapes where such a look-up can
go wrong, at the tolerances of tests/test_gpu_parity.py, plus bitwise equality of two runs from the same state.  The shapes whose
segment starts fall on / next to a 256-element block boundary assert that they do (BOUNDARY_CASES).

Tolerances (test_gpu_parity.py): scores 1e-5; loss and gradient norm 1e-5 relative; gradients 1e-5 relative + 1e-6 * max|g|
(nets with a LayerNorm over <= 6 units: the `_odd` band of test_gpu_parity.gtol, 2e-5 / 1e-5 * max|g| - fp32 evaluation-order noise
in their inputs is amplified by rstd for torch-CPU and the HIP path alike); parameters 1e-5 relative + 5e-6 where |g| is not ~0;
Adagrad state 2e-5 relative (`_odd`: 4e-5) + 2e-6 * max; EM state 1e-6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.hipref import dev  # noqa: E402
from tests.test_gpu_parity import gtol  # noqa: E402

LR = 0.05


def _odd(F, hidden):
    return min([F] + list(hidden)) <= 6  # a LayerNorm over 3-6 units (every Linear's input is normalised)


def _inputs(F, hidden, B, L, seed, n_pad=0):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import synthetic
    rng = np.random.RandomState(seed)
    feats, ids, y = synthetic.make_batch(rng, B, L, F, n_pad=n_pad)
    p0 = O.init_params(F, hidden, seed=seed + 1)
    for name, shape, off in O.param_layout(F, hidden):  # non-trivial LayerNorm affine parameters
        if "layer_norm" in name:
            n = int(np.prod(shape))
            p0[off:off + n] += rng.uniform(-0.3, 0.3, size=n).astype(np.float32)
    # a warm Adagrad accumulator: from zero the first update is lr * sign(g), which flips on rounding noise where g ~ 0
    s0 = rng.uniform(0.05, 0.2, size=p0.shape).astype(np.float32)
    return feats, ids, y, p0, s0


def _aux0(algo, L, rng):
    if algo == "dla":
        return rng.normal(scale=0.3, size=L + 1).astype(np.float32)
    if algo == "pairdebias":
        return rng.uniform(0.8, 1.2, size=2 * L).astype(np.float32)
    return None


def _oracle(algo, F, hidden, feats, ids, y, p0, s0, aux0, ipw):
    from oracle import ultr_oracle as O
    L = ids.shape[0]
    if algo == "softmax":
        return O.train_step_softmax(p0, s0, F, hidden, feats, ids, y, ipw_list=ipw, lr=LR, max_norm=5.0)
    if algo == "dla":
        return O.dla_step(p0, aux0, F, hidden, feats, ids, y, lr=LR, max_norm=5.0)
    r = O.pairdebias_step(p0, s0, aux0[:L], aux0[L:], F, hidden, feats, ids, y, lr=LR, max_norm=5.0)
    return r


def _gpu_step(eng, algo, feats, ids, y, p0, s0, aux0, ipw):
    params = dev(p0.copy())
    state = None if algo == "dla" else dev(s0.copy())
    aux = None if aux0 is None else dev(aux0.copy())
    sc = eng.train_step(params, state, dev(feats), feats.shape[0], dev(ids, torch.int32), dev(y), aux=aux,
                        ipw_table=dev(ipw) if algo == "softmax" else None)
    torch.cuda.synchronize()
    return dict(scores=eng.scores.cpu().numpy().copy(), grads=eng.grads.cpu().numpy().copy(), params=params.cpu().numpy().copy(),
                state=None if state is None else state.cpu().numpy().copy(), aux=None if aux is None else aux.cpu().numpy().copy(),
                scalars=sc.cpu().numpy().copy())


def _check(algo, F, hidden, out, ref, L):
    name = "x_odd" if _odd(F, hidden) else "x"
    P = ref["grads"].shape[0]
    sc = out["scalars"]
    np.testing.assert_allclose(out["scores"], ref["scores"], atol=1e-5, rtol=0, err_msg="scores")
    assert abs(float(sc[0]) - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"])), ("loss", sc[0], ref["loss"])
    assert abs(float(sc[1]) - ref["norm"]) <= 1e-5 * max(1.0, ref["norm"]), ("norm", sc[1], ref["norm"])
    gs = 1.0 if algo == "pairdebias" else 1.0 / float(sc[3])  # the gradient is kept unnormalised; the update applies 1 / D
    gref = ref["grads"]
    np.testing.assert_allclose(out["grads"][:P] * gs, gref, err_msg="grads", **gtol(gref, name))
    sel = np.abs(gref) > 1e-6 * max(1.0, float(np.abs(gref).max()))
    np.testing.assert_allclose(out["params"][sel], ref["params"][sel], atol=5e-6, rtol=1e-5, err_msg="params")
    if algo != "dla":
        np.testing.assert_allclose(out["state"], ref["state"], rtol=4e-5 if name == "x_odd" else 2e-5, atol=2e-6 * float(ref["state"].max()),
                                   err_msg="optimizer state")
    if algo == "dla":
        np.testing.assert_allclose(out["aux"], ref["prop_params"], atol=1e-6)
        assert abs(float(sc[6]) - ref["prop_norm"]) < 1e-6
        assert abs(float(sc[4]) - ref["rank_loss"]) < 1e-5 and abs(float(sc[5]) - ref["exam_loss"]) < 1e-5
    if algo == "pairdebias":
        np.testing.assert_allclose(out["aux"][:L], ref["t_plus"].ravel(), atol=1e-6)
        np.testing.assert_allclose(out["aux"][L:], ref["t_minus"].ravel(), atol=1e-6)


def _bits_equal(a, b):
    for k in a:
        if a[k] is None:
            assert b[k] is None
            continue
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "%s differs between two runs from the same state" % k


CASES = [
    # algo, F, hidden, B, L, n_pad
    # the most Linear layers ULTR_MAXL allows (7 hidden + scorer), tiny uneven widths: 32 reduction segments, most of them
    # shorter than a reduce block - a block spans five or more segments, the last block is partial; 7 layers in the wgrad head
    ("softmax", 5, [8, 12, 4, 20, 8, 4, 12], 3, 4, 0),
    # one hidden layer at odd sizes (the block-boundary shapes proper are BOUNDARY_CASES below)
    ("softmax", 16, [16], 8, 4, 0),
    ("softmax", 17, [16], 8, 4, 0),
    # a second k-tile with 8 live columns, several row splits; F = 70: not a multiple of 4 (the non-vector wgrad kernel)
    ("softmax", 72, [64, 68], 20, 10, 1),
    ("softmax", 70, [64, 68], 20, 10, 0),
    # the tail variants: dla = stateless update, separate kernels, doc-id resolution in the wgrad head; pairdebias = aux state
    # in update block 0 (softmax above: fused kernel, pre-normalised operands, layer-0 shortcut)
    ("dla", 72, [64, 68], 20, 10, 1),
    ("dla", 5, [8, 12, 4, 20, 8, 4, 12], 3, 4, 0),
    ("pairdebias", 70, [64, 68], 20, 10, 0),
    ("pairdebias", 17, [16], 8, 4, 0),
]


@pytest.mark.parametrize("algo,F,hidden,B,L,n_pad", CASES)
def test_step_against_the_oracle_and_twice_bitwise(algo, F, hidden, B, L, n_pad):
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    feats, ids, y, p0, s0 = _inputs(F, hidden, B, L, seed=11, n_pad=n_pad)
    aux0 = _aux0(algo, L, np.random.RandomState(3))
    ipw = np.asarray(synthetic.load_ipw(), np.float32)
    ref = _oracle(algo, F, hidden, feats, ids, y, p0, s0, aux0, ipw)
    shape = hip_ops.DnnShape(F, hidden, "elu")
    eng = engine.StepEngine(shape, B, L, torch.device("cuda"), algo=algo, learning_rate=LR, max_gradient_norm=5.0)
    out = _gpu_step(eng, algo, feats, ids, y, p0, s0, aux0, ipw)
    _check(algo, F, hidden, out, ref, L)
    _bits_equal(out, _gpu_step(eng, algo, feats, ids, y, p0, s0, aux0, ipw))


def _seg_starts(F, hidden):
    """Where the slab reduction's segments start: one per parameter tensor, in layout order (ln.w, ln.b, W, b per layer)."""
    from oracle import ultr_oracle as O
    return [off for _, _, off in O.param_layout(F, hidden)]


def _vs_begin(F, hidden):
    """DnnPlan::vs_begin: the update's vector-parameter map - per layer gamma | beta (2 K_j), then the bias (M_j), the scorer's
    weight row and bias last - as prefix sums; the last entry is the number of vector parameters."""
    K, M = [F] + list(hidden), list(hidden) + [1]
    v = [0]
    for j in range(len(K)):
        v.append(v[-1] + 2 * K[j])
        if j < len(K) - 1:
            v.append(v[-1] + M[j])
        else:
            v.append(v[-1] + K[j])
            v.append(v[-1] + 1)
    return v


# The small models take one thread per element, 256 elements per workgroup, in the reduction (grad_reduce_kernel<true>) and in
# the vector workgroups of the update; block 0 is elements 0 .. 255, block 1 starts at 256.  `where` names the table that gets an
# entry equal to `at` ("seg": the reduction's segment starts, "vs": DnnPlan::vs_begin).  The compares of the look-up then meet
#   at = 256: the first element of block 1 IS a segment's first (e0 == start), the last of block 0 is the one before (e1 == start - 1);
#   at = 257: block 1 begins one element before a segment start (e0 == start - 1);
#   at = 255: the last element of block 0 is a segment's first (e1 == start).
BOUNDARY_CASES = [
    # F, hidden, where, at
    (16, [14], "seg", 256),   # 2 * 16 + 14 * 16 = 256: W_0 ends with block 0, b_0 starts block 1
    (6, [35], "seg", 257),    # 2 * 6 + 35 * 6 + 35 = 257: b_0 ends one element into block 1, ln_1.w starts at 257
    (15, [15], "seg", 255),   # 2 * 15 + 15 * 15 = 255: b_0 starts on the last element of block 0
    (128, [8], "vs", 256),    # 2 * 128 = 256: gamma_0 | beta_0 fill the first vector workgroup, b_0 starts the second
    (124, [9], "vs", 257),    # 2 * 124 + 9 = 257: b_0 ends one element into the second vector workgroup
    (124, [7], "vs", 255),    # 2 * 124 + 7 = 255: the segment behind b_0 starts on the last element of the first
]


@pytest.mark.parametrize("F,hidden,where,at", BOUNDARY_CASES)
def test_segment_start_at_a_block_boundary(F, hidden, where, at):
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    table = _seg_starts(F, hidden) if where == "seg" else _vs_begin(F, hidden)
    assert at in table[1:-1] and table[-1] > 256, (at, table)  # the shape does what its comment says, and a second block exists
    B, L = 8, 4
    feats, ids, y, p0, s0 = _inputs(F, hidden, B, L, seed=17)
    ipw = np.asarray(synthetic.load_ipw(), np.float32)
    ref = _oracle("softmax", F, hidden, feats, ids, y, p0, s0, None, ipw)
    eng = engine.StepEngine(hip_ops.DnnShape(F, hidden, "elu"), B, L, torch.device("cuda"), algo="softmax", learning_rate=LR, max_gradient_norm=5.0)
    out = _gpu_step(eng, "softmax", feats, ids, y, p0, s0, None, ipw)
    _check("softmax", F, hidden, out, ref, L)
    _bits_equal(out, _gpu_step(eng, "softmax", feats, ids, y, p0, s0, None, ipw))


DEEP = [8, 12, 4, 20, 8, 4, 12]  # 7 hidden layers + scorer: 32 reduction segments, most of them shorter than a block


def _deep_step(F, B, L, env, monkeypatch, comm=False):
    """One softmax step of the 8-layer model under the knobs `env`, against the oracle; returns the outputs."""
    import ctypes
    from ultra_pytorch_amd import _lib, engine, hip_ops, parallel, synthetic
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    shape = hip_ops.DnnShape(F, DEEP, "elu")
    pc = None
    try:
        if comm:  # a one-rank communicator: the slab reduction takes grad_reduce_xchg_kernel<1>
            h = ctypes.c_void_p()
            n = shape.n_params + hip_ops.tail_floats(L)
            _lib.check(shape.lib.ultr_comm_create(0, 1, n, ctypes.byref(h)), "ultr_comm_create")
            pc = parallel.PeerComm(shape.lib, h, 0, 1, n)
        eng = engine.StepEngine(shape, B, L, torch.device("cuda"), algo="softmax", learning_rate=LR, max_gradient_norm=5.0, comm=pc)
        feats, ids, y, p0, s0 = _inputs(F, DEEP, B, L, seed=23)
        ipw = np.asarray(synthetic.load_ipw(), np.float32)
        ref = _oracle("softmax", F, DEEP, feats, ids, y, p0, s0, None, ipw)
        out = _gpu_step(eng, "softmax", feats, ids, y, p0, s0, None, ipw)
        _check("softmax", F, DEEP, out, ref, L)
        _bits_equal(out, _gpu_step(eng, "softmax", feats, ids, y, p0, s0, None, ipw))
        if pc is not None:
            assert pc.status() == 0
        return out
    finally:
        if pc is not None:
            pc.close()
        monkeypatch.undo()
        shape.lib.ultr_config_reload()


def test_deep_model_on_the_split_half_weight_gradients(monkeypatch):
    """wg_head inside dnn_wgrad_h3_kernel with seven layers (ULTR_WG_H3=2 forces the kernel onto a small batch): every width a
    multiple of 4 as that kernel requires, B * L = 160 rows = three row splits."""
    _deep_step(8, 40, 4, {"ULTR_WG_H3": "2"}, monkeypatch)


def test_deep_model_on_the_cooperating_reduction(monkeypatch):
    """red_lookup in grad_reduce_kernel<false> (64 elements per workgroup, four cooperating groups: taken when a short segment has
    more than 128 parts) at the many-short-segments shape: 9 000 rows in 64-row splits = 141 slabs per segment."""
    _deep_step(5, 900, 10, {"ULTR_WGRAD_WGS": "1000"}, monkeypatch)


def test_deep_model_through_the_exchanging_reduction(monkeypatch):
    """red_lookup in grad_reduce_xchg_kernel<1>: the step with a one-rank communicator gives the bits of the plain step."""
    plain = _deep_step(5, 3, 4, {}, monkeypatch)
    xchg = _deep_step(5, 3, 4, {}, monkeypatch, comm=True)
    for k in ("scores", "params", "state"):
        assert np.array_equal(plain[k].view(np.uint32), xchg[k].view(np.uint32)), k
    P = plain["params"].shape[0]
    assert np.array_equal(plain["grads"][:P].view(np.uint32), xchg["grads"][:P].view(np.uint32))


def test_plans_follow_the_batch_shape():
    """Two engines of different (B, L) on ONE model, used alternately (what a plugin does when the batch size changes between
    calls: one cached engine per (B, L)): every step is the oracle's for ITS shape - nothing of the other plan survives."""
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    F, hidden = 33, [17, 9]
    shape = hip_ops.DnnShape(F, hidden, "elu")
    ipw = np.asarray(synthetic.load_ipw(), np.float32)
    shapes = [(8, 4), (3, 6), (37, 5)]
    engs = [engine.StepEngine(shape, B, L, torch.device("cuda"), algo="softmax", learning_rate=LR, max_gradient_norm=5.0) for B, L in shapes]
    _, _, _, p, s = _inputs(F, hidden, 8, 4, seed=5)
    first = {}
    for it in range(6):
        k = it % 3
        B, L = shapes[k]
        feats, ids, y, _, _ = _inputs(F, hidden, B, L, seed=20 + k)
        ref = _oracle("softmax", F, hidden, feats, ids, y, p, s, None, ipw)
        out = _gpu_step(engs[k], "softmax", feats, ids, y, p, s, None, ipw)
        _check("softmax", F, hidden, out, ref, L)
        if it < 3:
            first[k] = (p.copy(), s.copy(), out)
        p, s = out["params"], out["state"]
    for k in range(3):  # ... and a step repeated after the other shapes ran gives the same bits
        B, L = shapes[k]
        feats, ids, y, _, _ = _inputs(F, hidden, B, L, seed=20 + k)
        _bits_equal(first[k][2], _gpu_step(engs[k], "softmax", feats, ids, y, first[k][0], first[k][1], None, ipw))


def _feed_run(steps=2):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd.input_layer import DeviceClickFeed
    from ultra_pytorch_amd.utils import find_class
    from tests.test_gpu_plugins import load_flat
    from tests.test_gpu_prs import DS, _feed_arrays
    F, L, B, hidden = 24, 10, 6, [16, 8]
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.IPWrank", "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=[16,8]",
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3]}
    ds = DS(64, L, F, seed=4)
    algo = find_class(exp["learning_algorithm"])(ds, exp)
    load_flat(algo.model, O.init_params(F, hidden, seed=6))
    algo.state_sum.fill_(0.1)
    feed = DeviceClickFeed(algo, B, "", seed=3)
    for _ in range(steps):
        input_feed, _ = feed.get_batch(ds, check_validation=True)
        feats, ids, y = _feed_arrays(algo, input_feed, L)
        p0, s0 = algo.model.flat_params.cpu().numpy().copy(), algo.state_sum.cpu().numpy().copy()
        loss, _, _ = algo.train(input_feed)  # ultr_feed_train_step: the next batch's draw rides behind the update's workgroups
        torch.cuda.synchronize()
        ref = O.train_step_softmax(p0, s0, F, hidden, feats, ids.astype(np.int32), y, ipw_list=algo.IPW_list, lr=LR, max_norm=5.0)
        assert abs(loss - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"]))
        g = ref["grads"]
        sel = np.abs(g) > 1e-6 * max(1.0, float(np.abs(g).max()))
        np.testing.assert_allclose(algo.model.flat_params.cpu().numpy()[sel], ref["params"][sel], atol=5e-6, rtol=1e-5, err_msg="params")
        np.testing.assert_allclose(algo.state_sum.cpu().numpy(), ref["state"], rtol=2e-5, atol=2e-6 * float(ref["state"].max()))
    return algo.model.flat_params.cpu().numpy().copy(), algo.state_sum.cpu().numpy().copy()


def test_device_feed_step_with_rider_workgroups():
    """The device-feed step at a small batch (B = 6: two rider workgroups behind the update's own) against the oracle, twice."""
    a, b = _feed_run(), _feed_run()
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
