"""NSGD on the GPU (csrc/ultr_nsgd.hip): the null-space noise through the C ABI against the host restatement (tests/nsgd_ref.py) and
its invariants, the memory kernel's two loser rules, the reference's recorded steps (tests/golden/nsgd_*.npz) with the recorded unit
noise injected, an interleaved step, determinism, online training through the device feed, and the refusals."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import dbgd_ref as D
from tests import nsgd_ref as S
from tests.test_gpu_dbgd import LearnableDS, _batch, _click_model, _cuda, _ptr, _valid_ndcg, make_algo

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED, STEP = 0x0123456789ABCDEF, 2 ** 32 + 5


def _memory(rng, F, hidden, R, P):
    """Random memory rows with an empty slot (R > 2) and, in the first weight, a row that is the sum of two others."""
    mem = np.zeros((R, P), np.float32)
    for off, n, _ in S.tensors(F, hidden):
        mem[:, off:off + n] = rng.standard_normal((R, n)) / np.sqrt(n)
    if R > 2:
        mem[1] = 0.0
    if R > 3:
        off, n, _ = S.tensors(F, hidden)[0]
        mem[3, off:off + n] = mem[0, off:off + n] + mem[2, off:off + n]
    return mem


def run_noise(F, hidden, R, mem, theta, rate, normals=None, unit=None, seed=SEED, step=STEP):
    from ultra_pytorch_amd import _lib, hip_ops
    shape = hip_ops.DnnShape(F, hidden, "elu")
    P = shape.n_params
    lib = _lib.load()
    th, m = _cuda(theta), _cuda(mem)
    u = torch.full((R, P), -7.0, device="cuda")
    cand = torch.full((R, P), -7.0, device="cuda")
    nb = lib.ultr_nsgd_workspace_bytes(ctypes.byref(shape.desc), R)
    assert nb > 0
    ws = torch.full(((nb + 7) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    zt = _cuda(np.asarray(normals, np.float32)) if normals is not None else None
    ut = _cuda(np.asarray(unit, np.float32)) if unit is not None else None
    a = _lib.DbgdArgs(desc=ctypes.pointer(shape.desc), n_params=P, n_rankers=R, batch=1, max_candidates=1, rank_list_size=1,
                      noise_rate=rate, seed=seed, step=step, params=_ptr(th), noise=_ptr(u), cand_params=_ptr(cand))
    n = _lib.NsgdArgs(dbgd=ctypes.pointer(a), memory=_ptr(m), normals_in=_ptr(zt), unit_noise_in=_ptr(ut), ws=_ptr(ws))
    _lib.check(lib.ultr_nsgd_noise_args(ctypes.byref(n), hip_ops.raw_stream()), "ultr_nsgd_noise_args")
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), mem)  # the noise launch only reads the memory
    return u.cpu().numpy(), cand.cpu().numpy()


def check_invariants(u, mem, F, hidden):
    lay, _ = D.layout(F, hidden)
    for og, k, *_ in lay:
        assert (u[:, og:og + 2 * k] == 0).all()  # LayerNorm: no noise
    for off, n, scalar in S.tensors(F, hidden):
        ut, mt = u[:, off:off + n].astype(np.float64), mem[:, off:off + n].astype(np.float64)
        if scalar:
            assert set(np.unique(ut)) <= {-1.0, 1.0}
            continue
        nrm = np.sqrt((ut ** 2).sum(1))
        if len(S.kept_rows(mt)) >= n:
            assert (ut == 0).all()
            continue
        np.testing.assert_allclose(nrm, 1.0, atol=1e-6)
        assert np.abs(ut @ mt[mt.any(1)].T).max(initial=0.0) <= 1e-5


@pytest.mark.parametrize("F,hidden,R_", [(24, [32, 16], 1), (12, [9, 3], 4), (136, [256, 256], 4), (40, [], 3), (70, [100, 7], 15)])
def test_noise_matches_restatement(F, hidden, R_):
    from ultra_pytorch_amd import hip_ops
    P = hip_ops.DnnShape(F, hidden, "elu").n_params
    rng = np.random.RandomState(F + R_)
    theta = rng.uniform(-1, 1, size=P).astype(np.float32)
    mem = _memory(rng, F, hidden, R_, P)
    z = rng.standard_normal((R_, P)).astype(np.float32)
    rate = 0.37
    u, cand = run_noise(F, hidden, R_, mem, theta, rate, normals=z)
    ref = S.null_space_noise(z, mem, F, hidden)
    np.testing.assert_allclose(u, ref, atol=1e-5, rtol=0)
    np.testing.assert_allclose(cand, theta + rate * u, atol=1e-6, rtol=0)
    lay, _ = D.layout(F, hidden)
    for og, k, *_ in lay:
        assert (cand[:, og:og + 2 * k] == theta[og:og + 2 * k]).all()
    check_invariants(u, mem, F, hidden)
    if hidden == [9, 3]:  # the bias of 3 entries under 3 independent memory rows: spanned, so 0
        off, n, _ = S.tensors(F, hidden)[3]
        assert n == 3 and (u[:, off:off + n] == 0).all()
    # the empty memory: whole-tensor normalization of the normals (not DBGD's per column)
    u0, _ = run_noise(F, hidden, R_, np.zeros_like(mem), theta, rate, normals=z)
    for off, n, scalar in S.tensors(F, hidden):
        zt = z[:, off:off + n].astype(np.float64)
        np.testing.assert_allclose(u0[:, off:off + n], zt / np.sqrt((zt ** 2).sum(1, keepdims=True)), atol=1e-6)
    # the Philox draw against the host Philox
    up, _ = run_noise(F, hidden, R_, mem, theta, rate)
    np.testing.assert_allclose(up, S.null_space_noise(S.normals(SEED, STEP, R_, P), mem, F, hidden), atol=1e-5, rtol=0)
    check_invariants(up, mem, F, hidden)
    # the injected unit noise replaces the law on the Linear entries
    w = rng.standard_normal((R_, P)).astype(np.float32)
    uu, cu = run_noise(F, hidden, R_, mem, theta, rate, unit=w)
    lin = np.zeros(P, bool)
    for off, n, _ in S.tensors(F, hidden):
        lin[off:off + n] = True
    assert np.array_equal(uu[:, lin], w[:, lin]) and (uu[:, ~lin] == 0).all()
    np.testing.assert_allclose(cu, theta + rate * uu, atol=1e-6, rtol=0)


def run_memory(F, hidden, R, noise, mem0, need_interleave, winners=None, ndcg=None):
    from ultra_pytorch_amd import _lib, hip_ops
    shape = hip_ops.DnnShape(F, hidden, "elu")
    P = shape.n_params
    lib = _lib.load()
    nz, m = _cuda(noise), _cuda(mem0)
    W = _cuda(np.asarray(winners, np.float32)) if winners is not None else None
    nd = _cuda(np.asarray(ndcg, np.float32)) if ndcg is not None else None
    B = W.shape[0] if W is not None else 1
    a = _lib.DbgdArgs(desc=ctypes.pointer(shape.desc), n_params=P, n_rankers=R, batch=B, max_candidates=1, rank_list_size=1,
                      need_interleave=int(need_interleave), noise=_ptr(nz), winners=_ptr(W), ndcg=_ptr(nd))
    n = _lib.NsgdArgs(dbgd=ctypes.pointer(a), memory=_ptr(m))
    _lib.check(lib.ultr_nsgd_memory_args(ctypes.byref(n), hip_ops.raw_stream()), "ultr_nsgd_memory_args")
    torch.cuda.synchronize()
    return m.cpu().numpy()


def test_memory_kernel_rules():
    from ultra_pytorch_amd import hip_ops
    F, hidden, R = 20, [33, 7], 5
    P = hip_ops.DnnShape(F, hidden, "elu").n_params
    rng = np.random.RandomState(1)
    noise = rng.standard_normal((R, P)).astype(np.float32)
    mem0 = np.full((R, P), -7.0, np.float32)
    lin = np.zeros(P, bool)
    for off, n, _ in S.tensors(F, hidden):
        lin[off:off + n] = True

    def expect(lost):
        e = S.memory_update(noise, lost, F, hidden)
        e[:, ~lin] = -7.0  # only the Linear entries are written
        return e
    B = 300
    W = rng.uniform(size=(B, R + 1)).astype(np.float32) * (rng.uniform(size=(B, R + 1)) < 0.01)
    W[:, 2] = 0.0
    W[:, 4] = 0.0
    W[B - 1, 4] = 0.25  # only the last list credits ranker 4
    lost = S.losers(R, winners_BR=W)
    assert lost.tolist() == [bool(not W[:, r + 1].any()) for r in range(R)] and lost[1] and not lost[3]
    assert np.array_equal(run_memory(F, hidden, R, noise, mem0, True, winners=W), expect(lost))
    for nd in ([0.5, 0.4, 0.5, 0.3, 0.2, 0.5], [0.5, 0.4, 0.6, 0.3, 0.2, 0.5], [0.3] * 6):
        lost = S.losers(R, ndcg=nd)
        assert np.array_equal(run_memory(F, hidden, R, noise, mem0, False, ndcg=nd), expect(lost))


def _engine(F, hidden, B, M, rls, R_, memory=None, **kw):
    from ultra_pytorch_amd import engine, hip_ops
    shape = hip_ops.DnnShape(F, hidden, "elu")
    model, ex, n_exam, cprob = _click_model(kw.pop("cm", "pbm"))
    eng = engine.NsgdEngine(shape, B, M, rls, R_, torch.device("cuda"), memory=memory, click_model=model, exam=ex, n_exam=n_exam,
                            cprob=_cuda(cprob), **kw)
    return shape, eng


def _golden(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return d, json.loads(str(d["meta"]))


@pytest.mark.parametrize("name", ["nsgd_noint", "nsgd_ada", "nsgd_linear"])
def test_golden_train_step(name):
    d, m = _golden(name)
    F, hidden, M, cut, B, R = m["F"], m["hidden"] or [], m["M"], m["cutoff"], m["B"], m["R"]
    shape, eng = _engine(F, hidden, B, M, cut, R, need_interleave=False, noise_rate=m["lr"], learning_rate=m["lr"],
                         max_gradient_norm=m["max_gradient_norm"], optimizer=m["grad_strategy"])
    P = shape.n_params
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        ids, lab, feats = d[p + "docids"], d[p + "labels"], d[p + "features"]
        th0 = d[p + "pre_params"]
        params, state = _cuda(th0), _cuda(d[p + "pre_adagrad"])
        eng.memory.copy_(_cuda(d[p + "pre_memory"]))
        eng.train_step(params, state, _cuda(feats), feats.shape[0], _cuda(ids), _cuda(lab), unit_noise_in=_cuda(d[p + "unit_noise"]))
        loss = eng.read_loss()
        torch.cuda.synchronize()
        assert abs(loss - float(d[p + "loss"])) < 1e-5
        np.testing.assert_allclose(eng.ndcg.cpu().numpy(), d[p + "ndcg"], atol=1e-5)
        np.testing.assert_allclose(eng.scores[R].cpu().numpy(), d[p + "cand_scores"], atol=2e-5, rtol=1e-5)
        assert np.array_equal(eng.memory.cpu().numpy(), d[p + "post_memory"])
        np.testing.assert_allclose(eng.grads[:P].cpu().numpy(), -d[p + "grads"], atol=1e-6)
        sc = eng.scalars.cpu().numpy()
        assert abs(sc[1] - float(d[p + "norm"])) < 1e-5 and abs(sc[2] - float(d[p + "clip_coef"])) < 1e-6
        # the update steps TOWARD the winners: the reference's step mirrored about theta_pre
        np.testing.assert_allclose(params.cpu().numpy(), th0 - (d[p + "post_params"] - th0), atol=1e-6)
        np.testing.assert_allclose(state.cpu().numpy(), d[p + "post_adagrad"], rtol=1e-5, atol=1e-9)


def test_interleaved_step_and_its_memory():
    """A step the reference cannot run: the team-draft invariants hold, and the memory becomes the noise of exactly the rankers no list
    credited; the noise avoided the memory it started from."""
    rng = np.random.RandomState(8)
    F, hidden, B, M, rls, R_ = 24, [32, 16], 24, 12, 8, 4
    shape, eng = _engine(F, hidden, B, M, rls, R_, need_interleave=True, stochastic=True, learning_rate=0.1, noise_rate=0.1, seed=5)
    P = shape.n_params
    from ultra_pytorch_amd.ranking_model.dnn import init_flat_params
    p = init_flat_params(shape, seed=3).cuda()
    mem0 = _memory(rng, F, hidden, R_, P)
    eng.memory.copy_(_cuda(mem0))
    feats, ids, y, n_docs = _batch(rng, F, B, M)
    inter = torch.empty(M, B, dtype=torch.int32, device="cuda")
    teams = torch.empty(M, B, dtype=torch.int32, device="cuda")
    eng.train_step(p, None, _cuda(feats), n_docs, _cuda(ids), _cuda(y), interleaved=inter, teams=teams, step=2)
    eng.read_loss()
    torch.cuda.synchronize()
    inter, teams, W = inter.cpu().numpy(), teams.cpu().numpy(), eng.winners.cpu().numpy()
    for b in range(B):
        n = D.list_len(ids[:, b], n_docs)
        assert sorted(inter[:n, b].tolist()) == list(range(n))
        t = teams[:n, b]
        k = int(np.argmax(t >= 0)) if (t >= 0).any() else n
        assert (t[:k] == -1).all() and (t[k:] >= 0).all()
        rest = t[k:]
        for r0 in range(0, len(rest), R_ + 1):
            assert len(set(rest[r0:r0 + R_ + 1].tolist())) == len(rest[r0:r0 + R_ + 1])
    u = eng.noise.cpu().numpy()
    check_invariants(u, mem0, F, hidden)
    lost = S.losers(R_, winners_BR=W)
    assert np.array_equal(eng.memory.cpu().numpy(), S.memory_update(u, lost, F, hidden))
    np.testing.assert_allclose(u, S.null_space_noise(S.normals(5, 2, R_, P), mem0, F, hidden), atol=1e-5)


@pytest.mark.parametrize("need_interleave", [True, False])
def test_step_repeats_bitwise(need_interleave):
    rng = np.random.RandomState(5)
    F, hidden, B, M, rls, R_ = 24, [32, 16], 16, 12, 8, 4
    shape, eng = _engine(F, hidden, B, M, rls, R_, need_interleave=need_interleave, optimizer="ada", learning_rate=0.1,
                         noise_rate=0.1, seed=77)
    from ultra_pytorch_amd.ranking_model.dnn import init_flat_params
    p0 = init_flat_params(shape, seed=3).cuda()
    mem0 = _cuda(_memory(rng, F, hidden, R_, shape.n_params))
    feats, ids, y, n_docs = _batch(rng, F, B, M)
    f, i_, yy = _cuda(feats), _cuda(ids), _cuda(y)
    outs = []
    for _ in range(2):
        p, st = p0.clone(), torch.full_like(p0, 0.1)
        eng.memory.copy_(mem0)
        eng.train_step(p, st, f, n_docs, i_, yy, step=3)
        loss = eng.read_loss()
        torch.cuda.synchronize()
        outs.append((loss, p.cpu().numpy(), st.cpu().numpy(), eng.noise.cpu().numpy(), eng.memory.cpu().numpy(),
                     eng.grads.cpu().numpy()))
    assert outs[0][0] == outs[1][0]
    for x, z in zip(outs[0][1:], outs[1][1:]):
        assert np.array_equal(x, z)


# test_gpu_dbgd's setting and bar (+0.08) except learning_rate 0.8: the whole-tensor normalization gives the Linear model's [1, 16]
# weight row a unit noise where DBGD / MGD's per-column law gives +-1 per entry (norm 4), so 0.8 takes MGD's steps at 0.2.  The run
# that fixed these numbers: validation NDCG@10 0.559 -> 0.670 (MGD at 0.2: 0.721); at learning_rate 0.2 NSGD reaches 0.622 in 150
# steps and 0.666 in 300.
def test_online_training_raises_validation_ndcg(capsys):
    from ultra_pytorch_amd import input_layer
    F, M, cutoff, B, n_steps = 16, 10, 10, 32, 150
    torch.manual_seed(0)
    algo = make_algo(F, M, cutoff, None, hp="learning_rate=0.8", algo="NSGD", model="Linear")
    train, valid = LearnableDS(400, M, F, seed=1), LearnableDS(100, M, F, seed=2)
    feed = input_layer.DeviceStochasticOnlineSimulationFeed(algo, B, "oracle_mode=True", seed=4)
    n0 = _valid_ndcg(algo, valid, M)
    for _ in range(n_steps):
        f, _ = feed.get_batch(train, check_validation=True)
        loss, _, _ = algo.train(f)
    assert np.isfinite(loss) and algo.global_step == n_steps
    n1 = _valid_ndcg(algo, valid, M)
    with capsys.disabled():
        print("\nNSGD validation NDCG@10 %.4f -> %.4f" % (n0, n1))
    assert n1 > n0 + 0.08, (n0, n1)


@pytest.mark.parametrize("feed_name", ["StochasticOnlineSimulationFeed", "DeviceDeterministicOnlineSimulationFeed"])
def test_plugin_steps_and_keeps_its_memory(feed_name, capsys):
    from ultra_pytorch_amd import input_layer
    F, M = 16, 10
    algo = make_algo(F, M, 7, [8], algo="NSGD", hp="interleave_strategy=Deterministic,ranker_num=3")
    assert tuple(algo.memory.shape) == (3, algo.model.shape.n_params) and not algo.memory.any()
    ds = LearnableDS(64, M, F, seed=4)
    cls = getattr(input_layer, feed_name)
    feed = cls(algo, 16, "", seed=3) if feed_name.startswith("Device") else cls(algo, 16, "")
    p0 = algo.model.flat_params.clone()
    for step in range(4):
        f, _ = feed.get_batch(ds, check_validation=True)
        capsys.readouterr()
        loss, _, _ = algo.train(f)
        assert " Loss " not in capsys.readouterr().out  # nsgd.py prints no loss line
        assert np.isfinite(loss) and 0.0 <= loss <= 1.0
    assert algo.global_step == 4 and not torch.equal(p0, algo.model.flat_params)
    eng = next(iter(algo._train_engines.values()))
    assert eng.memory is algo.memory
    for name, shp, off in algo.model.shape.layout():
        if "layer_norm" in name:
            n = int(np.prod(shp))
            assert torch.equal(p0[off:off + n], algo.model.flat_params[off:off + n])
            assert not algo.memory[:, off:off + n].any()


def test_refusals():
    from ultra_pytorch_amd import _lib, hip_ops
    algo = make_algo(16, 10, 10, [8], algo="NSGD", hp="ranker_num=16")
    with pytest.raises(ValueError, match="candidate rankers"):
        algo._dbgd_engine(4, 10)
    with pytest.raises(NotImplementedError, match="DNN and Linear"):
        make_algo(16, 10, 10, None, algo="NSGD", model="SetRank.SetRank",
                  extra={"ranking_model_hparams": "d_model=32,num_heads=4,num_layers=1,diff=16"})
    with pytest.raises(NotImplementedError, match="data-parallel"):
        make_algo(16, 10, 10, [8], algo="NSGD", extra={"process_group": object()})
    algo = make_algo(16, 300, 10, [8], algo="NSGD")
    with pytest.raises(ValueError, match="up to 256"):
        algo._dbgd_engine(4, 300)
    # the C ABI: no memory, no workspace, too many rankers
    shape = hip_ops.DnnShape(16, [8], "elu")
    P = shape.n_params
    lib = _lib.load()
    assert lib.ultr_nsgd_workspace_bytes(ctypes.byref(shape.desc), 16) == -1
    buf = torch.zeros(16 * P, device="cuda")
    ws = torch.zeros(lib.ultr_nsgd_workspace_bytes(ctypes.byref(shape.desc), 2) // 8, dtype=torch.float64, device="cuda")
    a = _lib.DbgdArgs(desc=ctypes.pointer(shape.desc), n_params=P, n_rankers=2, batch=1, max_candidates=1, rank_list_size=1,
                      params=_ptr(buf), noise=_ptr(buf), cand_params=_ptr(buf))
    st = hip_ops.raw_stream()
    assert lib.ultr_nsgd_noise_args(ctypes.byref(_lib.NsgdArgs(dbgd=ctypes.pointer(a), ws=_ptr(ws))), st) == -1
    assert lib.ultr_nsgd_noise_args(ctypes.byref(_lib.NsgdArgs(dbgd=ctypes.pointer(a), memory=_ptr(buf))), st) == -1
    a.n_rankers = 16
    assert lib.ultr_nsgd_noise_args(ctypes.byref(_lib.NsgdArgs(dbgd=ctypes.pointer(a), memory=_ptr(buf), ws=_ptr(ws))), st) == -1
    a.n_rankers, a.need_interleave = 2, 1
    assert lib.ultr_nsgd_memory_args(ctypes.byref(_lib.NsgdArgs(dbgd=ctypes.pointer(a), memory=_ptr(buf))), st) == -1
    torch.cuda.synchronize()
