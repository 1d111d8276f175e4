"""DBGD / MGD on the GPU (csrc/ultr_dbgd.hip): the three kernels through the C ABI against the host restatement (tests/dbgd_ref.py) -
the noise to 1e-6, the multileave bit for bit in deterministic mode and wherever the race keys are separated in stochastic mode -,
the team-draft invariants, the reference's recorded steps (tests/golden/dbgd_*.npz) with injected noise, shuffles and clicks, the
step without interleaving, determinism, online training through the device feed, and the refusals."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import dbgd_ref as R
from tests import draw_ref as D
from tests import online_draw_ref as O
from tests.test_gpu_draws import _exam_image

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ultra_pytorch_amd", "data")
JSON = {"pbm": ("pbm_0.1_1.0_4_1.0.json", D.PBM), "cascade": ("cascade_0.1_1.0_4_1.0.json", D.CASCADE),
        "ubm": ("ubm_0.1_1_4_1.0.json", D.UBM)}
SEED, STEP = 0x0123456789ABCDEF, 2 ** 32 + 5


def _click_model(name, never=False):
    from ultra_pytorch_amd.utils import click_models
    desc = json.load(open(os.path.join(DATA, JSON[name][0])))
    if never:  # label 0 is never clicked: a list of zeros never clicks
        desc["click_prob"] = [0.0] + list(desc["click_prob"][1:])
    hm = click_models.loadModelFromJson(desc)
    ex, n = _exam_image(hm, JSON[name][1])
    return JSON[name][1], ex, n, np.asarray(desc["click_prob"], np.float32)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _cuda(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def _args(**kw):
    from ultra_pytorch_amd import _lib
    a = _lib.DbgdArgs()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


# ---- dbgd_noise_kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,hidden,R_", [(24, [32, 16], 1), (136, [256, 256], 4), (40, [], 3), (70, [100, 7], 15)])
def test_noise_matches_restatement(F, hidden, R_):
    from ultra_pytorch_amd import _lib, hip_ops
    shape = hip_ops.DnnShape(F, hidden, "elu")
    lay, P = R.layout(F, hidden)
    assert P == shape.n_params
    rng = np.random.RandomState(F)
    theta = rng.uniform(-1, 1, size=P).astype(np.float32)
    th = _cuda(theta)
    u = torch.full((R_, P), -7.0, device="cuda")
    cand = torch.full((R_, P), -7.0, device="cuda")
    rate = 0.37
    a = _args(desc=ctypes.pointer(shape.desc), n_params=P, n_rankers=R_, batch=1, max_candidates=1, rank_list_size=1,
              noise_rate=rate, seed=SEED, step=STEP, params=_ptr(th), noise=_ptr(u), cand_params=_ptr(cand))
    _lib.check(_lib.load().ultr_dbgd_noise_args(ctypes.addressof(a), hip_ops.raw_stream()), "ultr_dbgd_noise_args")
    torch.cuda.synchronize()
    got = u.cpu().numpy().astype(np.float64)
    ref = R.normalize(R.normals(SEED, STEP, R_, P), F, hidden)
    np.testing.assert_allclose(got, ref, atol=1e-6, rtol=0)
    np.testing.assert_allclose(cand.cpu().numpy(), theta + rate * ref, atol=1e-6, rtol=0)
    for (og, k, ow, m, ob) in lay:
        assert (got[:, og:og + 2 * k] == 0).all()  # LayerNorm: no noise
        W = got[:, ow:ow + m * k].reshape(R_, m, k)
        np.testing.assert_allclose(np.sqrt((W ** 2).sum(1)), 1.0, atol=1e-6)
        np.testing.assert_allclose(np.sqrt((got[:, ob:ob + m] ** 2).sum(1)), 1.0, atol=1e-6)
        if m == 1:
            assert set(np.unique(W)) <= {-1.0, 1.0}  # the scorer row is sign(z)
    assert (cand.cpu().numpy()[:, lay[0][0]:lay[0][0] + 2 * F] == theta[:2 * F]).all()
    # injected normals replace the draw
    z = rng.standard_normal((R_, P)).astype(np.float32)
    a.noise_in = _ptr(zt := _cuda(z))
    _lib.check(_lib.load().ultr_dbgd_noise_args(ctypes.addressof(a), hip_ops.raw_stream()), "ultr_dbgd_noise_args")
    torch.cuda.synchronize()
    np.testing.assert_allclose(u.cpu().numpy(), R.normalize(z.astype(np.float64), F, hidden), atol=1e-6, rtol=0)
    del zt


# ---- dbgd_interleave_kernel -----------------------------------------------------------------------------------------------
def _case(rng, NR, B, M, n_docs, prefix_lists=True, nan=True):
    """scores [NR, B, M] with ties and NaNs; docids [M, B] with interior and tail PADs; graded labels (garbage at PADs)."""
    base = rng.standard_normal((B, M)).astype(np.float32)
    sc = np.stack([base + rng.standard_normal((B, M)).astype(np.float32) * np.float32(rng.choice([0.0, 0.3, 2.0]))
                   for _ in range(NR)]).astype(np.float32)
    sc[rng.uniform(size=sc.shape) < 0.2] = np.float32(0.5)  # ties
    if nan:
        sc[rng.uniform(size=sc.shape) < 0.03] = np.float32("nan")
    if prefix_lists:  # lists whose rankings agree on a prefix: the top documents far above the rest for every ranker
        for b in range(0, B, 3):
            k = int(rng.randint(1, min(4, M) + 1))
            sc[:, b][np.isnan(sc[:, b])] = np.float32(0.0)  # (a NaN sorts first: no agreement)
            sc[:, b, :k] = np.float32(100.0) + np.arange(k, 0, -1, dtype=np.float32)[None, :]
    ids = rng.randint(0, n_docs, size=(M, B)).astype(np.int32)
    for b in range(B):
        n = int(rng.randint(0, M + 1)) if b % 5 else M
        ids[n:, b] = n_docs
        ids[rng.uniform(size=M) < 0.1, b] = n_docs  # interior PADs
    y = rng.randint(0, 5, size=(M, B)).astype(np.float32)
    y[rng.uniform(size=(M, B)) < 0.4] = 0.0
    y[:, B - 1] = 0.0  # a list that never clicks: winners 0 after 101 draws
    return sc, ids, y


def run_interleave(sc, ids, y, n_docs, rls, mode, tau, seed, step, max_redraws, model, ex, n_exam, cprob, shuffles=None,
                   clicks_in=None, rc_only=False, **extra):
    from ultra_pytorch_amd import _lib, hip_ops
    NR, B, M = sc.shape
    d_sc, d_ids, d_y = _cuda(sc), _cuda(ids), _cuda(y)
    cp = _cuda(np.asarray(cprob, np.float32))
    W = torch.full((B, NR), -7.0, device="cuda")
    inter = torch.full((M, B), -7, dtype=torch.int32, device="cuda")
    teams = torch.full((M, B), -7, dtype=torch.int32, device="cuda")
    clicks = torch.full((M, B), -7.0, device="cuda")
    ls = torch.full((B, rls), -7.0, device="cuda")
    sh = _cuda(np.asarray(shuffles, np.int32)) if shuffles is not None else None
    ci = _cuda(np.asarray(clicks_in, np.float32)) if clicks_in is not None else None
    kw = dict(n_params=1, n_rankers=NR - 1, batch=B, max_candidates=M, rank_list_size=rls, need_interleave=1, mode=mode,
              max_redraws=max_redraws, click_model=model, n_exam=n_exam, n_rel=len(cprob), tau=float(tau), seed=seed, step=step,
              scores=_ptr(d_sc), docids=_ptr(d_ids), n_docs=n_docs, labels=_ptr(d_y), exam_prob=_ptr(ex), click_prob=_ptr(cp),
              shuffles_in=_ptr(sh), clicks_in=_ptr(ci), winners=_ptr(W), interleaved=_ptr(inter), teams=_ptr(teams),
              clicks=_ptr(clicks), loss_scores=_ptr(ls))
    kw.update(extra)
    a = _args(**kw)
    rc = _lib.load().ultr_dbgd_interleave_args(ctypes.addressof(a), hip_ops.raw_stream())
    if rc_only:
        return rc
    _lib.check(rc, "ultr_dbgd_interleave_args")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ls.cpu().numpy(), sc[0, :, :rls])
    return W.cpu().numpy(), inter.cpu().numpy(), teams.cpu().numpy(), clicks.cpu().numpy()


@pytest.mark.parametrize("NR", [2, 5, 16])
@pytest.mark.parametrize("cm", ["pbm", "cascade", "ubm"])
def test_interleave_deterministic_bitwise(NR, cm):
    rng = np.random.RandomState(NR * 7 + len(cm))
    B, M, n_docs, rls = 37, 23, 500, 15
    model, ex, n_exam, cprob = _click_model(cm, never=True)
    sc, ids, y = _case(rng, NR, B, M, n_docs)
    got = run_interleave(sc, ids, y, n_docs, rls, O.DETERMINISTIC, 1.0, SEED, STEP, 100, model, ex, n_exam, cprob)
    ref = R.interleave(sc, ids, y, n_docs, rls, O.DETERMINISTIC, 1.0, SEED, STEP, 100, model, ex.cpu().numpy(), n_exam, cprob)
    for g, r_, name in zip(got, ref, ("winners", "interleaved", "teams", "clicks")):
        np.testing.assert_array_equal(g, r_, err_msg=name)
    assert (got[0][B - 1] == 0).all()  # never clicked
    assert (got[2] == -1).any()  # agreed prefixes were exercised


def test_interleave_long_lists_and_injection():
    """M = 256 (four chunks of 64 per wave), injected shuffles and clicks."""
    rng = np.random.RandomState(3)
    NR, B, M, n_docs, rls = 4, 9, 256, 10000, 200
    model, ex, n_exam, cprob = _click_model("pbm")
    sc, ids, y = _case(rng, NR, B, M, n_docs, nan=False)
    sh = np.stack([np.stack([rng.permutation(NR) for _ in range(M)]) for _ in range(B)]).astype(np.int32)
    ck = (rng.uniform(size=(M, B)) < 0.2).astype(np.float32)
    got = run_interleave(sc, ids, y, n_docs, rls, O.DETERMINISTIC, 1.0, SEED, 9, 100, model, ex, n_exam, cprob, shuffles=sh, clicks_in=ck)
    ref = R.interleave(sc, ids, y, n_docs, rls, O.DETERMINISTIC, 1.0, SEED, 9, 100, model, ex.cpu().numpy(), n_exam, cprob, shuffles=sh,
                       clicks_in=ck)
    for g, r_, name in zip(got, ref, ("winners", "interleaved", "teams", "clicks")):
        np.testing.assert_array_equal(g, r_, err_msg=name)
    got = run_interleave(sc, ids, y, n_docs, rls, O.DETERMINISTIC, 1.0, SEED, 9, 100, model, ex, n_exam, cprob)
    ref = R.interleave(sc, ids, y, n_docs, rls, O.DETERMINISTIC, 1.0, SEED, 9, 100, model, ex.cpu().numpy(), n_exam, cprob)
    for g, r_, name in zip(got, ref, ("winners", "interleaved", "teams", "clicks")):
        np.testing.assert_array_equal(g, r_, err_msg=name)


@pytest.mark.parametrize("cm", ["cascade", "ubm"])
def test_interleave_clicks_across_chunks(cm):
    """The two models that carry state from one chunk of 64 positions to the next, on lists of 130 positions with a few clickable
    documents each (label 0 is never clicked): the cascade's `a click in an earlier chunk` and the user-browsing model's `rank of the
    last click` must cross the chunk boundary as the restatement's sequential walk does."""
    NR, B, M, n_docs = 3, 48, 130, 10000
    rng = np.random.RandomState(11)
    sc = rng.standard_normal((NR, B, M)).astype(np.float32)
    ids = rng.randint(0, n_docs, size=(M, B)).astype(np.int32)
    y = np.zeros((M, B), np.float32)
    for b in range(B):
        y[rng.choice(M, 4 if b % 2 else 2, replace=False), b] = 4.0
    model, ex, n_exam, cprob = _click_model(cm, never=True)
    got = run_interleave(sc, ids, y, n_docs, M, O.DETERMINISTIC, 1.0, SEED, STEP, 100, model, ex, n_exam, cprob)
    ref = R.interleave(sc, ids, y, n_docs, M, O.DETERMINISTIC, 1.0, SEED, STEP, 100, model, ex.cpu().numpy(), n_exam, cprob)
    for g, r_, name in zip(got, ref, ("winners", "interleaved", "teams", "clicks")):
        np.testing.assert_array_equal(g, r_, err_msg=name)
    low, high = got[3][:64].sum(0), got[3][64:].sum(0)
    if cm == "cascade":
        assert ((low == 0) & (high == 1)).any()  # a list whose only click lies behind the first chunk
    else:
        assert ((low > 0) & (high > 0)).any()  # a list whose walk carries a click into the next chunk


@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_interleave_stochastic_matches_where_keys_are_separated(tau):
    rng = np.random.RandomState(int(tau))
    NR, B, M, n_docs, rls = 5, 64, 20, 3000, 12
    model, ex, n_exam, cprob = _click_model("pbm")
    sc, ids, y = _case(rng, NR, B, M, n_docs, nan=False)
    got = run_interleave(sc, ids, y, n_docs, rls, O.STOCHASTIC, tau, SEED, STEP, 100, model, ex, n_exam, cprob)
    ref = R.interleave(sc, ids, y, n_docs, rls, O.STOCHASTIC, tau, SEED, STEP, 100, model, ex.cpu().numpy(), n_exam, cprob)
    checked = 0
    for b in range(B):
        n = R.list_len(ids[:, b], n_docs)
        if n == 0:
            continue
        safe = True
        for j in range(NR):
            keys, zero, margin = O.race_keys(sc[j, b, :n], tau, R.race_uniforms(SEED, STEP, b, j, n))
            k = np.sort(keys[~zero])
            if (k.size > 1 and np.min(np.diff(k)) < 1e-4) or (n and np.min(margin) < 1e-3):
                safe = False
        if not safe:
            continue
        checked += 1
        np.testing.assert_array_equal(got[1][:, b], ref[1][:, b])
        np.testing.assert_array_equal(got[2][:, b], ref[2][:, b])
        np.testing.assert_array_equal(got[3][:, b], ref[3][:, b])
        np.testing.assert_array_equal(got[0][b], ref[0][b])
    assert checked >= B // 2


def test_team_draft_invariants():
    rng = np.random.RandomState(11)
    NR, B, M, n_docs, rls = 6, 50, 40, 4000, 40
    model, ex, n_exam, cprob = _click_model("cascade")
    sc, ids, y = _case(rng, NR, B, M, n_docs)
    W, inter, teams, clicks = run_interleave(sc, ids, y, n_docs, rls, O.STOCHASTIC, 1.0, SEED, 1, 100, model, ex, n_exam, cprob)
    for b in range(B):
        n = R.list_len(ids[:, b], n_docs)
        assert sorted(inter[:n, b].tolist()) == list(range(n))  # every document placed once
        assert (inter[n:, b] == -1).all() and (teams[n:, b] == -2).all()
        t = teams[:n, b]
        p = int(np.argmax(t >= 0)) if (t >= 0).any() else n
        assert (t[:p] == -1).all() and (t[p:] >= 0).all()
        rest = t[p:]
        for r0 in range(0, len(rest), NR):  # every round is a permutation of the rankers (team sizes differ by at most 1)
            blk = rest[r0:r0 + NR]
            assert len(set(blk.tolist())) == len(blk)
        team_clicks = clicks[:min(n, rls), b][t[:min(n, rls)] >= 0].sum()
        assert abs(float(W[b].sum()) - (1.0 if team_clicks > 0 else 0.0)) < 1e-6


# ---- the step ---------------------------------------------------------------------------------------------------------------
def _engine(F, hidden, B, M, rls, R_, **kw):
    from ultra_pytorch_amd import engine, hip_ops
    shape = hip_ops.DnnShape(F, hidden, "elu")
    model, ex, n_exam, cprob = _click_model(kw.pop("cm", "pbm"))
    eng = engine.DbgdEngine(shape, B, M, rls, R_, torch.device("cuda"), click_model=model, exam=ex, n_exam=n_exam,
                            cprob=_cuda(cprob), **kw)
    return shape, eng


def _batch(rng, F, B, M, pads=True):
    n_docs = B * M
    feats = rng.uniform(-1, 1, size=(n_docs, F)).astype(np.float32)
    ids = np.arange(n_docs, dtype=np.int32).reshape(B, M).T.copy()
    if pads:
        for b in range(B):
            n = int(rng.randint(1, M + 1))
            ids[n:, b] = n_docs
            if n > 3:
                ids[1, b] = n_docs
    y = rng.randint(0, 3, size=(M, B)).astype(np.float32)
    return feats, ids, y, n_docs


@pytest.mark.parametrize("need_interleave", [True, False])
def test_step_repeats_bitwise_and_follows_its_parts(need_interleave):
    rng = np.random.RandomState(5)
    F, hidden, B, M, rls, R_ = 24, [32, 16], 16, 12, 8, 4
    shape, eng = _engine(F, hidden, B, M, rls, R_, need_interleave=need_interleave, stochastic=True, optimizer="ada",
                         learning_rate=0.1, noise_rate=0.1, seed=77)
    from ultra_pytorch_amd.ranking_model.dnn import init_flat_params
    p0 = init_flat_params(shape, seed=3).cuda()
    feats, ids, y, n_docs = _batch(rng, F, B, M)
    f, i_, yy = _cuda(feats), _cuda(ids), _cuda(y)
    outs = []
    for _ in range(2):
        p = p0.clone()
        st = torch.full_like(p, 0.1)
        eng.train_step(p, st, f, n_docs, i_, yy, step=3)
        loss = eng.read_loss()
        torch.cuda.synchronize()
        outs.append((loss, p.cpu().numpy(), st.cpu().numpy(), eng.grads.cpu().numpy(), eng.winners.cpu().numpy(), eng.ndcg.cpu().numpy()))
    a, b = outs
    assert a[0] == b[0]
    for x, z in zip(a[1:], b[1:]):
        assert np.array_equal(x, z)
    loss, p1, s1, g, W, nd = a
    assert abs(loss - (1.0 - float(nd[0]))) < 1e-7
    u = eng.noise.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(u, R.normalize(R.normals(77, 3, R_, shape.n_params), F, hidden), atol=1e-6)
    c = R.ranker_weights(W if need_interleave else None, None if need_interleave else nd)
    np.testing.assert_allclose(g[:shape.n_params], R.gradient(u, c), atol=1e-6)
    # Adagrad on -g: state + g^2, theta - lr g / sqrt(state)
    gg = g[:shape.n_params].astype(np.float64)
    norm = np.sqrt((gg ** 2).sum())
    gc = gg * min(1.0, 5.0 / (norm + 1e-6))
    s_ref = 0.1 + gc ** 2
    np.testing.assert_allclose(s1, s_ref, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(p1, p0.cpu().numpy() - 0.1 * gc / (np.sqrt(s_ref) + 1e-10), atol=2e-6)


# ---- the reference's recorded steps ---------------------------------------------------------------------------------------------
def _golden(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return d, json.loads(str(d["meta"]))


# dbgd_sto's rankings are the reference's own Plackett-Luce draws (np.random.choice), which the race cannot be handed: its multileave
# is pinned on the host (tests/test_dbgd_cpu.py) and its race here, against the restatement
@pytest.mark.parametrize("name", ["dbgd_det", "dbgd_noint", "dbgd_ada", "dbgd_linear"])
def test_golden_train_step(name):
    d, m = _golden(name)
    F, hidden, M, cut, B = m["F"], m["hidden"] or [], m["M"], m["cutoff"], m["B"]
    shape, eng = _engine(F, hidden, B, M, cut, 1, need_interleave=m["need_interleave"],
                         stochastic=m["interleave_strategy"] == "Stochastic", tau=m["tau"], noise_rate=m["lr"], learning_rate=m["lr"],
                         max_gradient_norm=m["max_gradient_norm"], optimizer=m["grad_strategy"])
    P = shape.n_params
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        ids, lab, feats = d[p + "docids"], d[p + "labels"], d[p + "features"]
        assert ids.shape[1] == B
        th0, s0 = d[p + "pre_params"], d[p + "pre_adagrad"]
        params, state = _cuda(th0), _cuda(s0)
        kw = dict(noise_in=_cuda(d[p + "noise"]))
        if m["need_interleave"]:
            kw.update(shuffles_in=_cuda(d[p + "shuffles"]), clicks_in=_cuda(d[p + "clicks"]))
            inter = torch.empty(M, B, dtype=torch.int32, device="cuda")
            teams = torch.empty(M, B, dtype=torch.int32, device="cuda")
            kw.update(interleaved=inter, teams=teams)
        eng.train_step(params, state, _cuda(feats), feats.shape[0], _cuda(ids), _cuda(lab), **kw)
        loss = eng.read_loss()
        torch.cuda.synchronize()
        assert abs(loss - float(d[p + "loss"])) < 1e-5
        np.testing.assert_allclose(eng.scores[0, :, :].cpu().numpy(), d[p + "scores"][:, :eng.L], atol=1e-5, rtol=1e-5)
        np.testing.assert_allclose(eng.scores[1].cpu().numpy(), d[p + "cand_scores"], atol=2e-5, rtol=1e-5)
        if m["need_interleave"]:
            n_docs = feats.shape[0]
            for b in range(B):
                n = R.list_len(ids[:, b], n_docs)
                np.testing.assert_array_equal(inter.cpu().numpy()[:n, b], d[p + "interleaved"][:n, b])
                np.testing.assert_array_equal(teams.cpu().numpy()[:n, b], d[p + "teams"][:n, b])
            np.testing.assert_allclose(eng.winners.cpu().numpy(), d[p + "winners"], rtol=1e-6, atol=1e-7)
        g = eng.grads[:P].cpu().numpy()
        np.testing.assert_allclose(g, -d[p + "grads"], atol=1e-6)
        sc = eng.scalars.cpu().numpy()
        assert abs(sc[1] - float(d[p + "norm"])) < 1e-5 and abs(sc[2] - float(d[p + "clip_coef"])) < 1e-6
        # the update steps TOWARD the winners: the reference's step mirrored about theta_pre
        np.testing.assert_allclose(params.cpu().numpy(), th0 - (d[p + "post_params"] - th0), atol=1e-6)
        np.testing.assert_allclose(state.cpu().numpy(), d[p + "post_adagrad"], rtol=1e-5, atol=1e-9)


# ---- the plugin ----------------------------------------------------------------------------------------------------------------
class LearnableDS:
    """Queries whose relevance is a noisy function of the features (a fixed linear score): a ranker can learn it."""

    def __init__(self, n_queries, M, F, seed, w_seed=0):
        rng, wr = np.random.RandomState(seed), np.random.RandomState(w_seed)
        w = wr.standard_normal(F)
        self.feature_size, self.features, self.initial_list, self.labels, self.dids, self.qids = F, [], [], [], [], []
        did = 0
        for q in range(n_queries):
            x = rng.uniform(-1, 1, size=(M, F)).astype(np.float32)
            s = x @ w / np.sqrt(F) * 3.0 + rng.standard_normal(M) * 0.3
            lab = np.clip(np.round(s + 1.0), 0, 4).astype(int)
            self.features += x.tolist()
            self.initial_list.append(list(range(did, did + M)))
            self.labels.append([int(v) for v in lab])
            self.dids += ["d%d" % i for i in range(did, did + M)]
            self.qids.append("q%d" % q)
            did += M
        self.rank_list_size = M


def make_algo(F, M, cutoff, hidden, hp="", algo="DBGD", model="DNN", extra=None):
    from ultra_pytorch_amd.utils import find_class
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm." + algo, "learning_algorithm_hparams": hp,
           "ranking_model": "ultra_pytorch_amd.ranking_model." + model,
           "ranking_model_hparams": "hidden_layer_sizes=%s" % json.dumps(hidden) if hidden is not None else "",
           "max_candidate_num": M, "selection_bias_cutoff": cutoff, "metrics": ["ndcg"], "metrics_topn": [10]}
    exp.update(extra or {})
    return find_class(exp["learning_algorithm"])(LearnableDS(2, M, F, 0), exp)


def _valid_ndcg(algo, ds, M):
    n = len(ds.initial_list)
    feed = {"letor_features": np.asarray(ds.features, np.float32)}
    for l in range(M):
        feed["docid_input%d" % l] = np.array([ds.initial_list[q][l] for q in range(n)], np.float32)
        feed["label%d" % l] = np.array([ds.labels[q][l] for q in range(n)], np.float32)
    return algo.validation(feed)[2]["ndcg_10"]


# Linear model, learning_rate 0.2, batch 32, the device stochastic feed in oracle mode (DBGD's own click model then draws on the
# relevance labels), 150 steps.  The run that fixed these numbers: validation NDCG@10 0.559 -> 0.771 (DBGD) and 0.559 -> 0.721 (MGD,
# 4 candidates); at 300 steps 0.654 and 0.732 (online DBGD is noisy).  The bar is half the smaller gain: +0.08.
@pytest.mark.parametrize("algo_name", ["DBGD", "MGD"])
def test_online_training_raises_validation_ndcg(algo_name, capsys):
    from ultra_pytorch_amd import input_layer
    F, M, cutoff, B, n_steps = 16, 10, 10, 32, 150
    torch.manual_seed(0)
    algo = make_algo(F, M, cutoff, None, hp="learning_rate=0.2", algo=algo_name, model="Linear")
    train, valid = LearnableDS(400, M, F, seed=1), LearnableDS(100, M, F, seed=2)
    feed = input_layer.DeviceStochasticOnlineSimulationFeed(algo, B, "oracle_mode=True", seed=4)
    n0 = _valid_ndcg(algo, valid, M)
    for _ in range(n_steps):
        f, _ = feed.get_batch(train, check_validation=True)
        loss, _, _ = algo.train(f)
    assert np.isfinite(loss) and algo.global_step == n_steps
    n1 = _valid_ndcg(algo, valid, M)
    with capsys.disabled():
        print("\n%s validation NDCG@10 %.4f -> %.4f" % (algo_name, n0, n1))
    assert n1 > n0 + 0.08, (n0, n1)


@pytest.mark.parametrize("feed_name", ["ClickSimulationFeed", "DeviceClickFeed", "StochasticOnlineSimulationFeed",
                                       "DeterministicOnlineSimulationFeed", "DeviceDeterministicOnlineSimulationFeed"])
def test_plugin_on_every_feed(feed_name, capsys):
    from ultra_pytorch_amd import input_layer
    F, M = 16, 10
    cutoff = M if feed_name == "ClickSimulationFeed" else 7  # (the click feed's lists are selection_bias_cutoff long)
    algo = make_algo(F, M, cutoff, [8], algo="MGD", hp="interleave_strategy=Deterministic,ranker_num=3")
    ds = LearnableDS(64, M, F, seed=4)
    cls = getattr(input_layer, feed_name)
    feed = cls(algo, 16, "", seed=3) if feed_name.startswith("Device") else cls(algo, 16, "")
    p0 = algo.model.flat_params.clone()
    for step in range(3):
        f, _ = feed.get_batch(ds, check_validation=True)
        capsys.readouterr()
        loss, out, summary = algo.train(f)
        assert " Loss %f at Global Step %d: " % (loss, step + 1) in capsys.readouterr().out
        assert np.isfinite(loss) and 0.0 <= loss <= 1.0
    assert algo.global_step == 3 and not torch.equal(p0, algo.model.flat_params)
    ln = algo.model.shape.layout()
    for name, shp, off in ln:  # LayerNorm parameters never move
        if "layer_norm" in name:
            n = int(np.prod(shp))
            assert torch.equal(p0[off:off + n], algo.model.flat_params[off:off + n])


def test_refusals():
    from ultra_pytorch_amd import _lib, hip_ops
    algo = make_algo(16, 10, 10, [8], algo="MGD", hp="ranker_num=16")
    with pytest.raises(ValueError, match="candidate rankers"):
        algo._dbgd_engine(4, 10)
    with pytest.raises(NotImplementedError, match="DNN and Linear"):
        make_algo(16, 10, 10, None, model="SetRank.SetRank", extra={"ranking_model_hparams": "d_model=32,num_heads=4,num_layers=1,diff=16"})
    with pytest.raises(NotImplementedError, match="data-parallel"):
        make_algo(16, 10, 10, [8], extra={"process_group": object()})
    algo = make_algo(16, 300, 10, [8])
    with pytest.raises(ValueError, match="up to 256"):
        algo._dbgd_engine(4, 300)
    # the C ABI: M > 256, R + 1 > 16, rank_list_size > M
    model, ex, n_exam, cprob = _click_model("pbm")
    sc, ids, y = _case(np.random.RandomState(0), 2, 4, 10, 100)
    for kw in (dict(max_candidates=257), dict(n_rankers=16), dict(rank_list_size=11)):
        rc = run_interleave(sc, ids, y, 100, 10, O.DETERMINISTIC, 1.0, 0, 0, 100, model, ex, n_exam, cprob, rc_only=True, **kw)
        assert rc == -1  # ULTR_E_BADARG
    shape = hip_ops.DnnShape(16, [8], "elu")
    a = _args(desc=ctypes.pointer(shape.desc), n_params=shape.n_params + 1, n_rankers=1, batch=1, max_candidates=1, rank_list_size=1)
    assert _lib.load().ultr_dbgd_noise_args(ctypes.addressof(a), hip_ops.raw_stream()) == -1
    torch.cuda.synchronize()
