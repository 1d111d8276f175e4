"""The trust-bias click model (ULTR_CLICK_TRUST) on the device, bit for bit against tests/trust_ref.py: through ultr_click_batch, as a
rider of the update launch, through ultr_propensity_count (both of its kernels), ultr_online_rerank_args and
ultr_dbgd_interleave_args; and ids 0 / 1 / 2 drawn in the same process against tests/draw_ref.py as before.

The clicks of ultr_click_batch are checked a second time, independently of the device's image: the kernel's uniforms replayed through
the host TrustBiasModel's own tables in float64.  Left out are only draws within MARGIN = 8 * 2^-24 of their threshold (the float32
roundings of alpha, beta, the product and the sum: a few ulps of a probability <= 1 - tests/test_gpu_draws.py's margin, for the same
reason); their share is capped at CLOSE_CAP = 1e-4 of the draws (expected: 2 * MARGIN ~ 1e-6; the seeds below were confirmed on the
CPU with the restatement)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import draw_ref as R
from tests import trust_ref as T
from tests.test_gpu_draws import BIG_STEP, HI_SEED, MARGIN, make_data, run_click

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ultra_pytorch_amd", "data")
SHIPPED = os.path.join(DATA, "trust_0.1_1.0_4_1.0.json")
CLOSE_CAP = 1e-4


def model_desc(kind):
    d = json.load(open(SHIPPED))
    if kind == "trust3":  # three rows: ranks 2 .. saturate
        d.update(exam_prob=[0.9, 0.5, 0.2], trust_pos=[0.95, 0.9, 0.8], trust_neg=[0.5, 0.2, 0.05])
    if kind == "trust_never":  # no trust in an unattractive document, labels 0 and 1 never attract: such a list never clicks
        d.update(click_prob=[0.0, 0.0, 0.5, 0.8, 1.0], trust_neg=[0.0] * 10)
    return d


CASES = {  # name: (model, L, B, lmax, n_queries, labels, seed, step, max_tries)
    "L1_B1_one_query": ("trust", 1, 1, 1, 1, "graded", 0, 0, 100),
    "L10_B5_three_queries": ("trust", 10, 5, 10, 3, "graded", 7, 1, 1),
    "L63_lmax40_wide_labels": ("trust", 63, 4096, 40, 1000, "wide", HI_SEED, BIG_STEP, 3),
    "L64_B5": ("trust", 64, 5, 64, 100, "wide", 3, 1, 100),
    "L65_B4096": ("trust", 65, 4096, 65, 100, "graded", 11, 0, 3),
    "L130_B4096": ("trust", 130, 4096, 130, 3, "wide", HI_SEED, 1, 100),
    "three_rows_L65": ("trust3", 65, 4096, 65, 100, "graded", 5, BIG_STEP, 2),
    "max_tries_exhausted": ("trust_never", 64, 4096, 64, 100, "graded", 17, 1, 3),
}


def case_inputs(name):
    from ultra_pytorch_amd.utils import click_models
    kind, L, B, lmax, n_queries, labels, seed, step, max_tries = CASES[name]
    desc = model_desc(kind)
    hm = click_models.loadModelFromJson(desc)
    lists, lab = make_data(100 + list(CASES).index(name), n_queries, lmax, 5000, ragged=lmax > 1, labels=labels,
                           never_frac=0.3 if kind.endswith("never") else 0.0)
    return desc, hm, lists, lab


def restated(name):
    """(restatement outputs, number of draws the second check leaves out, draws) - needs no GPU."""
    kind, L, B, lmax, n_queries, labels, seed, step, max_tries = CASES[name]
    desc, hm, lists, lab = case_inputs(name)
    image, n_exam = T.image_of(hm)
    out = T.click_draw(lists, lab, 5000, image, n_exam, desc["click_prob"], seed, step, B, L, max_tries)
    return out, T.replay(hm, out[1], out[4], out[5], MARGIN), L * B


@pytest.mark.parametrize("name", list(CASES))
def test_click_batch_is_the_restatement_bit_for_bit(name):
    from ultra_pytorch_amd.utils import click_models
    kind, L, B, lmax, n_queries, labels, seed, step, max_tries = CASES[name]
    desc, hm, lists, lab = case_inputs(name)
    exam, n_exam, _ = click_models.device_tables(hm, 3, torch.device("cuda"))
    assert tuple(exam.shape) == (2, n_exam)
    ids, ck, q = run_click(lists, lab, 5000, exam, n_exam, desc["click_prob"], T.TRUST, seed, step, B, L, max_tries)  # sentinel-filled
    (r_ids, r_ck, r_q, kept, u, y), _, _ = restated(name)
    np.testing.assert_array_equal(q, r_q)
    np.testing.assert_array_equal(ids, r_ids)
    np.testing.assert_array_equal(ck, r_ck)
    assert set(np.unique(ck)) <= {0.0, 1.0}
    # second, independent check: the host model's own tables in float64
    n_close = T.replay(hm, ck, u, y, MARGIN)
    print("%s: %d of %d draws within %.1e of the threshold" % (name, n_close, L * B, MARGIN))
    assert n_close <= max(CLOSE_CAP * L * B, 0)
    got = ck.sum(0)
    if kind == "trust_never":
        stuck = got == 0
        assert stuck.any() and (kept[stuck] == max_tries - 1).all()
    elif B > 100:
        assert got.mean() > 1.0 and ck[0].mean() > 0.4  # trust bias: rank 0 is clicked far beyond exam x click_prob
    if lmax < L:
        assert (ids[lmax:] == 5000).all()


def test_rider_of_the_update_launch_draws_the_restatement():
    """Two IPWrank.train(DeviceClickFeed.get_batch(...)) steps with the shipped trust JSON: the batch after each step was drawn by the
    rider of that step's update launch and must be the restatement's for (seed, step)."""
    from tests.test_gpu_feed import DS
    from ultra_pytorch_amd.input_layer import DeviceClickFeed
    from ultra_pytorch_amd.utils import find_class
    F, L, B, seed = 16, 70, 61, HI_SEED
    ds = DS(120, (30, 70), F, seed=12)
    ds.pad(L)
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.IPWrank", "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=[32,16]",
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3]}
    algo = find_class(exp["learning_algorithm"])(ds, exp)
    feed = DeviceClickFeed(algo, B, "click_model_json=%s" % SHIPPED, seed=seed)
    assert feed.model_id == 3 and tuple(feed.exam.shape) == (2, 10)
    rd = feed.resident(ds)
    lists, lab = rd.lists.cpu().numpy(), rd.labels.cpu().numpy()
    image, cprob = feed.exam.cpu().numpy().reshape(-1), feed.cprob.cpu().numpy()
    assert np.array_equal(image, T.image_of(feed.click_model)[0])
    for step in range(3):
        f, info = feed.get_batch(ds, check_validation=True)
        ids, ck, q = f["docids"].cpu().numpy(), f["labels"].cpu().numpy(), info["rank_list_idxs"].cpu().numpy()
        r_ids, r_ck, r_q, _, u, y = T.click_draw(lists, lab, rd.n_docs, image, feed.n_exam, cprob, seed, step, B, L, 100)
        np.testing.assert_array_equal(q, r_q, err_msg="step %d" % step)
        np.testing.assert_array_equal(ids, r_ids, err_msg="step %d" % step)
        np.testing.assert_array_equal(ck, r_ck, err_msg="step %d" % step)
        if step < 2:
            assert np.isfinite(algo.train(f)[0])
            assert feed._pre == (id(ds), 100)  # the next batch was handed to the step (drawn ahead), not left for get_batch


def test_eta_drift_rebuilds_alpha_and_beta():
    """DeviceClickFeed rebuilds its image through device_tables when the bias severity moves: alpha and beta follow exam_prob."""
    import types
    from ultra_pytorch_amd.input_layer import DeviceClickFeed
    hm = T.shipped_model()
    before = DeviceClickFeed._exam_tensor(types.SimpleNamespace(click_model=hm, model_id=3, device=torch.device("cuda")))[0].cpu().numpy()
    hm.setExamProb(0.5)
    after, n = DeviceClickFeed._exam_tensor(types.SimpleNamespace(click_model=hm, model_id=3, device=torch.device("cuda")))
    assert n == 10 and tuple(after.shape) == (2, 10) and np.array_equal(after.cpu().numpy().reshape(-1), T.image_of(hm)[0])
    assert (after.cpu().numpy() > before).all()  # exam^0.5 > exam: both rows grow


@pytest.mark.parametrize("lmax", [10, 40])  # the packed kernel (16-lane segments) and one wavefront per session
def test_propensity_count_is_exact(lmax):
    from tests.test_gpu_propensity import dataset
    from ultra_pytorch_amd import hip_ops
    hm = T.shipped_model()
    image, n_exam = T.image_of(hm)
    cprob = np.asarray(hm.click_prob, np.float32)
    labels, lengths = dataset(lmax)
    n_sessions, first = 4096, 2 ** 32 - 5
    want = T.click_count(labels, lengths, image, n_exam, cprob, HI_SEED, first, n_sessions)
    dev = torch.device("cuda")
    table = torch.zeros(lmax, lmax, dtype=torch.int64, device=dev)
    hip_ops.propensity_count(torch.from_numpy(labels).to(dev), torch.from_numpy(lengths).to(dev), torch.from_numpy(image).to(dev), n_exam,
                             torch.from_numpy(cprob).to(dev), T.TRUST, HI_SEED, first, n_sessions, table)
    torch.cuda.synchronize()
    got = table.cpu().numpy()
    print("lmax %d: %d clicks, %d differing cells" % (lmax, int(want.sum()), int((got != want).sum())))
    assert want.sum() > n_sessions // 2 and want[lmax - 1].sum() > 0 and want[0, 0] > 0
    assert got.dtype == np.int64 and np.array_equal(got, want)


def test_online_rerank_clicks_replay_from_the_returned_order():
    from tests import online_draw_ref as O
    from tests.test_gpu_online_feed import _candidates, run_rerank
    hm = T.shipped_model()
    image, n_exam = T.image_of(hm)
    cprob = np.asarray(hm.click_prob, np.float32)
    M, cutoff, B, n_docs, seed, step, redraws = 70, 66, 512, 100000, HI_SEED, BIG_STEP, 100
    ids, y, s = _candidates(M * 31 + cutoff, B, M, n_docs)
    rc, got_ids, got_y, got_perm = run_rerank(ids, y, s, n_docs, seed, step, O.DETERMINISTIC, 1, cutoff, redraws, False, T.TRUST,
                                              torch.from_numpy(image).cuda(), n_exam, cprob)
    assert rc == 0
    # the order does not depend on the click model: the oracle-mode restatement gives it, with the true labels in that order
    want_ids, true_y, want_perm, _ = O.rerank(ids, y, s, n_docs, seed, step, O.DETERMINISTIC, 1, cutoff, redraws, True, R.PBM,
                                              image[:n_exam], n_exam, cprob)
    np.testing.assert_array_equal(got_perm, want_perm)
    np.testing.assert_array_equal(got_ids, want_ids)
    lens = O.list_len(ids, n_docs)
    want_y, redrawn = np.zeros((M, B), np.float32), 0
    for b in range(B):
        cut = min(int(lens[b]), cutoff)
        if cut > 0:
            labels_in_order = y[got_perm[:cut, b], b]
            np.testing.assert_array_equal(labels_in_order, true_y[:cut, b])
            want_y[:cut, b], kept = T.redrawn_clicks(labels_in_order, lambda a, b=b, cut=cut: O.click_uniforms(seed, step, b, a, cut), image,
                                                     n_exam, cprob, redraws)
            redrawn += kept > 0
    np.testing.assert_array_equal(got_y, want_y)
    assert got_y.any() and (lens > 64).any() and redrawn > 0


def test_dbgd_interleave_clicks_replay_from_the_returned_order():
    from tests import dbgd_ref as G
    from tests import online_draw_ref as O
    from tests.test_gpu_dbgd import _case, run_interleave
    hm = T.shipped_model()
    image, n_exam = T.image_of(hm)
    cprob = np.asarray(hm.click_prob, np.float32)
    rng = np.random.RandomState(41)
    NR, B, M, n_docs, rls, seed, step, redraws = 3, 37, 70, 500, 66, HI_SEED, BIG_STEP, 100
    sc, ids, y = _case(rng, NR, B, M, n_docs)
    W, inter, teams, clicks = run_interleave(sc, ids, y, n_docs, rls, O.DETERMINISTIC, 1.0, seed, step, redraws, T.TRUST,
                                             torch.from_numpy(image).cuda(), n_exam, cprob)
    # interleaving and teams do not depend on the click model: the restatement with injected clicks gives them
    _, r_inter, r_teams, _ = G.interleave(sc, ids, y, n_docs, rls, O.DETERMINISTIC, 1.0, seed, step, redraws, R.PBM, image[:n_exam], n_exam,
                                          cprob, clicks_in=np.zeros((M, B), np.float32))
    np.testing.assert_array_equal(inter, r_inter)
    np.testing.assert_array_equal(teams, r_teams)
    want, want_W = np.zeros((M, B), np.float32), np.zeros((B, NR), np.float32)
    for b in range(B):
        cut = min(G.list_len(ids[:, b], n_docs), rls)
        if cut > 0:
            yb = y[inter[:cut, b], b]
            want[:cut, b], _ = T.redrawn_clicks(yb, lambda a, b=b, cut=cut: G.click_uniforms(seed, step, b, a, cut), image, n_exam, cprob, redraws)
        want_W[b] = G.winners(teams[:cut, b], want[:cut, b], NR)
    np.testing.assert_array_equal(clicks, want)
    np.testing.assert_array_equal(W, want_W)
    assert clicks.any()


def test_the_other_models_still_match_their_restatement():
    """Ids 0 / 1 / 2 in the same process, after the trust model ran: the shared walk kept their bits."""
    from tests.test_gpu_draws import _exam_image, _model_desc
    from ultra_pytorch_amd.utils import click_models
    hm_t = T.shipped_model()
    exam_t, n_t, _ = click_models.device_tables(hm_t, 3, torch.device("cuda"))
    lists, lab = make_data(9, 100, 70, 5000)
    run_click(lists, lab, 5000, exam_t, n_t, hm_t.click_prob, T.TRUST, 1, 2, 64, 70, 3)
    for kind, model in (("pbm", R.PBM), ("cascade", R.CASCADE), ("ubm", R.UBM)):
        desc = _model_desc(kind)
        hm = click_models.loadModelFromJson(desc)
        exam, n_exam = _exam_image(hm, model)
        ids, ck, q = run_click(lists, lab, 5000, exam, n_exam, desc["click_prob"], model, HI_SEED, BIG_STEP, 257, 70, 3)
        r_ids, r_ck, r_q, _, _, _ = R.click_draw(lists, lab, 5000, exam.cpu().numpy(), n_exam, desc["click_prob"], model, HI_SEED, BIG_STEP,
                                                 257, 70, 3)
        np.testing.assert_array_equal(q, r_q)
        np.testing.assert_array_equal(ids, r_ids)
        np.testing.assert_array_equal(ck, r_ck, err_msg=kind)


# ---- the Python layers that take a click model, with the shipped trust JSON ---------------------------------------------------------
def test_randomized_estimator_counts_the_restatements_clicks():
    """RandomizedPropensityEstimator.estimateParametersFromModel under the trust model: its counts are the restatement's, its table
    the examination-only one those counts give."""
    from tests.test_gpu_propensity import dataset
    from ultra_pytorch_amd.utils import propensity_estimator as PE
    hm = T.shipped_model()
    image, n_exam = T.image_of(hm)
    padded, lengths = dataset(10)

    class Data(object):
        rank_list_size = 10
        labels = [[float(v) for v in row[:n]] for row, n in zip(padded, lengths)]

    est = PE.RandomizedPropensityEstimator()
    est.estimateParametersFromModel(hm, Data(), session_num=4096, seed=HI_SEED)
    want = T.click_count(padded, lengths, image, n_exam, np.asarray(hm.click_prob, np.float32), HI_SEED, 0, 4096)
    assert est.click_model is hm and np.array_equal(est.click_count, want) and want.sum() > 2048
    assert est.IPW_list == PE.ipw_from_click_count(want) and len(est.IPW_list) == 10


@pytest.mark.parametrize("mode", ["deterministic", "stochastic"])
def test_device_online_feed_draws_trust_clicks_and_pdgd_trains(mode, capsys):
    from tests.test_gpu_online_feed import DS, _feed, make_algo
    F, M, cutoff, B = 16, 12, 8, 256
    algo = make_algo(F, M, cutoff, [8])
    feed = _feed(algo, B, mode, hp="click_model_json=%s" % SHIPPED, seed=3)
    assert feed.model_id == 3 and tuple(feed.exam.shape) == (2, 10) and type(feed.click_model).__name__ == "TrustBiasModel"
    assert np.array_equal(feed.exam.cpu().numpy().reshape(-1), T.image_of(feed.click_model)[0])
    ds = DS(200, M, F, seed=5)
    f, _ = feed.get_batch(ds, check_validation=True)
    ck = f["labels"].cpu().numpy()
    assert set(np.unique(ck)) <= {0.0, 1.0} and not ck[cutoff:].any() and (ck.sum(0) > 0).all()
    # whatever stands at rank 0, one attempt clicks it with at least alpha_0 click_prob[0] + beta_0 = 0.465 (beta_0 alone is 0.442)
    assert ck[0].mean() > 0.35
    loss, _, _ = algo.train(f)
    capsys.readouterr()
    assert np.isfinite(loss)


@pytest.mark.parametrize("algo_name", ["DBGD", "MGD", "NSGD"])
def test_interleaving_learners_take_the_trust_json(algo_name, capsys):
    from tests.test_gpu_dbgd import LearnableDS, make_algo
    from ultra_pytorch_amd import input_layer
    F, M, B = 16, 10, 16
    algo = make_algo(F, M, 7, [8], algo=algo_name, hp="click_model_json=%s" % SHIPPED)
    assert algo.click_model_id == 3 and tuple(algo.exam.shape) == (2, 10) and algo.n_exam == 10
    ds = LearnableDS(64, M, F, seed=4)
    feed = input_layer.DeviceStochasticOnlineSimulationFeed(algo, B, "oracle_mode=True", seed=3)  # the learner's own model draws the clicks
    p0 = algo.model.flat_params.clone()
    for _ in range(2):
        f, _ = feed.get_batch(ds, check_validation=True)
        loss, _, _ = algo.train(f)
        assert np.isfinite(loss) and 0.0 <= loss <= 1.0
    capsys.readouterr()
    assert algo.global_step == 2 and not torch.equal(p0, algo.model.flat_params)
