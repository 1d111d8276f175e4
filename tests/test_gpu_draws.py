"""The device draws bit for bit: click_draw (csrc/ultr_feed.h) through its own launch (ultr_click_batch) and as a rider on the update
launch (ultr_feed_train_step), and RegressionEM's Bernoulli pseudo-labels from the device Philox stream (regem_kernel, uniforms ==
NULL) - against the host restatements of tests/draw_ref.py.  The clicks are checked a second time, independently of the device's
table image, by replaying the same uniforms through the host click models (ultra_pytorch_amd/utils/click_models.py) in float64.
The distributional tests of tests/test_gpu_feed.py stay: they compare with the reference's Mersenne-Twister feed, these do not."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import draw_ref as R
from tests.test_gpu_feed import DS

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ultra_pytorch_amd", "data")
HI_SEED = 0x123456789ABCDEF0
BIG_STEP = 2 ** 32 + 3
MARGIN = 8 * 2.0 ** -24  # float32 rounding of exam, click_prob and their product / quotient: a few ulps of a probability <= 1


def _desc(name):
    return json.load(open(os.path.join(DATA, name)))


def _three_row_ubm():
    return {"model_name": "user_browsing_model", "eta": 1.0, "click_prob": [0.1, 0.3, 0.5, 0.7, 0.9],
            "exam_prob": [[0.9], [0.7, 0.95], [0.85, 0.45, 0.6]]}


def _small_pbm():
    return {"model_name": "position_biased_model", "eta": 1.0, "click_prob": [0.1, 0.16, 0.28, 0.52, 1.0], "exam_prob": [0.9, 0.5, 0.2]}


def _low_cascade():  # first clicks reach the second and third 64-position chunk
    d = _desc("cascade_0.1_1.0_4_1.0.json")
    d["click_prob"] = [0.004, 0.01, 0.02, 0.03, 0.05]
    return d


def _never(desc):  # labels 0 and 1 are never clicked: a query without a label >= 2 can never produce a click
    d = dict(desc)
    d["click_prob"] = [0.0, 0.0, 0.5, 0.8, 1.0]
    return d


def _exam_image(hm, model_id):
    """The device table, built by the feed's own image code (DeviceClickFeed._exam_tensor) from the host model."""
    from ultra_pytorch_amd.input_layer import DeviceClickFeed
    ex, n = DeviceClickFeed._exam_tensor(types.SimpleNamespace(click_model=hm, model_id=model_id, device=torch.device("cuda")))
    return ex, n


def make_data(seed, n_queries, lmax, n_docs, ragged=True, labels="graded", never_frac=0.0):
    """lists [n_queries, lmax] (-1 = PAD, ragged tails and a few PAD holes), labels [n_queries, lmax] float32; PAD positions carry
    garbage labels (the kernel must read them as 0)."""
    rng = np.random.RandomState(seed)
    lists = rng.randint(0, n_docs, size=(n_queries, lmax)).astype(np.int32)
    if ragged:
        lens = rng.randint(1, lmax + 1, size=n_queries)
        lists[np.arange(lmax)[None, :] >= lens[:, None]] = -1
        lists[rng.rand(n_queries, lmax) < 0.03] = -1
    if labels == "graded":
        lab = rng.randint(0, 5, size=(n_queries, lmax)).astype(np.float32)
    else:  # above n_rel - 1, fractional, negative
        lab = rng.choice(np.array([0.0, 0.5, 0.99, 1.0, 1.7, 2.2, 3.9, 4.0, 6.5, 9.0, -1.0], np.float32), size=(n_queries, lmax))
    if never_frac > 0:
        lab[rng.rand(n_queries) < never_frac] = rng.choice(np.array([0.0, 1.0, 1.5], np.float32), size=lmax)
    lab = np.where(lists < 0, np.float32(3.0), lab).astype(np.float32)
    return lists, lab


def run_click(lists, labels, n_docs, exam, n_exam, cprob, model, seed, step, B, L, max_tries):
    from ultra_pytorch_amd import _lib, hip_ops
    dev = torch.device("cuda")
    dl, dy = torch.from_numpy(lists).to(dev), torch.from_numpy(labels).to(dev)
    cp = torch.tensor(np.asarray(cprob, np.float32), device=dev)
    ids = torch.full((L, B), -7, dtype=torch.int32, device=dev)  # sentinels: every element must be written
    ck = torch.full((L, B), -7.0, dtype=torch.float32, device=dev)
    q = torch.full((B,), -7, dtype=torch.int32, device=dev)
    rc = _lib.load().ultr_click_batch(dl.data_ptr(), dy.data_ptr(), lists.shape[0], lists.shape[1], n_docs, exam.data_ptr(), n_exam,
                                      cp.data_ptr(), len(cprob), model, seed, step, B, L, max_tries, ids.data_ptr(), ck.data_ptr(),
                                      q.data_ptr(), hip_ops.raw_stream())
    _lib.check(rc, "ultr_click_batch")
    torch.cuda.synchronize()
    return ids.cpu().numpy(), ck.cpu().numpy(), q.cpu().numpy()


def host_replay(hm, model, clicks, u, y):
    """The clicks the host model (float64, its own tables) makes from the kernel's uniforms.  Returns (number of draws within MARGIN
    of the threshold, mask of the slots free of such draws); asserts agreement on those slots."""
    L, B = u.shape
    cp_tab = np.asarray(hm.click_prob, np.float64)
    lab = np.where(y > 0, np.trunc(y), 0).astype(np.int64)
    cp = cp_tab[np.minimum(lab, len(cp_tab) - 1)]
    u = u.astype(np.float64)
    expect = np.zeros((L, B))
    close = np.zeros((L, B), bool)
    if model == R.UBM:
        last = np.full(B, -1, np.int64)
        for r in range(L):
            ex = np.zeros(B)
            for lc in np.unique(last):
                ex[last == lc] = hm.getExamProb(r, int(lc))
            p = ex * cp[r]
            close[r] = np.abs(u[r] - p) <= MARGIN
            expect[r] = u[r] < p
            last = np.where(expect[r] > 0, r, last)
    else:
        ex = np.array([hm.getExamProb(r) for r in range(L)])[:, None]
        p = ex * cp
        close = np.abs(u - p) <= MARGIN
        expect = (u < p).astype(np.float64)
        if model == R.CASCADE:
            first = np.where(expect.any(0), expect.argmax(0), L)
            expect = (np.arange(L)[:, None] == first[None, :]).astype(np.float64)
            close &= np.arange(L)[:, None] <= first[None, :]  # draws behind the first click decide nothing
    ok = ~close.any(0)
    np.testing.assert_array_equal(clicks[:, ok], expect[:, ok])
    return int(close.sum()), ok


CASES = {  # name: (click model json, L, B, lmax, n_queries, labels, seed, step, max_tries)
    "pbm_L1_B1_one_query": ("pbm", 1, 1, 1, 1, "graded", 0, 0, 100),
    "pbm_L10_B5_three_queries": ("pbm", 10, 5, 10, 3, "graded", 7, 1, 1),
    "pbm_L63_lmax40_wide_labels_100k_queries": ("pbm", 63, 4096, 40, 100000, "wide", HI_SEED, BIG_STEP, 3),
    "pbm_L64_B5": ("pbm", 64, 5, 64, 100, "wide", 3, 1, 100),
    "pbm3_L65_nexam3": ("pbm3", 65, 4096, 65, 100, "graded", 11, 0, 3),
    "pbm_L130_B4096": ("pbm", 130, 4096, 130, 3, "wide", HI_SEED, 1, 100),
    "cascade_L130_low_click_prob": ("cascade_low", 130, 4096, 130, 100, "graded", 5, BIG_STEP, 2),
    "cascade_L65_B5_lmax20": ("cascade", 65, 5, 20, 100, "wide", 9, 0, 100),
    "ubm_L130_json": ("ubm", 130, 4096, 130, 100, "graded", HI_SEED, BIG_STEP, 3),
    "ubm_L130_three_rows": ("ubm3", 130, 4096, 100, 1, "wide", 13, 1, 100),
    "ubm_L1_B5": ("ubm", 1, 5, 1, 3, "graded", 2, 0, 100),
    "ubm_L10_B1_lmax40": ("ubm", 10, 1, 40, 100000, "wide", 4, BIG_STEP, 100),
    "pbm_max_tries_exhausted": ("pbm_never", 64, 4096, 64, 100, "graded", 17, 1, 3),
    "ubm_max_tries_exhausted": ("ubm_never", 70, 4096, 70, 100, "graded", 19, BIG_STEP, 3),
}


def _model_desc(kind):
    return {"pbm": lambda: _desc("pbm_0.1_1.0_4_1.0.json"), "pbm3": _small_pbm, "cascade": lambda: _desc("cascade_0.1_1.0_4_1.0.json"),
            "cascade_low": _low_cascade, "ubm": lambda: _desc("ubm_0.1_1_4_1.0.json"), "ubm3": _three_row_ubm,
            "pbm_never": lambda: _never(_desc("pbm_0.1_1.0_4_1.0.json")),
            "ubm_never": lambda: _never(_desc("ubm_0.1_1_4_1.0.json"))}[kind]()


@pytest.mark.parametrize("name", list(CASES))
def test_click_batch_is_the_restatement_bit_for_bit(name):
    from ultra_pytorch_amd.utils import click_models
    kind, L, B, lmax, n_queries, labels, seed, step, max_tries = CASES[name]
    desc = _model_desc(kind)
    hm = click_models.loadModelFromJson(desc)
    model = {"position_biased_model": R.PBM, "cascade_model": R.CASCADE, "user_browsing_model": R.UBM}[desc["model_name"]]
    exam, n_exam = _exam_image(hm, model)
    n_docs = 5000
    lists, lab = make_data(list(CASES).index(name) + 1, n_queries, lmax, n_docs, ragged=lmax > 1, labels=labels,
                           never_frac=0.3 if kind.endswith("never") else 0.0)
    ids, ck, q = run_click(lists, lab, n_docs, exam, n_exam, desc["click_prob"], model, seed, step, B, L, max_tries)
    r_ids, r_ck, r_q, kept, u, y = R.click_draw(lists, lab, n_docs, exam.cpu().numpy(), n_exam, desc["click_prob"], model, seed, step,
                                                B, L, max_tries)
    np.testing.assert_array_equal(q, r_q)
    np.testing.assert_array_equal(ids, r_ids)
    np.testing.assert_array_equal(ck, r_ck)
    # second, independent check: the host model's own tables in float64
    n_close, ok = host_replay(hm, model, ck, u, y)
    print("%s: %d draws within %.1e of the threshold, %d of %d slots compared" % (name, n_close, MARGIN, ok.sum(), B))
    assert ok.sum() >= B - 2
    # the case exercises what it is named for
    got = ck.sum(0)
    if model == R.CASCADE:
        assert (got <= 1).all()
    if name == "cascade_L130_low_click_prob":
        first = ck.argmax(0)[got > 0]
        assert (first < 64).any() and ((first >= 64) & (first < 128)).any() and (first >= 128).any()
    if kind.endswith("never"):
        stuck = got == 0
        assert stuck.any() and (kept[stuck] == max_tries - 1).all() and (kept[~stuck] <= max_tries - 1).all()
    if lmax < L:
        assert (ids[lmax:] == n_docs).all()


def test_click_draw_riding_on_the_update_launch():
    """A plugin's train(feed) on a DeviceClickFeed draws the NEXT batch as extra workgroups of its update launch (update_tiled_kernel,
    blockIdx.x - rider_first): user-browsing clicks at L = 70 (two 64-position chunks), B = 61 (a partly empty last workgroup).  The
    batch handed out next must be the restatement's for (seed, step 1) - on the feed's own table image and click probabilities, and
    on the host model's tables."""
    from ultra_pytorch_amd.input_layer import DeviceClickFeed
    from ultra_pytorch_amd.utils import find_class
    F, L, B, seed = 16, 70, 61, HI_SEED
    ds = DS(120, (30, 70), F, seed=12)
    ds.pad(L)
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.IPWrank", "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=[32,16]",
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3]}
    algo = find_class(exp["learning_algorithm"])(ds, exp)
    feed = DeviceClickFeed(algo, B, "click_model_json=%s" % os.path.join(DATA, "ubm_0.1_1_4_1.0.json"), seed=seed)
    rd = feed.resident(ds)
    lists, lab = rd.lists.cpu().numpy(), rd.labels.cpu().numpy()
    exam, cprob = feed.exam.cpu().numpy(), feed.cprob.cpu().numpy()
    for step in range(3):
        f, info = feed.get_batch(ds, check_validation=True)
        ids, ck, q = f["docids"].cpu().numpy(), f["labels"].cpu().numpy(), info["rank_list_idxs"].cpu().numpy()
        r_ids, r_ck, r_q, _, u, y = R.click_draw(lists, lab, rd.n_docs, exam, feed.n_exam, cprob, R.UBM, seed, step, B, L, 100)
        np.testing.assert_array_equal(q, r_q, err_msg="step %d" % step)
        np.testing.assert_array_equal(ids, r_ids, err_msg="step %d" % step)
        np.testing.assert_array_equal(ck, r_ck, err_msg="step %d" % step)
        n_close, ok = host_replay(feed.click_model, R.UBM, ck, u, y)
        print("rider step %d: %d draws within %.1e of the threshold" % (step, n_close, MARGIN))
        assert ok.sum() >= B - 2
        loss, _, _ = algo.train(f)
        assert np.isfinite(loss)
        assert feed._pre == (id(ds), 100)  # the next batch was handed to the step (drawn ahead), not left for get_batch


REGEM_CASES = [(10, 0, 0), (70, HI_SEED, 1), (130, 7, BIG_STEP), (70, 0xFFFFFFFF00000001, 0)]


@pytest.mark.parametrize("L,seed,step", REGEM_CASES)
def test_regression_em_pseudo_labels_are_the_restatement(L, seed, step):
    """regem_kernel without injected uniforms: y = ceil(p_r1 - u) with u from Philox(b, l, 0x5245454D, 1) under the (seed, step) key,
    p_r1 = c + (1 - c)(1 - pr) gamma / (1 - pr gamma) - exact wherever p_r1 is not within 1e-6 of u; clicked positions give y = 1;
    dscores = gamma - y."""
    from ultra_pytorch_amd import hip_ops
    B = 1000
    rng = np.random.RandomState(L)
    s = rng.normal(scale=2.0, size=(B, L)).astype(np.float32)
    c = (rng.uniform(size=(L, B)) < 0.15).astype(np.float32)
    pr = (0.95 * 0.9 ** np.arange(L) + 0.02).astype(np.float32)  # propensities that vary by position
    dev = torch.device("cuda")
    ds = torch.full((B, L), np.nan, device=dev)
    y = torch.full((B, L), -7.0, device=dev)
    ws = torch.zeros(hip_ops.loss_workspace_bytes(B, L) // 4, device=dev)
    hip_ops.regem_loss(torch.from_numpy(s).to(dev), torch.from_numpy(c).to(dev), torch.from_numpy(pr).to(dev), B, L, ds, ws,
                       uniforms=None, seed=seed, step=step, pseudo_out=y)
    torch.cuda.synchronize()
    y, ds = y.cpu().numpy(), ds.cpu().numpy()
    u = R.regem_uniforms(seed, step, B, L).astype(np.float64)
    g = 1.0 / (1.0 + np.exp(-s.astype(np.float64)))
    c64, p64 = c.T.astype(np.float64), pr.astype(np.float64)[None, :]
    p_r1 = c64 + (1 - c64) * (1 - p64) * g / (1 - p64 * g)
    expect = np.ceil(p_r1 - u) + 0.0  # (+ 0.0: -0.0 counts as 0)
    far = np.abs(p_r1 - u) > 1e-6
    print("regem L=%d: %d of %d elements within 1e-6 of the threshold" % (L, (~far).sum(), far.size))
    assert set(np.unique(y)) <= {0.0, 1.0}
    np.testing.assert_array_equal(y[far] + 0.0, expect[far])
    assert (y[c.T > 0] == 1.0).all() and (c > 0).any()
    assert 0.05 < y[c.T == 0].mean() < 0.95
    np.testing.assert_allclose(ds, g - y, rtol=0, atol=1e-6)
