"""PDGD and the online simulation feeds on the host: the float64 restatement (tests/pdgd_ref.py) against the reference's recorded
steps and against the reference's brute-force formula, both online feeds against the reference's batches, and the C-ABI
constants.  CPU only."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import pdgd_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(GOLDEN, "ultra_toy_data") + "/"
STEP_FIXTURES = ["pdgd_tiny", "pdgd_sgd_tau2", "pdgd_linear", "pdgd_cutoff"]


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return d, json.loads(str(d["meta"]))


@pytest.mark.parametrize("name", STEP_FIXTURES)
def test_restatement_matches_reference_pairs_and_loss(name):
    d, m = load(name)
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        ids, lab, sc = d[p + "docids"], d[p + "labels"], d[p + "scores"]
        n_docs = d[p + "features"].shape[0]
        pairs = R.batch_pairs(sc, lab, ids, n_docs, m["cutoff"], m["tau"])
        assert len(pairs) == d[p + "pair_weights"].size > 0
        np.testing.assert_array_equal([ids[l, b] for (b, l, k, w) in pairs], d[p + "pair_pos"])
        np.testing.assert_array_equal([ids[k, b] for (b, l, k, w) in pairs], d[p + "pair_neg"])
        np.testing.assert_allclose([w for (*_, w) in pairs], d[p + "pair_weights"], rtol=2e-5, atol=1e-9)
        step = R.pdgd_step(d[p + "pre_params"], d[p + "pre_adagrad"], m["F"], m["hidden"], d[p + "features"], ids, lab, m["cutoff"],
                           m["tau"], m["lr"], m["max_gradient_norm"], m["l2_loss"], m["grad_strategy"])
        np.testing.assert_allclose(step["scores"], sc, rtol=1e-5, atol=1e-6)
        assert abs(step["loss"] - float(d[p + "loss"])) <= 1e-5 * max(1.0, abs(float(d[p + "loss"])))
        np.testing.assert_allclose(step["grads"], d[p + "grads"], rtol=1e-4, atol=1e-6)
        gref = d[p + "grads"]  # Adagrad's first step moves by +-lr whatever |g|: the sign of a vanishing gradient is noise
        sel = np.abs(gref) > 1e-6 * max(1.0, float(np.abs(gref).max()))
        np.testing.assert_allclose(step["params"][sel], d[p + "post_params"][sel], rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(step["state"], d[p + "post_adagrad"], rtol=1e-4, atol=1e-8)


def test_fixtures_cover_the_cases():
    """PADs inside and past the cutoff, graded labels, a clipped weight (delta > 20 would need a larger gap: see the random test),
    tau 2, sgd, l2_loss 0 and 0.005, Linear."""
    d, m = load("pdgd_cutoff")
    assert m["cutoff"] < m["M"]
    seen_in = seen_past = graded = False
    for t in range(m["n_steps"]):
        ids, lab = d["s%d_docids" % t], d["s%d_labels" % t]
        pad = ids == d["s%d_features" % t].shape[0]
        seen_in |= bool(pad[:m["cutoff"]].any())
        seen_past |= bool(pad[m["cutoff"]:].any())
        graded |= bool((lab > 1).any())
    assert seen_in and seen_past and graded
    ms = [load(n)[1] for n in STEP_FIXTURES]
    assert {x["tau"] for x in ms} == {1.0, 2.0} and {x["l2_loss"] for x in ms} == {0.0, 0.005}
    assert {x["grad_strategy"] for x in ms} == {"ada", "sgd"} and {x["model"] for x in ms} == {"DNN", "Linear"}


def random_list(rng, M):
    s = rng.standard_normal(M).astype(np.float32) * rng.choice([0.5, 3.0, 15.0])
    s[rng.uniform(size=M) < 0.25] = np.float32(0.25)  # ties
    y = rng.randint(0, 4, size=M).astype(np.float64) * (rng.uniform(size=M) < 0.6)
    valid = rng.uniform(size=M) > 0.15
    return s, y, valid


@pytest.mark.parametrize("M", [1, 2, 3, 7, 10, 33, 64, 65])
def test_local_delta_equals_bruteforce(M):
    rng = np.random.RandomState(M)
    n = 0
    for trial in range(12):
        s, y, valid = random_list(rng, M)
        cutoff = int(rng.randint(1, M + 1))
        tau = int(rng.randint(1, 4))
        a = R.list_pairs(s, y, valid, cutoff, tau)
        b = R.list_pairs(s, y, valid, cutoff, tau, brute=True)
        assert [(l, k) for l, k, _ in a] == [(l, k) for l, k, _ in b]
        np.testing.assert_allclose([w for *_, w in a], [w for *_, w in b], rtol=1e-9, atol=1e-12)
        n += len(a)
    assert M < 3 or n > 0


def test_pad_past_cutoff_keeps_its_exp_score_and_clip_at_20():
    s = np.array([0.0, -1.0, 5.0, 2.0], dtype=np.float32)
    valid = np.array([True, True, False, False])
    e = R.exp_scores(s, valid, 3, 1)
    assert e[2] == 0.0 and e[3] > 0.0  # the PAD at 3 >= cutoff keeps exp(2 - 5)
    # a huge gap: delta > 20, the weight stops at 1 / (1 + e^20)
    s = np.array([0.0, -40.0], dtype=np.float32)
    (l, k, w), = R.list_pairs(s, np.array([0.0, 1.0]), np.array([True, True]), 2, 1)
    assert (l, k) == (1, 0) and w == pytest.approx(1.0 / (1.0 + np.exp(20.0)), rel=1e-12)


class StubModel:
    """validation() replays the scores the reference's stub returned (tests/golden/make_golden_pdgd.py)."""

    def __init__(self, feature_size, rank_list_size, max_candidate_num, scores):
        self.feature_size, self.rank_list_size, self.max_candidate_num = feature_size, rank_list_size, max_candidate_num
        self.letor_features_name = "letor_features"
        self.docid_inputs_name = ["docid_input%d" % i for i in range(max_candidate_num)]
        self.labels_name = ["label%d" % i for i in range(max_candidate_num)]
        self.hparams = type("H", (), {})()
        self.scores = list(scores)

    def validation(self, input_feed, is_online_simulation=False):
        s = self.scores.pop(0)
        assert s.shape[0] == len(input_feed[self.docid_inputs_name[0]])
        return None, torch.from_numpy(s), {}


def feed_arrays(model, feed, M):
    ids = np.stack([feed[model.docid_inputs_name[l]] for l in range(M)]).astype(np.int32)
    lab = np.stack([feed[model.labels_name[l]] for l in range(M)]).astype(np.float32)
    return ids, lab


def test_online_feeds_reproduce_reference_batches():
    from ultra_pytorch_amd import input_layer, utils
    d, m = load("pdgd_feeds")
    ds = utils.read_data(DATA, "train")
    M, cutoff = m["M"], m["cutoff"]
    ds.pad(M)
    seed = m["seed"]
    redraw_seen = False
    for ci, (key, cls, hparams, check, n_batches, B) in enumerate(m["cases"]):
        scores = [d["%s_b%d_scores" % (key, t)] for t in range(n_batches)]
        det = cls.startswith("Deterministic")
        if det:
            scores += [d[key + "_next_scores"], d[key + "_byidx_scores"]]
        model = StubModel(ds.feature_size, cutoff, M, scores)
        random.seed(seed + ci)
        np.random.seed(seed + ci)
        feed = getattr(input_layer, cls)(model, B, hparams.replace("./example/ClickModel/", ""))
        for t in range(n_batches):
            f, info = feed.get_batch(ds, check_validation=check)
            p = "%s_b%d_" % (key, t)
            ids, lab = feed_arrays(model, f, M)
            np.testing.assert_array_equal(info["rank_list_idxs"], d[p + "idxs"], err_msg=p)
            assert len(f["letor_features"]) == int(d[p + "n_features"])
            np.testing.assert_array_equal(ids, d[p + "docids"], err_msg=p)
            np.testing.assert_array_equal(lab, d[p + "labels"], err_msg=p)
            assert (lab[cutoff:] == 0).all()
            redraw_seen |= check and (lab[:cutoff].sum(axis=0) > 0).all()
        assert getattr(feed.click_model, "eta", 0.0) == pytest.approx(float(d[key + "_eta"]))
        if det:
            f, _ = feed.get_next_batch(3, ds, check_validation=False)
            np.testing.assert_array_equal(feed_arrays(model, f, M), (d[key + "_next_docids"], d[key + "_next_labels"]))
            f, _ = feed.get_data_by_index(ds, 7, check_validation=False)
            np.testing.assert_array_equal(feed_arrays(model, f, M), (d[key + "_byidx_docids"], d[key + "_byidx_labels"]))
    assert redraw_seen


def test_stochastic_feed_next_batch_and_by_index_work():
    """The reference's stochastic feed crashes in both (self.model.letor_features.name); here they build re-ranked batches."""
    from ultra_pytorch_amd import input_layer, utils
    ds = utils.read_data(DATA, "train")
    M = ds.rank_list_size
    ds.pad(M)
    rng = np.random.RandomState(0)
    model = StubModel(ds.feature_size, 5, M, [rng.standard_normal((n, M)).astype(np.float32) for n in (4, 1)])
    np.random.seed(0)
    random.seed(0)
    feed = input_layer.StochasticOnlineSimulationFeed(model, 4, "oracle_mode=True")
    f, _ = feed.get_next_batch(2, ds)
    ids, lab = feed_arrays(model, f, M)
    assert ids.shape == (M, 4) and (lab[5:] == 0).all()
    f, _ = feed.get_data_by_index(ds, 3)
    ids, _ = feed_arrays(model, f, M)
    n = len(f["letor_features"])
    col = ids[:, 0]
    assert sorted(col[col < n].tolist()) == list(range(n))


def test_interleaving_refused():
    from ultra_pytorch_amd import input_layer
    model = StubModel(4, 2, 3, [])
    model.hparams.need_interleave = True
    with pytest.raises(NotImplementedError):
        input_layer.DeterministicOnlineSimulationFeed(model, 2, "")


def test_abi_constants():
    from ultra_pytorch_amd import _lib, engine
    hdr = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    assert int(re.search(r"ULTR_ALGO_PDGD\s*=\s*(\d+)", hdr).group(1)) == _lib.ALGO_PDGD == 6
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8
    assert re.search(r"\bint ultr_pdgd_loss\(", hdr) and "ultr_pdgd_loss" in _lib.SIGNATURES
    assert engine.ALGOS["pdgd"] == 6


def test_plugin_is_exported():
    from ultra_pytorch_amd import input_layer, learning_algorithm
    from ultra_pytorch_amd.utils import find_class
    assert find_class("ultra_pytorch_amd.learning_algorithm.PDGD") is learning_algorithm.PDGD
    assert learning_algorithm.PDGD.DEFAULT_HPARAMS == dict(learning_rate=0.05, tau=1, max_gradient_norm=1.0, l2_loss=0.005,
                                                           grad_strategy="ada")
    assert find_class("ultra_pytorch_amd.input_layer.StochasticOnlineSimulationFeed") is input_layer.StochasticOnlineSimulationFeed
