"""DBGD / MGD on the host: the restatement of the kernels (tests/dbgd_ref.py) against the reference's recorded steps
(tests/golden/dbgd_*.npz, make_golden_dbgd.py) from the recorded noise, shuffles and clicks; the plugin's defaults and exports; the
C-ABI entries; the online feeds' acceptance of the interleaving algorithms.  CPU only."""
import json
import os
import re

import numpy as np
import pytest

from tests import dbgd_ref as R
from tests import ndcg_ref as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_FIXTURES = ["dbgd_det", "dbgd_sto", "dbgd_noint", "dbgd_ada", "dbgd_linear"]


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return d, json.loads(str(d["meta"]))


def ndcg_mean(scores_BL, labels_LB, topn):
    return float(np.mean(N.ndcg_per_list(np.asarray(scores_BL, np.float32), np.asarray(labels_LB, np.float32).T, [topn])[0]))


@pytest.mark.parametrize("name", STEP_FIXTURES)
def test_restatement_reproduces_the_recorded_steps(name):
    d, m = load(name)
    M, cut, F, hidden = m["M"], m["cutoff"], m["F"], m["hidden"] or []
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        ids, lab, n_docs = d[p + "docids"], d[p + "labels"], d[p + "features"].shape[0]
        # the noise law: F.normalize of the recorded normals, sign(z) on the scorer row
        u = R.normalize(d[p + "noise"].astype(np.float64), F, hidden)
        lay, P = R.layout(F, hidden)
        assert u.shape == (1, P) == d[p + "pre_params"][None].shape
        ow, m_last, k_last = lay[-1][2], lay[-1][3], lay[-1][1]
        assert m_last == 1 and set(np.unique(u[0, ow:ow + k_last])) <= {-1.0, 1.0}
        # the loss: 1 - NDCG@cutoff of the current model, PADs unmasked
        sc = d[p + "scores"]
        assert abs((1.0 - ndcg_mean(sc[:, :cut], lab[:cut], cut)) - float(d[p + "loss"])) < 1e-6
        if m["need_interleave"]:
            NR = 2
            W = np.zeros((ids.shape[1], NR))
            for b in range(ids.shape[1]):
                n = R.list_len(ids[:, b], n_docs)
                rk = d[p + "rankings"][b, :, :n]
                if m["interleave_strategy"] != "Stochastic":  # the stable descending sort of each ranker's scores
                    assert np.array_equal(R.ranking(sc[b], n, R.DETERMINISTIC), rk[0])
                    assert np.array_equal(R.ranking(d[p + "cand_scores"][b], n, R.DETERMINISTIC), rk[1])
                sh = d[p + "shuffles"][b]
                ml, tm = R.team_draft(rk, lambda r_, asg: list(sh[r_]))
                assert np.array_equal(ml, d[p + "interleaved"][:n, b]) and np.array_equal(tm, d[p + "teams"][:n, b])
                c = min(n, cut)
                W[b] = R.winners(tm[:c], d[p + "clicks"][:c, b], NR)
            np.testing.assert_allclose(W, d[p + "winners"], rtol=1e-6, atol=1e-7)
            c = R.ranker_weights(W)
        else:
            nd = [ndcg_mean(sc[:, :cut], lab[:cut], cut), ndcg_mean(d[p + "cand_scores"], lab[:cut], cut)]
            c = R.ranker_weights(ndcg=nd)
        # the reference's parameter.grad is the negative of the direction the update applies here
        np.testing.assert_allclose(R.gradient(u, c), -d[p + "grads"].astype(np.float64), atol=1e-6)
        assert abs(float(np.sqrt((d[p + "grads"].astype(np.float64) ** 2).sum())) - float(d[p + "norm"])) < 1e-5


def test_fixtures_cover_the_cases():
    seen = {"pad_inside": False, "pad_tail": False, "prefix": False, "no_click_team": False}
    for name in STEP_FIXTURES:
        d, m = load(name)
        for t in range(m["n_steps"]):
            ids, n_docs = d["s%d_docids" % t], d["s%d_features" % t].shape[0]
            for b in range(ids.shape[1]):
                n = R.list_len(ids[:, b], n_docs)
                seen["pad_inside"] |= bool((ids[:n, b] == n_docs).any())
                seen["pad_tail"] |= n < ids.shape[0]
            if m["need_interleave"]:
                seen["prefix"] |= bool((d["s%d_teams" % t] == -1).any())
                seen["no_click_team"] |= bool((d["s%d_winners" % t].sum(1) == 0).any())
    assert all(seen.values()), seen
    ms = [load(n)[1] for n in STEP_FIXTURES]
    assert {x["grad_strategy"] for x in ms} == {"sgd", "ada"} and {x["model"] for x in ms} == {"DNN", "Linear"}
    assert {x["interleave_strategy"] for x in ms if x["need_interleave"]} == {"Stochastic", "Deterministic"}
    assert any(not x["need_interleave"] for x in ms) and any(x["cutoff"] < x["M"] for x in ms)


def test_post_step_is_the_reference_arithmetic():
    """The recorded update is theta - lr * clip(g) (SGD) / Adagrad on clip(g): what the mirrored GPU step is checked against."""
    for name in STEP_FIXTURES:
        d, m = load(name)
        for t in range(m["n_steps"]):
            p = "s%d_" % t
            g = d[p + "grads"].astype(np.float64) * float(d[p + "clip_coef"])
            th = d[p + "pre_params"].astype(np.float64)
            if m["grad_strategy"] == "sgd":
                ref = th - m["lr"] * g
            else:
                s = d[p + "pre_adagrad"].astype(np.float64) + g * g
                ref = th - m["lr"] * g / (np.sqrt(s) + 1e-10)
                np.testing.assert_allclose(s, d[p + "post_adagrad"], rtol=1e-5, atol=1e-9)
            np.testing.assert_allclose(ref, d[p + "post_params"], atol=2e-6)


def test_mgd_multileave_and_gradient():
    d, m = load("dbgd_mgd")
    NR = m["NR"]
    prefixes = 0
    for i in range(m["n_lists"]):
        rk, sh = d["l%d_rankings" % i], d["l%d_shuffles" % i]
        ml, tm = R.team_draft(rk, lambda r_, asg: list(sh[r_]))
        assert np.array_equal(ml, d["l%d_multileaved" % i]) and np.array_equal(tm, d["l%d_teams" % i])
        np.testing.assert_allclose(R.winners(tm, d["l%d_clicks" % i], NR), d["l%d_winners" % i], rtol=1e-6, atol=1e-7)
        prefixes += int((tm == -1).sum() > 1)
    assert prefixes > 0
    g = R.gradient(d["mgd_noise"], R.ranker_weights(d["mgd_winners"]))
    np.testing.assert_allclose(g, -d["mgd_grads"].astype(np.float64), atol=1e-6)


def test_shuffle_is_a_permutation_and_team_draft_rounds():
    for b in range(20):
        sh = R.philox_shuffle(7, 3, b)
        asg = list(range(6))
        for t in range(5):
            asg = sh(t, asg)
            assert sorted(asg) == list(range(6))
    rk = np.array([[0, 1, 2, 3, 4], [0, 1, 4, 3, 2], [0, 2, 1, 3, 4]])
    ml, tm = R.team_draft(rk, lambda t, asg: asg)
    assert ml[0] == 0 and tm[0] == -1 and sorted(ml.tolist()) == list(range(5)) and list(tm[1:4]) == [0, 1, 2]


def test_hparam_defaults_and_export():
    from ultra_pytorch_amd import learning_algorithm
    from ultra_pytorch_amd.utils import find_class
    assert find_class("ultra_pytorch_amd.learning_algorithm.DBGD") is learning_algorithm.DBGD
    assert find_class("ultra_pytorch_amd.learning_algorithm.MGD") is learning_algorithm.MGD
    ref = dict(click_model_json="./example/ClickModel/pbm_0.1_1.0_4_1.0.json", learning_rate=0.5, max_gradient_norm=5.0,
               need_interleave=True, interleave_strategy="Stochastic", grad_strategy="sgd")
    assert learning_algorithm.DBGD.DEFAULT_HPARAMS == dict(ref, tau=1)
    assert learning_algorithm.MGD.DEFAULT_HPARAMS == dict(ref, tau=1, ranker_num=4)
    assert learning_algorithm.DBGD.INTERLEAVES_IN_TRAIN and issubclass(learning_algorithm.MGD, learning_algorithm.DBGD)


def test_abi_entries():
    from ultra_pytorch_amd import _lib, engine
    hdr = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION
    assert int(re.search(r"ULTR_ALGO_DBGD\s*=\s*(\d+)", hdr).group(1)) == _lib.ALGO_DBGD == engine.ALGOS["dbgd"] == 7
    for fn in ("ultr_dbgd_noise_args", "ultr_dbgd_interleave_args", "ultr_dbgd_grad_args"):
        assert re.search(r"\bint %s\(const ultr_dbgd_args\* a, void\* stream\);" % fn, hdr) and fn in _lib.SIGNATURES
    assert int(re.search(r"#define\s+ULTR_DBGD_MAX_M\s+(\d+)", hdr).group(1)) == _lib.DBGD_MAX_M == 256
    assert int(re.search(r"#define\s+ULTR_DBGD_MAX_RANKERS\s+(\d+)", hdr).group(1)) == _lib.DBGD_MAX_RANKERS == 16
    body = hdr[hdr.index("typedef struct ultr_dbgd_args"):hdr.index("} ultr_dbgd_args;")]
    fields = re.findall(r"\b(\w+)(?:,|;)", body.split("{", 1)[1])
    assert fields == [f for f, _ in _lib.DbgdArgs._fields_]


class StubModel:
    def __init__(self, interleaves):
        self.feature_size, self.rank_list_size, self.max_candidate_num = 4, 2, 3
        self.letor_features_name = "letor_features"
        self.docid_inputs_name = ["docid_input%d" % i for i in range(3)]
        self.labels_name = ["label%d" % i for i in range(3)]
        self.hparams = type("H", (), {"need_interleave": True})()
        if interleaves:
            self.INTERLEAVES_IN_TRAIN = True


def test_host_feeds_accept_dbgd_and_refuse_other_interleaving_models():
    from ultra_pytorch_amd import input_layer, learning_algorithm
    for cls in (input_layer.StochasticOnlineSimulationFeed, input_layer.DeterministicOnlineSimulationFeed):
        feed = cls(StubModel(True), 2, "")
        assert feed.need_interleave
        with pytest.raises(NotImplementedError, match="interleaving"):
            cls(StubModel(False), 2, "")
    for algo in (learning_algorithm.DBGD, learning_algorithm.MGD):
        assert getattr(algo, "INTERLEAVES_IN_TRAIN", False)
