"""The trust-bias click model and AffineRank without a GPU: the host model (JSON, the shipped file, its refusals, one draw of Python's
random stream per position), how it reaches the device (id 3, the [2, n] image), the closed-form unbiasedness of the affine
correction, OraclePropensityEstimator.affine_table, AffineRank's hyper-parameters and table files, and the host-only answers of the
C entries (ULTR_E_BADARG, the list bound, ultr_opt_state_floats)."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest

from tests import trust_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "ultra_pytorch_amd", "data")
SHIPPED = os.path.join(DATA, "trust_0.1_1.0_4_1.0.json")


def CM():
    from ultra_pytorch_amd.utils import click_models
    return click_models


def test_json_round_trip_and_the_shipped_file():
    cm = CM()
    m = cm.TrustBiasModel(0.1, 1.0, 4, 1.0)
    desc = m.getModelJson()
    assert desc["model_name"] == "trust_bias_model" and set(desc) == {"model_name", "eta", "click_prob", "exam_prob", "trust_pos", "trust_neg"}
    assert desc["exam_prob"] == cm.PositionBiasedModel(0.1, 1.0, 4, 1.0).exam_prob
    assert desc["trust_pos"] == [1 - (r + 1) / 100 for r in range(10)] and desc["trust_neg"] == [0.65 / (r + 1) for r in range(10)]
    with open(SHIPPED) as f:
        assert json.load(f) == desc
    back = cm.loadModelFromJson(json.loads(json.dumps(desc)))
    assert type(back) is cm.TrustBiasModel and back.getModelJson() == desc
    # an unknown name keeps falling to the position-biased model
    other = dict(desc, model_name="some_other_model")
    assert type(cm.loadModelFromJson(other)) is cm.PositionBiasedModel
    # eta moves the examination table, alpha and beta follow it
    m.setExamProb(2.0)
    a, b = m.affine_parameters(10)
    assert a[3] == 0.34 ** 2.0 * (m.trust_pos[3] - m.trust_neg[3]) and b[3] == 0.34 ** 2.0 * m.trust_neg[3]


def test_load_for_device_and_the_image(tmp_path):
    cm = CM()
    desc, model, mid = cm.load_for_device(SHIPPED, "test")
    assert mid == 3 == cm.CLICK_MODEL_IDS["trust_bias_model"] and type(model) is cm.TrustBiasModel
    # a path that does not exist falls back to the package's data/
    assert cm.load_for_device("./nowhere/trust_0.1_1.0_4_1.0.json", "test")[2] == 3
    bad = tmp_path / "dcm.json"
    bad.write_text(json.dumps(dict(desc, model_name="dependent_click_model")))
    with pytest.raises(NotImplementedError, match="position-biased, the cascade and the user-browsing model"):
        cm.load_for_device(str(bad), "X")
    exam, n, cprob = cm.device_tables(model, mid, "cpu")
    assert n == 10 and tuple(exam.shape) == (2, 10) and exam.dtype.is_floating_point and exam.element_size() == 4
    for k in range(10):
        assert float(exam[0, k]) == float(np.float32(model.exam_prob[k] * (model.trust_pos[k] - model.trust_neg[k])))
        assert float(exam[1, k]) == float(np.float32(model.exam_prob[k] * model.trust_neg[k]))
    assert np.array_equal(exam.numpy().reshape(-1), T.image_of(model)[0])
    assert cprob.tolist() == [float(np.float32(x)) for x in model.click_prob]
    # ids 0 / 1 / 2 keep their images
    pbm = cm.PositionBiasedModel(0.1, 1.0, 4, 1.0)
    assert tuple(cm.device_tables(pbm, 0, "cpu")[0].shape) == (10,)


@pytest.mark.parametrize("kw", [dict(trust_pos=[0.9] * 9), dict(trust_neg=[0.1] * 11), dict(trust_neg=[-0.1] + [0.1] * 9),
                                dict(trust_pos=[1.1] + [0.9] * 9), dict(trust_pos=[0.5] * 10, trust_neg=[0.5] * 10),
                                dict(trust_pos=[0.2] * 10, trust_neg=[0.3] * 10)])
def test_bad_tables_raise(kw):
    cm = CM()
    with pytest.raises(ValueError, match="trust_bias_model"):
        cm.TrustBiasModel(0.1, 1.0, 4, 1.0, **kw)
    desc = cm.TrustBiasModel(0.1, 1.0, 4, 1.0).getModelJson()
    desc.update(kw)
    with pytest.raises(ValueError, match="trust_bias_model"):
        cm.loadModelFromJson(desc)


def test_one_draw_per_position_and_the_law():
    cm = CM()
    trust, pbm = cm.TrustBiasModel(0.1, 1.0, 4, 1.0), cm.PositionBiasedModel(0.1, 1.0, 4, 1.0)
    labels = [0, 4, 2, 7, 0.5, -1, 3, 1, 0, 2, 4, 0, 1]  # beyond the tables' ten rows, beyond the grades, fractional, negative
    random.seed(11)
    clicks, exams, cps = trust.sampleClicksForOneList(labels)
    after_trust = random.getstate()
    random.seed(11)
    pbm.sampleClicksForOneList(labels)
    assert random.getstate() == after_trust
    random.seed(11)
    us = [random.random() for _ in labels]
    for r, (y, u) in enumerate(zip(labels, us)):
        k = min(r, 9)
        gamma = trust.click_prob[min(max(int(y), 0) if y > 0 else 0, 4)]
        assert exams[r] == trust.exam_prob[k] and cps[r] == trust.trust_neg[k] + (trust.trust_pos[k] - trust.trust_neg[k]) * gamma
        assert clicks[r] == (1 if u < exams[r] * cps[r] else 0)
    random.seed(5)
    one = trust.sampleClick(12, 3)
    assert one[1] == trust.exam_prob[9] and len(one) == 3
    # the examination-only weights are the base class's, the affine ones are new
    c = [1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0]
    assert trust.estimatePropensityWeightsForOneList(c) == pbm.estimatePropensityWeightsForOneList(c)
    a, b = trust.affine_parameters(len(c))
    assert trust.estimateAffineWeightsForOneList(c) == [(ci - bi) / ai for ci, ai, bi in zip(c, a, b)]
    assert a[11] == a[9] and b[10] == b[9] and all(isinstance(x, float) for x in a + b)


def test_the_affine_correction_is_unbiased_in_closed_form():
    with open(SHIPPED) as f:
        m = CM().loadModelFromJson(json.load(f))
    alpha, beta = m.affine_parameters(12)
    for k in range(12):
        kk = min(k, 9)
        for gamma in m.click_prob:
            p = m.exam_prob[kk] * (m.trust_neg[kk] + (m.trust_pos[kk] - m.trust_neg[kk]) * gamma)
            assert abs(p * (1 - beta[k]) / alpha[k] + (1 - p) * (-beta[k]) / alpha[k] - gamma) <= 1e-12
    # ... and the examination-only weight is not: at rank 0 a document of the lowest grade is estimated at 0.684, not at 0.1
    p = m.exam_prob[0] * (m.trust_neg[0] + (m.trust_pos[0] - m.trust_neg[0]) * m.click_prob[0])
    assert abs(p / m.exam_prob[0] - 0.684) <= 1e-12 and m.click_prob[0] == 0.1


def test_affine_table_of_the_oracle_estimator():
    cm = CM()
    from ultra_pytorch_amd.utils.propensity_estimator import OraclePropensityEstimator
    trust = cm.TrustBiasModel(0.1, 1.0, 4, 1.0)
    est = OraclePropensityEstimator(trust)
    a, b = est.affine_table(12)
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (12,)
    ra, rb = trust.affine_parameters(12)
    assert np.array_equal(a, np.asarray(ra, np.float32)) and np.array_equal(b, np.asarray(rb, np.float32))
    kind, w = est.weight_table(12)  # the examination-only weights: PBM's expression
    pbm = cm.PositionBiasedModel(0.1, 1.0, 4, 1.0)
    kind_p, w_p = OraclePropensityEstimator(pbm).weight_table(12)
    assert kind == kind_p == "position" and np.array_equal(w, w_p)
    a, b = OraclePropensityEstimator(pbm).affine_table(12)
    assert np.array_equal(a, np.asarray([pbm.getExamProb(r) for r in range(12)], np.float32)) and not b.any()
    for other in (cm.CascadeModel(0.1, 1.0, 4, 1.0), cm.UserBrowsingModel(0.1, 1.0, 4, 1.0)):
        with pytest.raises(NotImplementedError, match="depends on the clicks"):
            OraclePropensityEstimator(other).affine_table(10)
    with pytest.raises(ValueError):
        est.affine_table(0)


def test_affine_rank_hyper_parameters_and_tables(tmp_path):
    from ultra_pytorch_amd.learning_algorithm import AffineRank
    from ultra_pytorch_amd.learning_algorithm.affine_rank import load_affine_table
    hp = AffineRank.parse_hparams("")
    assert (hp.learning_rate, hp.max_gradient_norm, hp.l2_loss, hp.grad_strategy) == (0.05, 5.0, 0.0, "ada")
    assert hp.affine_clip == 0.0 and hp.mask_padding is True and hp.affine_estimator_json.endswith("trust_0.1_1.0_4_1.0.json")
    hp = AffineRank.parse_hparams("affine_clip=0.1,mask_padding=false,grad_strategy=adam,affine_estimator_json=/x/y.json")
    assert hp.affine_clip == 0.1 and hp.mask_padding is False and hp.grad_strategy == "adam" and hp.affine_estimator_json == "/x/y.json"
    with pytest.raises(ValueError, match="affine_clip"):
        AffineRank.parse_hparams("affine_clip=-1.0")
    assert AffineRank.ENGINE_ALGO == "affine"
    # a click-model description (the default path falls back to the package's data/), and a file with a "click_model" entry
    trust = T.shipped_model()
    ra, rb = (np.asarray(x, np.float32) for x in trust.affine_parameters(12))
    a, b = load_affine_table(AffineRank.parse_hparams("").affine_estimator_json, 12)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
    wrapped = tmp_path / "oracle.json"
    wrapped.write_text(json.dumps({"click_model": trust.getModelJson(), "IPW_list": [1.0]}))
    a, b = load_affine_table(str(wrapped), 5)
    assert np.array_equal(a, ra[:5]) and np.array_equal(b, rb[:5])
    # a table, its clip, and what write_affine_table writes
    table = tmp_path / "table.json"
    table.write_text(json.dumps({"alpha": [0.5, 0.25, 0.01], "beta": [0.25, 0.1, 0.0]}))
    a, b = load_affine_table(str(table), 10)
    assert a.tolist() == [0.5, 0.25, float(np.float32(0.01))] and b.tolist() == [0.25, float(np.float32(0.1)), 0.0]
    a, b2 = load_affine_table(str(table), 10, affine_clip=0.3)
    assert a.tolist() == [0.5, float(np.float32(0.3)), float(np.float32(0.3))] and np.array_equal(b2, b)
    algo = AffineRank.__new__(AffineRank)  # the table file needs the two arrays only, no GPU
    algo.alpha, algo.beta = a, b2
    out = tmp_path / "written.json"
    algo.write_affine_table(str(out))
    assert set(json.load(open(out))) == {"alpha", "beta"}
    a3, b3 = load_affine_table(str(out), 10)
    assert np.array_equal(a3, a) and np.array_equal(b3, b2)
    for bad in ({"alpha": [0.5, 0.0], "beta": [0.1, 0.1]}, {"alpha": [0.5, -0.1], "beta": [0.1, 0.1]}, {"alpha": [0.5], "beta": [0.1, 0.1]},
                {"alpha": [], "beta": []}):
        table.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            load_affine_table(str(table), 10)
    table.write_text(json.dumps({"IPW_list": [1.0]}))
    with pytest.raises(KeyError):
        load_affine_table(str(table), 10)
    table.write_text(json.dumps(CM().CascadeModel(0.1, 1.0, 4, 1.0).getModelJson()))
    with pytest.raises(NotImplementedError):
        load_affine_table(str(table), 10)


def test_entries_are_exported_bound_and_declared():
    from ultra_pytorch_amd import _lib, engine
    lib = _lib.load()
    assert int(lib.ultr_abi_version()) == _lib.ABI_VERSION == 8
    assert hasattr(lib, "ultr_affine_loss") and engine.ALGOS["affine"] == _lib.ALGO_AFFINE == 12
    hdr = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    m = re.search(r"\bint ultr_affine_loss\(([^)]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == 12 == len(_lib.SIGNATURES["ultr_affine_loss"][1])
    assert re.search(r"ULTR_ALGO_AFFINE = %d\b" % _lib.ALGO_AFFINE, hdr) and re.search(r"#define ULTR_CLICK_TRUST 3\b", hdr)
    one = ctypes.c_void_p(16)  # (never dereferenced: every call below is refused before a launch)

    def call(scores=one, labels=one, alpha=one, beta=one, n_aff=10, docids=None, n_docs=0, B=3, L=5, ds=one, ws=one):
        return lib.ultr_affine_loss(scores, labels, alpha, beta, n_aff, docids, n_docs, B, L, ds, ws, None)

    for bad in (dict(scores=None), dict(labels=None), dict(alpha=None), dict(beta=None), dict(ds=None), dict(ws=None), dict(B=0), dict(B=-1),
                dict(L=0), dict(n_aff=0), dict(n_aff=-2), dict(docids=one, n_docs=-1)):
        assert call(**bad) == -1, bad
    # the list bound is the layout's own
    lo, hi = 1, 1 << 20
    assert int(lib.ultr_loss_lds_bytes(_lib.ALGO_AFFINE, lo)) > 0 and int(lib.ultr_loss_lds_bytes(_lib.ALGO_AFFINE, hi)) == -2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if int(lib.ultr_loss_lds_bytes(_lib.ALGO_AFFINE, mid)) >= 0 else (lo, mid)
    assert lo == 4095 and int(lib.ultr_loss_lds_bytes(_lib.ALGO_AFFINE, lo)) == int(lib.ultr_loss_lds_bytes(_lib.ALGO_SOFTMAX, lo))
    assert call(L=lo + 1) == -2 and call(L=lo + 1, B=0) == -1
    assert "list_size up to %d " % lo in hdr[hdr.index("---- AffineRank"):hdr.index("int ultr_affine_loss(")]
    assert int(lib.ultr_loss_lds_bytes(_lib.ALGO_AFFINE, 0)) == -1


def test_optimizer_state_is_sized_as_softmax():
    from ultra_pytorch_amd import _lib
    lib = _lib.load()
    for opt, n in ((_lib.OPT_ADAGRAD, 1000), (_lib.OPT_SGD, 0), (_lib.OPT_ADAM, 2000)):
        u = _lib.UpdateDesc()
        u.algo, u.optimizer, u.list_size, u.n_params = _lib.ALGO_AFFINE, opt, 10, 1000
        got = int(lib.ultr_opt_state_floats(ctypes.byref(u)))
        u.algo = _lib.ALGO_SOFTMAX
        assert got == int(lib.ultr_opt_state_floats(ctypes.byref(u))) == n
    u.algo = 13  # the next value is no algorithm
    assert int(lib.ultr_opt_state_floats(ctypes.byref(u))) == -1
