"""The Oracle propensity estimator without a GPU: its weight tables against the click models' own per-list weights, the constructor
from an object and from the two kinds of JSON, the ABI declarations of the two new entries, and the restatement of the GPU lookup
(tests/history_pw_ref.py) against the weights the reference formed (tests/golden/oracle_pw/*.npz)."""
import itertools
import json
import os
import re

import numpy as np
import pytest

from tests import history_pw_ref as R
from tests.hipref import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "ultra_pytorch_amd", "data")
MODELS = ["pbm_0.1_1.0_4_1.0.json", "cascade_0.1_1.0_4_1.0.json", "ubm_0.1_1_4_1.0.json"]
FIXTURES = ["ipw_oracle_ubm_tiny", "ipw_oracle_ubm_odd", "ipw_oracle_pbm_tiny", "prs_oracle_ubm_tiny", "prs_oracle_ubm_l50",
            "ipw_oracle_ubm_setrank_tiny"]


def _model(name):
    from ultra_pytorch_amd.utils import click_models as CM
    return CM.loadModelFromJson(json.load(open(os.path.join(DATA, name))))


def _patterns():
    """(L, click lists): all 2^6 patterns at L 6, seeded random ones at L 12 and L 25 (beyond the models' 10 rows)."""
    out = [(6, [list(p) for p in itertools.product((0, 1), repeat=6)])]
    rng = np.random.RandomState(5)
    for L in (12, 25):
        pats = [(rng.uniform(size=L) < p).astype(int).tolist() for p in (0.1, 0.3, 0.6, 0.9) for _ in range(8)]
        out.append((L, pats + [[0] * L, [1] * L]))
    return out


def table_lookup(kind, w, clicks, all_positions):
    lab = np.asarray(clicks, np.float32)[:, None]  # [L, 1]
    return (R.history_pw if kind == "history" else R.position_pw)(lab, w, all_positions)[0]


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("all_positions", [False, True])
def test_weight_table_lookups_equal_the_click_models_weights(name, all_positions):
    from ultra_pytorch_amd.utils.propensity_estimator import OraclePropensityEstimator
    cm = _model(name)
    est = OraclePropensityEstimator(cm)
    for L, pats in _patterns():
        kind, w = est.weight_table(L)
        assert w.dtype == np.float32
        assert (kind, w.shape) == (("history", (L, L)) if "ubm" in name else ("position", (L,)))
        if kind == "history":
            assert not np.triu(w, 1).any() and (w[np.tril_indices(L)] > 0).all()
        for clicks in pats:
            want = np.asarray(cm.estimatePropensityWeightsForOneList(clicks, all_positions), np.float64).astype(np.float32)
            got = table_lookup(kind, w, clicks, all_positions)
            assert got.dtype == np.float32 and np.array_equal(got, want), (L, clicks)


def test_constructor_takes_an_object_an_oracle_json_and_a_randomized_json(tmp_path):
    from ultra_pytorch_amd.utils.propensity_estimator import OraclePropensityEstimator, RandomizedPropensityEstimator
    cm = _model(MODELS[2])
    a = OraclePropensityEstimator(cm)
    assert a.click_model is cm
    path = str(tmp_path / "oracle.json")
    a.outputEstimatorToFile(path)
    assert set(json.load(open(path))) == {"click_model"}
    b = OraclePropensityEstimator(path)
    assert b.click_model.getModelJson() == cm.getModelJson()
    assert np.array_equal(b.weight_table(12)[1], a.weight_table(12)[1])
    rnd = RandomizedPropensityEstimator()
    rnd.click_model, rnd.IPW_list = _model(MODELS[0]), [1.0, 2.0, 3.0]
    rpath = str(tmp_path / "randomized_pbm.json")
    rnd.outputEstimatorToFile(rpath)
    c = OraclePropensityEstimator(rpath)
    assert c.click_model.model_name == "position_biased_model"
    kind, w = c.weight_table(4)
    ep = c.click_model.exam_prob
    assert kind == "position" and np.array_equal(w, np.asarray([1.0 / ep[r] * ep[0] for r in range(4)], np.float32))
    bare = tmp_path / "table_only.json"
    bare.write_text(json.dumps({"IPW_list": [1.0]}))
    with pytest.raises(KeyError):
        OraclePropensityEstimator(str(bare))


def test_zero_examination_probability_and_unknown_models_raise():
    from ultra_pytorch_amd.utils import click_models as CM
    from ultra_pytorch_amd.utils.propensity_estimator import OraclePropensityEstimator
    pbm = _model(MODELS[0])
    pbm.exam_prob = list(pbm.exam_prob)
    pbm.exam_prob[3] = 0.0
    with pytest.raises(ValueError):
        OraclePropensityEstimator(pbm)
    ubm = _model(MODELS[2])
    ubm.exam_prob = [list(r) for r in ubm.exam_prob]
    ubm.exam_prob[4][2] = 0.0
    with pytest.raises(ValueError):
        OraclePropensityEstimator(ubm)
    with pytest.raises(NotImplementedError):
        OraclePropensityEstimator(CM.ClickModel())


def test_abi_declares_both_entries_and_stays_at_8():
    from ultra_pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == 8
    assert re.search(r"\bint ultr_history_pw\(const ultr_history_pw_args\* a, void\* stream\);", hdr)
    assert re.search(r"\bint ultr_prs_loss_pw\(", hdr)
    assert "ultr_history_pw" in _lib.SIGNATURES and "ultr_prs_loss_pw" in _lib.SIGNATURES
    # the argument block as the header declares it: three pointers, then batch, list_size, all_positions (+ padding)
    body = re.search(r"typedef struct ultr_history_pw_args \{(.*?)\} ultr_history_pw_args;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [n for n, _ in _lib.HistoryPwArgs._fields_] == ["labels", "table", "pw_out", "batch", "list_size", "all_positions", "pad_"]


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_recorded_weights(name):
    """The weights the reference's learner formed from each list's clicks, from weight_table + the lookup law: equal exactly."""
    from ultra_pytorch_amd.utils.propensity_estimator import OraclePropensityEstimator
    d, m = load_golden("oracle_pw/" + name)
    est = OraclePropensityEstimator(_model(m["oracle_model"]))
    assert est.click_model.getModelJson() == m["oracle_model_json"]  # the shipped file is the one the fixture was recorded with
    kind, w = est.weight_table(m["L"])
    assert kind == ("position" if "pbm" in name else "history")
    all_positions = m["algo"] == "prs"
    for t in range(m["n_steps"]):
        labels, want = d["s%d_labels" % t], d["s%d_pw" % t]
        got = (R.history_pw if kind == "history" else R.position_pw)(labels, w, all_positions)
        assert want.dtype == np.float32 and np.array_equal(got, want)
        if kind == "history":
            assert ((labels > 0).sum(0) >= 2).any()  # lists with several clicks: the history matters
