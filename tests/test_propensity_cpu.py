"""Propensity estimation without a GPU: the ABI entry, the reference's table formula, the Oracle estimator, the JSON files, and the
session law itself - the numpy restatement (tests/propensity_ref.py) of ultr_propensity_count must recover the position-biased
model's true weights on the golden dataset within 6 sigma of the analytic count statistics (the bar tests/test_gpu_propensity.py
holds the device to, at the same seed)."""
import json
import os
import re

import numpy as np
import pytest

from tests import propensity_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "ultra_pytorch_amd", "data")
GOLDEN = os.path.join(ROOT, "tests", "golden", "propensity_ref.npz")


def _desc(name):
    with open(os.path.join(DATA, name)) as f:
        return json.load(f)


def test_abi_entry():
    from ultra_pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION
    assert re.search(r"\bint ultr_propensity_count\(const ultr_propensity_args\* a, void\* stream\);", hdr)
    assert "ultr_propensity_count" in _lib.SIGNATURES
    assert int(re.search(r"#define\s+ULTR_PROPENSITY_MAX_L\s+(\d+)", hdr).group(1)) == _lib.PROPENSITY_MAX_L >= 128
    body = hdr[hdr.index("typedef struct ultr_propensity_args"):hdr.index("} ultr_propensity_args;")]
    fields = re.findall(r"\b(\w+)(?:,|;)", body.split("{", 1)[1])
    assert fields == [f for f, _ in _lib.PropensityArgs._fields_]
    assert _lib.load().ultr_abi_version() == 8


def test_formula_on_hand_made_counts():
    """4 positions; the longest length (4) never occurs, position 2 was never clicked (agg == 0: the clamp min(.., first) shows)."""
    from ultra_pytorch_amd.utils.propensity_estimator import ipw_from_click_count
    cc = [[40, 0, 0, 0],
          [30, 15, 0, 0],
          [20, 5, 0, 0],
          [0, 0, 0, 0]]
    want = [90 / (90 + 10e-6), 50 / (20 + 10e-6), 20.0, 0.0]
    got = R.ipw_formula(cc)
    assert got == want                                  # first = [90, 50, 20, 0], agg = [90, 20, 0, 0]
    assert got[2] == 20.0 and 20 / 10e-6 > 20.0         # 20 / (0 + 10e-6) = 2e6 is clamped to first
    assert got[3] == 0.0                                # 0 / 10e-6
    assert ipw_from_click_count(np.asarray(cc, np.int64)) == want
    # entries above the diagonal are never read (the reference's rows are ragged)
    junk = np.asarray(cc, np.int64) + np.triu(np.full((4, 4), 7, np.int64), 1)
    assert R.ipw_formula(junk) == want and ipw_from_click_count(junk) == want


@pytest.mark.parametrize("name", ["pbm_0.1_1.0_4_1.0.json", "cascade_0.1_1.0_4_1.0.json", "ubm_0.1_1_4_1.0.json"])
def test_oracle_estimator_answers_from_the_click_model(name, tmp_path):
    from ultra_pytorch_amd.utils import click_models as CM
    from ultra_pytorch_amd.utils.propensity_estimator import OraclePropensityEstimator
    cm = CM.loadModelFromJson(_desc(name))
    est = OraclePropensityEstimator(cm)
    clicks = [0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0]
    for non_clicked in (False, True):
        assert est.getPropensityForOneList(clicks, non_clicked) == cm.estimatePropensityWeightsForOneList(clicks, non_clicked)
    assert est.getPropensityForOneList(clicks)[0] == 0.0 and est.getPropensityForOneList(clicks)[1] > 0.0
    path = str(tmp_path / "oracle.json")
    est.outputEstimatorToFile(path)
    assert set(json.load(open(path))) == {"click_model"}
    back = OraclePropensityEstimator(None)
    back.loadEstimatorFromFile(path)
    assert type(back.click_model) is type(cm) and back.click_model.getModelJson() == cm.getModelJson()
    assert back.getPropensityForOneList(clicks, True) == est.getPropensityForOneList(clicks, True)


def test_randomized_estimator_json_round_trip(tmp_path):
    from ultra_pytorch_amd.utils import click_models as CM
    from ultra_pytorch_amd.utils.propensity_estimator import BasicPropensityEstimator, RandomizedPropensityEstimator
    est = RandomizedPropensityEstimator()
    assert est.click_model is None and est.IPW_list == []
    est.click_model = CM.loadModelFromJson(_desc("cascade_0.1_1.0_4_1.0.json"))
    est.IPW_list = [1.0, 1.25, 3.5]
    path = str(tmp_path / "randomized.json")
    est.outputEstimatorToFile(path)
    data = json.load(open(path))
    assert set(data) == {"click_model", "IPW_list"} and data["click_model"]["model_name"] == "cascade_model"
    back = RandomizedPropensityEstimator(path)
    assert back.IPW_list == est.IPW_list and isinstance(back.click_model, CM.CascadeModel)
    assert back.getPropensityForOneList([1, 0, 1, 1, 1]) == [1.0, 0.0, 3.5, 3.5, 3.5]
    # a table without a click model (what BasicPropensityEstimator writes) loads with click_model None
    plain = str(tmp_path / "plain.json")
    BasicPropensityEstimator.outputEstimatorToFile(est, plain)
    assert RandomizedPropensityEstimator(plain).click_model is None and RandomizedPropensityEstimator(plain).IPW_list == est.IPW_list


def test_shipped_table_still_loads():
    from ultra_pytorch_amd.learning_algorithm.ipw_rank import load_ipw_list
    from ultra_pytorch_amd.utils import click_models as CM
    from ultra_pytorch_amd.utils.propensity_estimator import RandomizedPropensityEstimator
    path = os.path.join(DATA, "randomized_pbm_0.1_1.0_4_1.0.json")
    est = RandomizedPropensityEstimator(path)
    raw = json.load(open(path))
    assert est.IPW_list == raw["IPW_list"] == load_ipw_list(path) and len(est.IPW_list) > 0
    assert isinstance(est.click_model, CM.PositionBiasedModel) and est.click_model.exam_prob == raw["click_model"]["exam_prob"]
    assert est.getPropensityForOneList([0, 1])[1] == raw["IPW_list"][1]


def test_module_docstring_and_unknown_click_model():
    from ultra_pytorch_amd.utils import propensity_estimator as PE
    assert "offline tooling" not in open(PE.__file__).read()

    class Other(object):
        model_name = "dependent_click_model"

    class Data(object):
        rank_list_size, labels = 2, [[1, 0]]

    with pytest.raises(NotImplementedError, match="position-biased, the cascade and the user-browsing model"):
        PE.RandomizedPropensityEstimator().estimateParametersFromModel(Other(), Data())


def test_restatement_recovers_the_pbm_weights():
    """The session law alone, on the golden dataset, PBM, seed 0, 2^20 sessions: |IPW[x] - e[0] / e[min(x, 9)]| <= 6 sigma_x with
    sigma_x = IPW[x] sqrt(1 / E[first_x] + 1 / E[agg_x]) from the analytic expected counts."""
    g = np.load(GOLDEN)
    d = _desc("pbm_0.1_1.0_4_1.0.json")
    S = 1 << 20
    cc = R.click_count(g["labels"].astype(np.float32), g["lengths"], d["exam_prob"], len(d["exam_prob"]), d["click_prob"], R.PBM, 0, 0, S)
    lengths = g["lengths"]
    assert cc.sum() > 0 and np.array_equal(np.triu(cc, 1), np.zeros_like(cc))
    assert all(cc[n - 1].sum() > 0 for n in set(int(v) for v in lengths))
    ipw = np.asarray(R.ipw_formula(cc))
    e_first, e_agg, true = R.pbm_expectation(g["labels"], lengths, d["exam_prob"], d["click_prob"], S)
    bound = R.six_sigma(ipw, e_first, e_agg)
    print("IPW", ipw, "\ntrue", true, "\n|err| / bound", np.abs(ipw - true) / bound)
    assert np.all(np.abs(ipw - true) <= bound)
    # the realised counts sit at their analytic means (6 sigma of a binomial count, sigma^2 <= mean)
    first = np.array([cc[x:, 0].sum() for x in range(len(ipw))])
    assert np.all(np.abs(first - e_first) <= 6 * np.sqrt(e_first))
