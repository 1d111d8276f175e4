"""PRSrank without a GPU: the float64 restatement (tests/prs_ref.py) against the reference's own steps
(tests/golden/prs_*.npz, made by tests/golden/make_golden_prs.py), the plugin seam and hyper-parameters, the ABI constants."""
import os
import re

import numpy as np
import pytest
import torch

from tests import prs_ref
from tests.hipref import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["prs_tiny", "prs_odd", "prs_sgd", "prs_setrank_tiny", "prs_l50"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    d, m = load_golden(name)
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        r = prs_ref.fixture_step(d, m, t)
        np.testing.assert_allclose(r["scores"], d[p + "scores"], atol=1e-5, rtol=0)
        ref_loss = float(d[p + "loss"])
        assert abs(r["loss"] - ref_loss) <= 1e-6 * abs(ref_loss), (r["loss"], ref_loss)
        g = d[p + "grads"]
        np.testing.assert_allclose(r["grads"], g, rtol=0, atol=1e-5 * float(np.abs(g).max()))
        assert abs(r["norm"] - float(d[p + "norm"])) <= 1e-5 * max(1.0, float(d[p + "norm"]))


def test_l50_fixture_clamps_the_table():
    d, m = load_golden("prs_l50")
    assert m["L"] > len(d["ipw_list"])
    ipw, pw = prs_ref.ipw_of_positions(d["ipw_list"], m["L"])
    assert (ipw[len(d["ipw_list"]):] == float(d["ipw_list"][-1])).all()


def test_saturation_quirks_of_the_restatement():
    """The float32 chain reproduces what the reference's autograd does at large gaps: a clamped loss of 100 x weight
    with an exploding (not saturating) gradient once x rounds to 1, NaN once exp overflows in the lower triangle."""
    lab = np.array([[0.0, 1.0]])
    ipw = [1.0]
    # gap 17: x == 1.0 in fp32, BCE(1, 0) = 100; dL/dz = 1 / 1e-12 * exp(-17) ~ 4.1e4 (times the delta weight)
    loss, g = prs_ref.prs_score_grad(np.array([[17.0, 0.0]]), lab, ipw, dtype=torch.float32)
    w = np.log(2.0) * (1.0 - 1.0 / np.log2(3.0))  # |g_i - g_j| / IDCG = 1 / (1 / ln 2), times the discount difference
    assert abs(loss - 100.0 * w) <= 1e-4 * 100.0 * w
    assert abs(g[0, 0] - np.exp(-17.0) * 1e12 * w) <= 1e-3 * abs(g[0, 0]) and g[0, 1] == -g[0, 0]
    # gap 95: exp(95) overflows in the lower triangle -> NaN for both scores of the pair
    loss, g = prs_ref.prs_score_grad(np.array([[95.0, 0.0]]), lab, ipw, dtype=torch.float32)
    assert np.isfinite(loss) and np.isnan(g).all()
    # float64 does not saturate at gap 17
    _, g64 = prs_ref.prs_score_grad(np.array([[17.0, 0.0]]), lab, ipw)
    assert abs(g64[0, 0]) < 2.0 * w


def test_plugin_resolves_by_class_path():
    from ultra_pytorch_amd.utils import find_class
    import ultra_pytorch_amd.learning_algorithm as la
    cls = find_class("ultra_pytorch_amd.learning_algorithm.PRSrank")
    assert cls is la.PRSrank and cls.ENGINE_ALGO == "prs"


def _hparams_of(values):
    """The hyper-parameter object PRSrank.__init__ builds, parsed without constructing the (GPU-only) algorithm."""
    from ultra_pytorch_amd.learning_algorithm import PRSrank
    from ultra_pytorch_amd.utils import HParams
    return HParams(**PRSrank.DEFAULT_HPARAMS).parse(values)


def test_hparams_parse_as_the_reference(capsys):
    hp = _hparams_of("")
    assert hp.values() == dict(
        propensity_estimator_type="ultra.utils.propensity_estimator.RandomizedPropensityEstimator",
        propensity_estimator_json="./example/PropensityEstimator/randomized_pbm_0.1_1.0_4_1.0.json",
        learning_rate=0.05, max_gradient_norm=5.0, grad_strategy="ada", sigma=1.0)
    hp = _hparams_of("sigma=2.5,learning_rate=0.1,grad_strategy=sgd,l2_loss=1.0")
    assert hp.sigma == 2.5 and hp.learning_rate == 0.1 and hp.grad_strategy == "sgd"
    assert not hasattr(hp, "l2_loss")  # PRSrank has no l2_loss: reported and ignored
    assert "Unknown hyperparameter type for l2_loss" in capsys.readouterr().out


def test_shipped_estimator_table_is_found():
    from ultra_pytorch_amd.learning_algorithm.ipw_rank import load_ipw_list
    ipw = load_ipw_list("./example/PropensityEstimator/randomized_pbm_0.1_1.0_4_1.0.json")
    assert len(ipw) == 40 and all(v > 0 for v in ipw)


def test_abi_constants():
    from ultra_pytorch_amd import _lib, engine
    hdr = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    assert int(re.search(r"ULTR_ALGO_PRS\s*=\s*(\d+)", hdr).group(1)) == _lib.ALGO_PRS == 5
    assert re.search(r"\bint ultr_prs_loss\(", hdr)
    assert "ultr_prs_loss" in _lib.SIGNATURES
    assert engine.ALGOS["prs"] == _lib.ALGO_PRS
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8
