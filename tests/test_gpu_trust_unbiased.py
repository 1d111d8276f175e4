"""The clicks ultr_click_batch draws under the trust-bias model carry the law they are meant to carry: the affine correction
(c - beta_k) / alpha_k averages to the click probability of the grade in every (rank, grade) cell, and the examination-only weight
c / exam[k] does not.

Five lists of ten positions, label[q][l] = (q + l) % 5: every grade stands at every rank.  The shipped model, max_tries = 1 (redrawing
click-less lists would bias the check), B = 4096 slots over the steps 0 .. 15: n ~ 13000 draws per cell.  Every number of the bar is
known: a cell's clicks are Bernoulli(p), p = alpha_k gamma + beta_k, so the mean of the corrected clicks has
sigma^2 = p (1 - p) / (alpha_k^2 n); the bar is 5 sigma.  The draw is a pure function of the seed: SEED was confirmed on the CPU with the
restatement (tests/trust_ref.click_draw) to pass both assertions before it was written here."""
import numpy as np
import pytest
import torch

from tests import trust_ref as T
from tests.test_gpu_draws import run_click

pytestmark = pytest.mark.gpu

SEED, B, L, STEPS = 20260101, 4096, 10, 16
LISTS = np.arange(50, dtype=np.int32).reshape(5, 10)
LABELS = ((np.arange(5)[:, None] + np.arange(10)[None, :]) % 5).astype(np.float32)


def hold(clicks, q):
    """clicks [steps, L, B], q [steps, B]: both assertions, cell by cell.  Returns the largest |z| of the affine estimate."""
    hm = T.shipped_model()
    alpha, beta = (np.asarray(x, np.float64) for x in hm.affine_parameters(L))
    exam = np.asarray(hm.exam_prob, np.float64)
    gamma_of = np.asarray(hm.click_prob, np.float64)
    grade = LABELS[q].transpose(0, 2, 1).astype(np.int64)  # [steps, L, B]
    worst = 0.0
    for k in range(L):
        for g in range(5):
            c = clicks[:, k, :][grade[:, k, :] == g].astype(np.float64)
            n, gamma = c.size, gamma_of[g]
            p = alpha[k] * gamma + beta[k]
            sigma = np.sqrt(p * (1.0 - p) / n) / alpha[k]
            z = (((c - beta[k]) / alpha[k]).mean() - gamma) / sigma
            print("rank %d grade %d: n %d, affine estimate %.4f (gamma %.2f, z %+.2f), examination-only %.4f"
                  % (k, g, n, ((c - beta[k]) / alpha[k]).mean(), gamma, z, (c / exam[k]).mean()))
            assert n > 10000 and abs(z) <= 5.0, (k, g, z)
            worst = max(worst, abs(z))
            if (k, g) == (0, 0):
                # the examination-only estimate: sigma of c / exam is sqrt(p (1 - p) / n) / exam
                ips = (c / exam[0]).mean()
                assert abs(ips - gamma) > 5.0 * np.sqrt(p * (1.0 - p) / n) / exam[0] and 0.6 < ips < 0.76 and gamma == 0.1
    return worst


def test_affine_estimate_is_unbiased_and_examination_only_is_not():
    from ultra_pytorch_amd.utils import click_models
    hm = T.shipped_model()
    exam, n_exam, _ = click_models.device_tables(hm, 3, torch.device("cuda"))
    clicks, qs = [], []
    for step in range(STEPS):
        ids, ck, q = run_click(LISTS, LABELS, 50, exam, n_exam, hm.click_prob, T.TRUST, SEED, step, B, L, 1)
        assert np.array_equal(ids, LISTS[q].T)
        clicks.append(ck)
        qs.append(q)
    worst = hold(np.stack(clicks), np.stack(qs))
    print("largest |z| over the 50 cells: %.2f" % worst)
