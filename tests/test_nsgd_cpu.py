"""NSGD on the host: the restatement (tests/nsgd_ref.py, tests/dbgd_ref.py) against the reference's recorded steps
(tests/golden/nsgd_*.npz, make_golden_nsgd.py) from the recorded noise; the reference's noise quirk the law departs from; the
restated null-space law against an SVD; the plugin's defaults and export; the C-ABI entries.  CPU only."""
import json
import os
import re

import numpy as np
import pytest

from tests import dbgd_ref as D
from tests import ndcg_ref as N
from tests import nsgd_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_FIXTURES = ["nsgd_noint", "nsgd_ada", "nsgd_linear"]


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return d, json.loads(str(d["meta"]))


def ndcg_mean(scores_BL, labels_LB, topn):
    return float(np.mean(N.ndcg_per_list(np.asarray(scores_BL, np.float32), np.asarray(labels_LB, np.float32).T, [topn])[0]))


@pytest.mark.parametrize("name", STEP_FIXTURES)
def test_restatement_reproduces_the_recorded_steps(name):
    d, m = load(name)
    F, hidden, cut, R = m["F"], m["hidden"] or [], m["cutoff"], m["R"]
    assert not m["need_interleave"]
    _, P = D.layout(F, hidden)
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        u, lab = d[p + "unit_noise"].astype(np.float64), d[p + "labels"]
        assert u.shape == (R, P)
        if t > 0:  # the memory carries over from step to step
            assert np.array_equal(d[p + "pre_memory"], d["s%d_post_memory" % (t - 1)])
        # the loss and every ranker's NDCG: the current model's and the last candidate's are restated from their scores
        nd = d[p + "ndcg"]
        assert abs((1.0 - nd[0]) - float(d[p + "loss"])) < 1e-6
        assert abs(ndcg_mean(d[p + "scores"][:, :cut], lab[:cut], cut) - nd[0]) < 1e-6
        assert abs(ndcg_mean(d[p + "cand_scores"], lab[:cut], cut) - nd[R]) < 1e-6
        # the winners, the gradient (the reference's parameter.grad is the negative of the direction applied here)
        g = np.ceil(nd.astype(np.float32) - np.float32(nd[0])).astype(np.float32)
        np.testing.assert_allclose(g / (g.sum() + np.float32(1e-9)), d[p + "final_winners"], rtol=1e-6)
        c = D.ranker_weights(ndcg=nd)
        grads = D.gradient(u, c)
        np.testing.assert_allclose(grads, -d[p + "grads"].astype(np.float64), atol=1e-6)
        assert abs(float(np.sqrt((grads ** 2).sum())) - float(d[p + "norm"])) < 1e-5
        # the memory, exactly
        lost = S.losers(R, ndcg=nd)
        assert np.array_equal(S.memory_update(d[p + "unit_noise"], lost, F, hidden), d[p + "post_memory"])
        # the update on the restated direction: the reference's step mirrored about theta_pre
        th = d[p + "pre_params"].astype(np.float64)
        gc = grads * float(d[p + "clip_coef"])
        if m["grad_strategy"] == "sgd":
            ours = th - m["lr"] * gc
        else:
            s = d[p + "pre_adagrad"].astype(np.float64) + gc * gc
            np.testing.assert_allclose(s, d[p + "post_adagrad"], rtol=1e-5, atol=1e-9)
            ours = th - m["lr"] * gc / (np.sqrt(s) + 1e-10)
        np.testing.assert_allclose(ours, th - (d[p + "post_params"] - th), atol=2e-6)


def test_fixtures_cover_the_cases():
    all_lost = won = False
    for name in STEP_FIXTURES:
        d, m = load(name)
        for t in range(m["n_steps"]):
            fw, post = d["s%d_final_winners" % t], d["s%d_post_memory" % t]
            if fw.sum() == 0:
                all_lost = True
                assert post.any(0).sum() > 0 and all(post[r].any() for r in range(m["R"]))
            else:
                won = True
                assert not post.any()
    assert all_lost and won
    d, m = load("nsgd_noint")
    assert m["R"] == 3 and m["grad_strategy"] == "sgd" and m["model"] == "DNN"
    assert any(d["s%d_final_winners" % t].sum() == 0 for t in range(m["n_steps"]))
    assert any(d["s%d_final_winners" % t].sum() != 0 for t in range(m["n_steps"]))
    ms = [load(n)[1] for n in STEP_FIXTURES]
    assert {x["grad_strategy"] for x in ms} == {"sgd", "ada"} and {x["model"] for x in ms} == {"DNN", "Linear"}
    for name in STEP_FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 100 * 1024


@pytest.mark.parametrize("name", STEP_FIXTURES)
def test_reference_noise_lies_in_the_first_R_axes(name):
    """The quirk the law departs from: torch.svd of the empty memory returns the first R coordinate axes, and every later null space
    stays in their span, so the reference's noise (and update) touches only the first R entries of each flattened Linear tensor."""
    d, m = load(name)
    R = m["R"]
    for t in range(m["n_steps"]):
        u = d["s%d_unit_noise" % t]
        for off, n, scalar in S.tensors(m["F"], m["hidden"] or []):
            seg = u[:, off:off + n]
            assert not seg[:, R:].any()
            nrm = np.sqrt((seg.astype(np.float64) ** 2).sum(1))
            assert np.all((np.abs(nrm - 1) < 1e-5) | (nrm == 0))  # unit, or 0 once the memory fills the null space
            if scalar:
                assert set(np.unique(seg)) <= {-1.0, 1.0}


def _svd_projection(z, mt, tol=1e-6):
    """The complement of the row space of mt through numpy's SVD (the check on the restated pivoted-Cholesky projection)."""
    if not mt.any():
        return z
    _, s, vt = np.linalg.svd(mt, full_matrices=False)
    V = vt[s > tol * s.max()]
    return z - (z @ V.T) @ V


def test_null_space_law_against_svd():
    rng = np.random.RandomState(0)
    F, hidden, R = 12, [9, 3], 5
    tens = S.tensors(F, hidden)
    _, P = D.layout(F, hidden)
    mem = np.zeros((R, P), np.float32)
    for off, n, _ in tens:
        mem[:, off:off + n] = rng.standard_normal((R, n))
    mem[1] = 0.0  # an empty slot
    w_off, w_n, _ = tens[0]
    mem[3, w_off:w_off + w_n] = mem[0, w_off:w_off + w_n] + mem[2, w_off:w_off + w_n]  # a dependent row of the first weight
    z = S.normals(5, 7, R, P)
    u = S.null_space_noise(z, mem, F, hidden)
    lay, _ = D.layout(F, hidden)
    for og, k, *_ in lay:
        assert not u[:, og:og + 2 * k].any()  # LayerNorm: no noise
    for off, n, scalar in tens:
        ut, mt, zt = u[:, off:off + n], mem[:, off:off + n].astype(np.float64), z[:, off:off + n]
        if scalar:
            assert set(np.unique(ut)) <= {-1.0, 1.0}
            continue
        if n <= 4:  # the bias of 3 entries: the 4 non-empty rows span it
            assert not ut.any()
            continue
        np.testing.assert_allclose(np.sqrt((ut ** 2).sum(1)), 1.0, atol=1e-12)
        kept = S.kept_rows(mt)
        assert np.abs(ut @ mt[kept].T).max() < 1e-10
        assert np.abs(ut @ mt.T).max() < 1e-5  # (a dropped row depends on the kept ones up to float32 rounding)
        v = _svd_projection(zt, mt)
        np.testing.assert_allclose(ut, v / np.sqrt((v ** 2).sum(1, keepdims=True)), atol=1e-7)
    assert S.kept_rows(mem[:, w_off:w_off + w_n]) and len(S.kept_rows(mem[:, w_off:w_off + w_n])) == 3
    # the empty memory: the reference's whole-tensor normalization, not DBGD's per-column one
    u0 = S.null_space_noise(z, np.zeros_like(mem), F, hidden)
    for off, n, _ in tens:
        zt = z[:, off:off + n]
        np.testing.assert_allclose(u0[:, off:off + n], zt / np.sqrt((zt ** 2).sum(1, keepdims=True)), atol=1e-12)


def test_loser_rules():
    W = np.array([[0.0, 0.5, 0.0, 0.5], [0.0, 0.0, 0.0, 1.0]], np.float32)
    assert S.losers(3, winners_BR=W).tolist() == [False, True, False]
    assert S.losers(3, ndcg=[0.5, 0.4, 0.5, 0.3]).tolist() == [True] * 3
    assert S.losers(3, ndcg=[0.5, 0.4, 0.6, 0.3]).tolist() == [False] * 3


def test_hparam_defaults_and_export():
    from ultra_pytorch_amd import learning_algorithm
    from ultra_pytorch_amd.utils import find_class
    assert find_class("ultra_pytorch_amd.learning_algorithm.NSGD") is learning_algorithm.NSGD
    ref = dict(click_model_json="./example/ClickModel/pbm_0.1_1.0_4_1.0.json", learning_rate=0.5, max_gradient_norm=5.0,
               need_interleave=True, grad_strategy="sgd", ranker_num=4)
    assert learning_algorithm.NSGD.DEFAULT_HPARAMS == dict(ref, interleave_strategy="Stochastic", tau=1)
    assert learning_algorithm.NSGD.DEFAULT_HPARAMS == learning_algorithm.MGD.DEFAULT_HPARAMS
    assert learning_algorithm.NSGD.BANNER == "Build Null Space Gradient Descent (DBGD) algorithm."
    assert issubclass(learning_algorithm.NSGD, learning_algorithm.DBGD) and learning_algorithm.NSGD.INTERLEAVES_IN_TRAIN


def test_abi_entries():
    from ultra_pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION
    for fn in ("ultr_nsgd_noise_args", "ultr_nsgd_memory_args"):
        assert re.search(r"\bint %s\(const ultr_nsgd_args\* a, void\* stream\);" % fn, hdr) and fn in _lib.SIGNATURES
    assert re.search(r"\bint64_t ultr_nsgd_workspace_bytes\(const ultr_dnn_desc\* desc, int32_t n_rankers\);", hdr)
    assert "ultr_nsgd_workspace_bytes" in _lib.SIGNATURES
    body = hdr[hdr.index("typedef struct ultr_nsgd_args"):hdr.index("} ultr_nsgd_args;")]
    fields = re.findall(r"\b(\w+)(?:,|;)", body.split("{", 1)[1])
    assert fields == [f for f, _ in _lib.NsgdArgs._fields_] == ["dbgd", "memory", "normals_in", "unit_noise_in", "ws"]
    assert int(re.search(r"#define\s+ULTR_DBGD_MAX_RANKERS\s+(\d+)", hdr).group(1)) == _lib.DBGD_MAX_RANKERS == 16
