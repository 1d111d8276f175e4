"""PLRank without a GPU: the yardstick itself (tests/plrank_ref.py) against the exact expected reward, the kernel's float32 arithmetic
restated in numpy against the yardstick, hyper-parameter parsing, and what the built library exports and refuses on the host.

Bars (tests/loss_ref.py): SCALAR_RTOL for the per-sample reward, TERMS_RTOL * (|ref| + sum |terms|) for the per-sample gradient - plus
float32's smallest normal number as an absolute floor: below it a float32 output carries no relative precision."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import loss_ref as R
from tests import plrank_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("L,K", [(4, 4), (5, 3), (5, 1)])
def test_the_estimator_is_unbiased_for_the_exact_gradient(L, K):
    """Enumerated over all L! rankings, the expectation of the twin's g equals the central-difference gradient of the exact expected
    reward to 1e-7."""
    rng = np.random.RandomState(100 * L + K)
    s = rng.normal(scale=1.2, size=L).astype(np.float32).astype(np.float64)
    rho = rng.uniform(0.0, 3.0, size=L) * (rng.uniform(size=L) < 0.7)
    reward, mean, sd = T.enumerate_exact(s, rho, K)
    assert abs(reward - T.exact_reward(s, rho, K)) <= 1e-12
    h = 1e-5
    grad = np.zeros(L)
    for d in range(L):
        up, dn = s.copy(), s.copy()
        up[d] += h
        dn[d] -= h
        grad[d] = (T.exact_reward(up, rho, K) - T.exact_reward(dn, rho, K)) / (2 * h)
    err = float(np.abs(mean - grad).max())
    print("L=%d K=%d: |E[g] - central difference| = %.3g; sd of g up to %.3g" % (L, K, err, sd.max()))
    assert err <= 1e-7
    assert abs(grad.sum()) <= 1e-7 and (sd > 0).any()  # a shift of all scores changes nothing


def _uniforms(rng, n):
    return (rng.randint(0, 1 << 24, size=n).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def _random_lists(rng, B, L, scale, pads):
    scores = (rng.normal(size=(B, L)) * scale).astype(np.float32)
    docids = np.zeros((L, B), np.int32)
    if pads and L > 2:
        docids[rng.randint(0, L, size=B), np.arange(B)] = 7  # one PAD per list (n_docs = 7)
        docids[L - 1, ::3] = 7
    labels = (rng.uniform(size=(L, B)) < 0.3).astype(np.float32) * rng.choice(np.array([1.0, 1.0, 2.0, 0.5], np.float32), size=(L, B))
    return scores, docids, labels


@pytest.mark.parametrize("scale", [1.5, 8.0, 40.0])
def test_the_kernels_float32_arithmetic_holds_the_bars(scale):
    """About 6700 random (list, sample) pairs per score scale (2 x 10^4 in all): per-sample g in the kernel's float32 arithmetic
    (two-factor staging, scans in trips of 64 lanes) against the float64 law.  At scale 40 documents underflow to probability 0."""
    rng = np.random.RandomState(int(scale * 10))
    worst_g = worst_r = 0.0
    pairs = zero_prob = 0
    for L, B, N, cutoff, gain, weights in [(10, 200, 10, 0, "linear", "table"), (70, 100, 20, 5, "exp2", "pw"),
                                           (130, 60, 45, 0, "linear", None)]:
        scores, docids, labels = _random_lists(rng, B, L, scale, pads=True)
        valid = T.valid_of(docids, 7)
        pw = rng.uniform(0.5, 4.0, size=(B, L)).astype(np.float32) if weights == "pw" else None
        ipw = np.array([1.0, 1.6, 2.2, 3.1], np.float32) if weights == "table" else None
        rho = T.rho_of(labels, valid, gain, pw=pw, ipw=ipw)
        n_pos, _ = T.n_pos_of(scores, valid)
        zero_prob += int((valid.sum(axis=1) - n_pos).sum())
        orders = np.zeros((B, N, L), np.int64)
        for b in range(B):
            for n in range(N):
                orders[b, n] = T.order_of(scores[b], valid[b], _uniforms(rng, L))[0]
        g64, t64, fr64 = T.per_sample(scores, rho, valid, orders, T.cutoff_of(cutoff, L), n_pos)
        g32, fr32 = T.kernel_f32(scores, rho, valid, orders, cutoff, n_pos)
        assert np.isfinite(g32).all() and (g32[~np.broadcast_to(valid[:, None, :], g32.shape)] == 0).all()
        err = np.abs(g32.astype(np.float64) - g64)
        bar = T.dscores_bar(g64, t64, R.TERMS_RTOL)
        worst_g = max(worst_g, float((err / bar).max()))
        worst_r = max(worst_r, float((np.abs(fr32 - fr64) / np.maximum(1.0, np.abs(fr64))).max()))
        assert (err <= bar).all(), (L, float((err / bar).max()))
        pairs += B * N
    print("scale %g: %d pairs, %d zero-probability documents; worst g error %.3g of its bar, reward %.3g (bar %.0e)"
          % (scale, pairs, zero_prob, worst_g, worst_r, R.SCALAR_RTOL))
    assert worst_r <= R.SCALAR_RTOL and pairs >= 6600
    if scale == 40.0:
        assert zero_prob > 0


def test_hyper_parameters():
    from ultra_pytorch_amd.learning_algorithm import PLRank
    hp = PLRank.parse_hparams("")
    assert (hp.learning_rate, hp.max_gradient_norm, hp.l2_loss, hp.grad_strategy) == (0.05, 5.0, 0.0, "ada")
    assert (hp.num_samples, hp.cutoff, hp.gain) == (64, 0, "linear")
    assert hp.propensity_estimator_type.endswith("RandomizedPropensityEstimator")
    hp = PLRank.parse_hparams("num_samples=256,cutoff=10,gain=exp2,grad_strategy=adam,l2_loss=0.01,learning_rate=0.1")
    assert (hp.num_samples, hp.cutoff, hp.gain, hp.grad_strategy, hp.l2_loss, hp.learning_rate) == (256, 10, "exp2", "adam", 0.01, 0.1)
    with pytest.raises(ValueError, match="gain"):
        PLRank.parse_hparams("gain=log")
    for bad in (0, 4096, -3):
        with pytest.raises(ValueError, match="num_samples"):
            PLRank.parse_hparams("num_samples=%d" % bad)
    assert PLRank.parse_hparams("num_samples=1").num_samples == 1 and PLRank.parse_hparams("num_samples=4095").num_samples == 4095


def test_entry_is_exported_bound_and_declared():
    from ultra_pytorch_amd import _lib, engine, hip_ops
    lib = _lib.load()
    assert int(lib.ultr_abi_version()) == _lib.ABI_VERSION == 8
    assert hasattr(lib, "ultr_plrank_loss") and "plrank" in engine.ALGOS and engine.ALGOS["plrank"] == _lib.ALGO_PLRANK
    hdr = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    m = re.search(r"\bint ultr_plrank_loss\(([^)]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == 18 == len(_lib.SIGNATURES["ultr_plrank_loss"][1])
    assert re.search(r"ULTR_ALGO_PLRANK = %d\b" % _lib.ALGO_PLRANK, hdr)
    # bad arguments are refused on the host, with nothing launched
    one = ctypes.c_void_p(16)  # (never dereferenced: every call below is refused before a launch)
    ok = dict(cutoff=0, n=64, gain=0, B=3, L=5)
    for bad in (dict(n=0), dict(n=4096), dict(gain=2), dict(cutoff=-1), dict(B=0), dict(L=0)):
        a = dict(ok, **bad)
        assert lib.ultr_plrank_loss(one, one, None, None, 0, one, 10, a["cutoff"], a["n"], a["gain"], 1, 2, a["B"], a["L"], one, None, one,
                                    None) == -1, bad
    assert lib.ultr_plrank_loss(None, one, None, None, 0, one, 10, 0, 64, 0, 1, 2, 3, 5, one, None, one, None) == -1
    assert lib.ultr_plrank_loss(one, one, None, one, 0, one, 10, 0, 64, 0, 1, 2, 3, 5, one, None, one, None) == -1  # a table of none
    assert lib.ultr_plrank_loss(one, one, None, None, 0, one, 10, 0, 64, 0, 1, 2, 3, T.MAX_L + 1, one, None, one, None) == -2
    # the descriptor field of a step
    assert _lib.plrank_pack(0, 64, "linear") == 64 << 12 and _lib.plrank_pack(10, 4095, "exp2") == 10 | (4095 << 12) | (1 << 24)
    assert _lib.plrank_pack(5000, 1, "linear") == 4095 | (1 << 12)
    # optimizer state: the ranker's alone
    P = 1234
    assert [engine.opt_state_floats("plrank", o, 17, P) for o in ("sgd", "ada", "adam")] == [0, P, 2 * P]


def test_lds_layout_bound():
    """ultr_loss_lds_bytes is positive up to the stated longest list, ULTR_E_UNSUPPORTED one past it; header and DESIGN state it."""
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    words = lambda L: 88 * L + 37  # noqa: E731  (tail 4 + 2 L, six arrays per list, 16 waves x (5 L + 1), 17 words of sums)
    for L in (1, 2, 64, 65, 256, T.MAX_L):
        assert int(lib.ultr_loss_lds_bytes(_lib.ALGO_PLRANK, L)) == 4 * words(L) <= 160 * 1024
    longest = max(L for L in range(400, 520) if int(lib.ultr_loss_lds_bytes(_lib.ALGO_PLRANK, L)) >= 0)
    assert longest == T.MAX_L and int(lib.ultr_loss_lds_bytes(_lib.ALGO_PLRANK, longest + 1)) == -2
    assert int(lib.ultr_loss_lds_bytes(_lib.ALGO_PLRANK, 0)) == -1
    assert hip_ops.loss_route(_lib.ALGO_PLRANK, longest) == "short"
    with pytest.raises(_lib.UltrHipError):
        hip_ops.loss_route(_lib.ALGO_PLRANK, longest + 1)
    hdr = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    assert "list_size up to %d " % longest in hdr[hdr.index("---- PLRank"):hdr.index("int ultr_plrank_loss(")]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 4d." in design and "%d documents" % longest in design[design.index("## 4d."):]
