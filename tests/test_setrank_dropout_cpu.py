"""SetRank's dropout without a GPU: the restated mask law (tests/setrank_dropout_ref.py) has the statistics of a Bernoulli mask and
independent sites / steps / streams, the float64 restatement equals the pinned oracle at rate 0 and reproduces the step recorded
from the reference with site masks (tests/golden/setrank_dropout_tiny.npz), the C ABI declares and binds the entries, and the
model accepts `rate`."""
import os
import re

import numpy as np
import pytest
import torch

from tests import setrank_dropout_ref as R
from tests.hipref import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 20
GEOM = dict(B=16, L=64, d=1024)  # B * L * d = 2^20 elements


def _keep(rate, seed=7, step=3, stream=0, site=1):
    return R.keep(seed, step, stream, site, GEOM["B"], GEOM["L"], GEOM["d"], rate).reshape(-1)


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_mask_keep_fraction(rate):
    k = _keep(rate)
    assert k.size == N
    frac = float(k.mean())
    bound = 4.0 * np.sqrt(rate * (1.0 - rate) / N) + 2.0 ** -24
    print("rate %.2f keep fraction %.6f (bound %.2e around %.2f)" % (rate, frac, bound, 1.0 - rate))
    assert abs(frac - (1.0 - rate)) <= bound


def _corr(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.corrcoef(a, b)[0, 1])


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_mask_sites_steps_streams_are_independent(rate):
    base = _keep(rate)
    for what, other in (("site", _keep(rate, site=2)), ("step", _keep(rate, step=4)), ("stream", _keep(rate, stream=1))):
        c = _corr(base, other)
        print("rate %.2f %s correlation %.2e (bound %.2e)" % (rate, what, c, 4.0 / np.sqrt(N)))
        assert abs(c) <= 4.0 / np.sqrt(N), what


def test_mask_law_details():
    """The element takes word c & 3 of the quad c >> 2; a width that is no multiple of 4 cuts the last quad; scale is float32."""
    from tests import philox_ref as P
    B, L, d, rate, seed, step, stream, site = 3, 5, 30, 0.3, 0x123456789ABCDEF, 11, 2, 4
    k = R.keep(seed, step, stream, site, B, L, d, rate)
    assert k.shape == (B, L, d)
    for b, l, c in ((0, 0, 0), (2, 4, 29), (1, 3, 17)):
        w = P.philox4x32(l * B + b, (stream << 8) | site, c >> 2, R.SR_DROPOUT_TAG, *P.key(seed, step))[c & 3]
        assert bool(k[b, l, c]) == bool(P.u01(w) >= np.float32(rate))
    m = R.mask(seed, step, stream, site, B, L, d, rate)
    assert m.dtype == np.float32 and set(np.unique(m)) <= {np.float32(0.0), np.float32(1.0) / (np.float32(1.0) - np.float32(rate))}
    # distinct from every other Philox tag of csrc/
    tags = set()
    for fn in os.listdir(os.path.join(ROOT, "ultra_pytorch_amd", "csrc")):
        for name, v in re.findall(r"#define\s+(\w+_TAG)\s+(0x[0-9A-Fa-f]+)u", open(os.path.join(ROOT, "ultra_pytorch_amd", "csrc", fn)).read()):
            if name == "SR_DROPOUT_TAG":
                assert int(v, 16) == R.SR_DROPOUT_TAG
            else:
                tags.add(int(v, 16))
    assert len(tags) >= 10 and R.SR_DROPOUT_TAG not in tags and R.SR_DROPOUT_TAG != 0x5245454D  # (RegressionEM's word 2)


def test_restatement_equals_oracle_at_rate_0(monkeypatch):
    """(F, dm, H, nl, dff, B, L) = (20, 48, 6, 1, 20, 3, 7).  The oracle casts to float32 with Tensor.float(); here that cast is made
    a cast to float64, so its own statements run in double and the comparison is to float64 round-off."""
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import synthetic
    F, dm, H, nl, dff, B, L = 20, 48, 6, 1, 20, 3, 7
    rng = np.random.RandomState(5)
    feats, ids, y = synthetic.make_batch(rng, B, L, F, n_pad=0)
    ipw = np.asarray(synthetic.load_ipw(), np.float32)
    n_params = R.layout(F, dm, nl, dff)[-1][2] + dm
    p0 = np.random.RandomState(6).uniform(-0.3, 0.3, n_params)
    r = R.train_step(p0, np.zeros_like(p0), (F, dm, H, nl, dff), feats, ids, y, ipw_list=ipw, rate=0.0)
    monkeypatch.setattr(torch.Tensor, "float", lambda self: self.double())
    p = torch.as_tensor(p0, dtype=torch.float64).clone().requires_grad_(True)
    scores = O.setrank_forward(p, F, dm, H, nl, dff, feats, ids)
    assert scores.dtype == torch.float64
    labels = torch.from_numpy(np.ascontiguousarray(np.transpose(y))).double()
    loss = O.softmax_loss(scores, labels, O.ipw_weights(y, ipw).double())
    (g,) = torch.autograd.grad(loss, p)
    np.testing.assert_allclose(r["scores"], scores.detach().numpy(), rtol=0, atol=1e-13)
    assert abs(r["loss"] - float(loss.detach())) <= 1e-13
    np.testing.assert_allclose(r["grads"], g.numpy(), rtol=1e-10, atol=1e-13 * float(np.abs(g.numpy()).max()))


def _cfg(m):
    shapes = dict(zip(m["param_keys"], m["param_shapes"]))
    dff, F = shapes["Encoder_layer.input_embedding.0.weight"]
    dm = shapes["Encoder_layer.input_embedding.2.weight"][0]
    nl = sum(1 for k in m["param_keys"] if k.endswith("mha.dense.weight"))
    return F, dm, 4, nl, dff


def test_restatement_reproduces_the_golden():
    d, m = load_golden("setrank_dropout_tiny")
    cfg = _cfg(m)
    assert cfg == (20, 32, 4, 2, 16) and (m["B"], m["L"]) == (4, 6) and float(d["rate"]) == 0.25
    assert [n for n, _, _ in R.layout(cfg[0], cfg[1], cfg[3], cfg[4])] == m["param_keys"]
    for t in range(m["n_steps"]):
        p = "s%d_" % t
        r = R.train_step(d[p + "pre_params"], d[p + "pre_adagrad"], cfg, d[p + "features"], d[p + "docids"], d[p + "labels"],
                         ipw_list=d["ipw_list"], rate=float(d["rate"]), seed=int(d["seed"]), step=int(d["steps"][t]),
                         lr=m["lr"], max_norm=m["max_gradient_norm"])
        np.testing.assert_allclose(r["scores"], d[p + "scores"], rtol=0, atol=1e-6)
        gref = d[p + "grads"]
        np.testing.assert_allclose(r["grads"], gref, rtol=1e-5, atol=1e-6 * float(np.abs(gref).max()))
        assert abs(r["loss"] - float(d[p + "loss"])) <= 1e-6
        # the masks matter: without them the recorded step is NOT reproduced
        r0 = R.train_step(d[p + "pre_params"], d[p + "pre_adagrad"], cfg, d[p + "features"], d[p + "docids"], d[p + "labels"],
                          ipw_list=d["ipw_list"], rate=0.0)
        assert float(np.abs(r0["scores"] - d[p + "scores"]).max()) > 1e-3


def test_header_declares_and_lib_binds_the_entries():
    from ultra_pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ultr_hip.h")).read()
    assert int(re.search(r"#define\s+ULTR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION
    assert re.search(r"\bint64_t ultr_setrank_dropout_workspace_bytes\(const ultr_setrank_desc\* c, int64_t n_rows\);", hdr)
    for fn in ("ultr_setrank_forward_dropout", "ultr_setrank_backward_dropout"):
        assert re.search(r"\bint %s\(const ultr_setrank_desc\* c,[^;]*const ultr_setrank_dropout\* dropout, void\* stream\);" % fn, hdr)
        assert fn in _lib.SIGNATURES
    assert "ultr_setrank_dropout_workspace_bytes" in _lib.SIGNATURES
    assert "SetRank.py:103-117, 141-153" in re.sub(r"\s*\n \*\s*", " ", hdr)
    body = re.search(r"typedef struct ultr_setrank_dropout \{(.*?)\} ultr_setrank_dropout;", hdr, re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*[,;]", body)
    assert fields == [f for f, _ in _lib.SetRankDropout._fields_] == ["rate", "seed", "step", "stream", "scratch", "scratch_bytes"]
    lib = _lib.load()
    desc = _lib.SetRankDesc(20, 48, 6, 1, 20, 0, 0)
    import ctypes
    assert lib.ultr_setrank_dropout_workspace_bytes(ctypes.byref(desc), 21) >= 21 * 48 * 4
    # the existing size functions do not know about dropout
    assert lib.ultr_setrank_workspace_bytes(ctypes.byref(desc), 21) > 0


def test_rate_hyper_parameter():
    from ultra_pytorch_amd import hip_ops
    from ultra_pytorch_amd.ranking_model.SetRank import SetRank
    torch.manual_seed(4321)
    m = SetRank("d_model=32,num_heads=4,num_layers=1,diff=16,rate=0.1", 20)
    assert m.shape.rate == pytest.approx(0.1) and m.training and m.dropout_seed == 4321 and m.dropout_step == 0
    for bad in ("rate=1.0", "rate=-0.1"):
        with pytest.raises(ValueError):
            SetRank("d_model=32,num_heads=4,num_layers=1,diff=16," + bad, 20)
    with pytest.raises(ValueError):
        hip_ops.SetRankShape(20, 32, 4, 1, 16, rate=1.5)
    with pytest.raises(ValueError):
        hip_ops.setrank_dropout(float("nan"), 0, 0)
    # rate changes neither the layout nor any size
    a, b = hip_ops.SetRankShape(20, 32, 4, 1, 16, rate=0.3), hip_ops.SetRankShape(20, 32, 4, 1, 16)
    assert a.layout() == b.layout() and a.saved_bytes(24) == b.saved_bytes(24) and a.workspace_bytes(24) == b.workspace_bytes(24)
    assert bytes(a.desc) == bytes(b.desc)
