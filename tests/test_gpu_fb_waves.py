"""dnn_fb_kernel on 16 waves per workgroup (ULTR_FB_NW=16: one row per wave in the row-wise phases, one 16-column tile per wave in
the products) against the 8-wave build and against the oracle, through the ONE-call product step (engine.StepEngine.train_step).

Bitwise: rows, lanes, wave reductions and the k-order of every output element are the same in both builds; the one fold whose
association could change - rows w and w + 8 of a workgroup's column / loss partials, which one 8-wave wave adds in registers - is
redone in that order by the 16-wave `finalize` from the operands waves 8..15 leave.  So every output is compared with
np.array_equal: scores, the whole gradient vector with its tail, loss, norm, parameters and Adagrad state after the update.
Parity: the 16-wave step against oracle.ultr_oracle.train_step_softmax at the bars of tests/test_gpu_knobs.py (1e-5).
The planner ultr_fused_fb_waves (host-only) says which build a shape takes; its own test needs no GPU.
Reference: DNN.py:58-88, base_algorithm.py:118-154, ipw_rank.py:102-182."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

# name: (F, hidden, B, L, padded positions per list, per-entry weights instead of the table, waves under ULTR_FB_NW=16: 0 = the step does not take
# the fused kernel)
CASES = {
    "L10_B3_F136": (136, [256, 256], 3, 10, 0, False, 16),      # rows 10..15 dead; layer-0 contraction padded 136 -> 160
    "L16_B2": (136, [256, 256], 2, 16, 0, False, 16),           # all 16 rows live: waves 10..15 own real rows
    "L5_B4": (136, [256, 256], 4, 5, 0, False, 16),             # three lists per workgroup (loss on waves 0..2), last workgroup: one list
    "L3_B7": (136, [256, 256], 7, 3, 0, False, 16),             # five lists per workgroup, 15 live rows, last workgroup partial
    "F100": (100, [256, 256], 3, 10, 0, False, 16),             # layer-0 padding 100 -> 128
    "one_hidden": (136, [256], 3, 10, 0, False, 16),            # layer loops at 2 layers
    # ... and at 4: five 16 x 260 activation tiles + du + planes + the parameter image are 129 KB, 16 column-partial rows of 768 floats
    # 48 KB more - past the 160 KB of LDS, so the planner keeps the 8-wave build (8 rows: 153 KB)
    "three_hidden": (136, [256, 256, 256], 3, 10, 0, False, 8),
    "padded_docs": (136, [256, 256], 3, 10, 2, False, 16),      # doc ids equal to n_docs, as data_utils.pad leaves them
    "per_entry_pw": (136, [256, 256], 3, 10, 0, True, 16),      # `pw` [B, L] instead of the position table
    # fallbacks: tiles wider than 256 keep 8 waves.  [320, 256] is the widest kind the fused kernel holds in LDS; at [512, 256] its
    # tiles alone are past 160 KB and the step takes the separate kernels (planner 0) under either setting
    "maxdim320": (136, [320, 256], 3, 10, 0, False, 8),
    "maxdim512": (136, [512, 256], 3, 10, 0, False, 0),
}
LR = 0.05


def planned_waves(F, hidden, B, L):
    from ultra_pytorch_amd import _lib, hip_ops
    return _lib.load().ultr_fused_fb_waves(hip_ops.DnnShape(F, hidden, "elu").desc, B, L)


@pytest.fixture
def set_knobs(monkeypatch):
    from ultra_pytorch_amd import _lib

    def apply(**kv):
        for k, v in kv.items():
            monkeypatch.setenv(k, str(v))
        _lib.load().ultr_config_reload()
    yield apply
    monkeypatch.undo()
    _lib.load().ultr_config_reload()


_INPUTS, _STEPS, _ORACLE = {}, {}, {}


def inputs(name):
    if name not in _INPUTS:
        from oracle import ultr_oracle as O
        from ultra_pytorch_amd import synthetic
        F, hidden, B, L, n_pad, use_pw, _ = CASES[name]
        feats, ids, y = synthetic.make_batch(np.random.RandomState(5), B, L, F, n_pad=n_pad)
        y[0, :] = 1.0  # a click in every list (an all-zero list has weight 1e-7 everywhere: nothing to compare)
        params = O.init_params(F, hidden, seed=3)
        rng = np.random.RandomState(9)
        # gamma / beta away from their 1 / 0 initial values and a non-zero Adagrad state: every term of the backward carries weight
        params = (params + rng.normal(scale=0.05, size=params.shape)).astype(np.float32)
        state = rng.uniform(0.0, 0.01, size=params.shape).astype(np.float32)
        _INPUTS[name] = (feats, ids, y, params, state)
    return _INPUTS[name]


def oracle_step(name):
    if name not in _ORACLE:
        from oracle import ultr_oracle as O
        from ultra_pytorch_amd import synthetic
        F, hidden, B, L, n_pad, use_pw, _ = CASES[name]
        feats, ids, y, params, state = inputs(name)
        _ORACLE[name] = O.train_step_softmax(params, state, F, hidden, feats, ids, y, ipw_list=synthetic.load_ipw(), lr=LR)
    return _ORACLE[name]


def step(name, pw=None):
    """One product step; everything the step writes, as numpy."""
    from tests.hipref import dev
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    F, hidden, B, L, n_pad, use_pw, _ = CASES[name]
    feats, ids, y, params, state = inputs(name)
    shape = hip_ops.DnnShape(F, hidden, "elu")
    eng = engine.StepEngine(shape, B, L, torch.device("cuda"), algo="softmax", learning_rate=LR)
    p, st = dev(params), dev(state)
    tab = None if pw is not None else dev(np.asarray(synthetic.load_ipw(), np.float32))
    pwd = None if pw is None else dev(np.asarray(pw, np.float32))
    eng.train_step(p, st, dev(feats), feats.shape[0], dev(ids, torch.int32), dev(y, torch.float32), ipw_table=tab, pw=pwd)
    sc = eng.read_scalars()
    out = dict(scores=eng.scores.cpu().numpy(), raw_grads=eng.grads.cpu().numpy(), loss=np.float32(sc[0]), norm=np.float32(sc[1]),
               params=p.cpu().numpy(), state=st.cpu().numpy(), n=shape.n_params)
    eng.close()
    return out


def step_under(name, set_knobs, **knobs):
    key = (name,) + tuple(sorted(knobs.items()))
    if key not in _STEPS:
        set_knobs(**knobs)
        F, hidden, B, L, n_pad, use_pw, _ = CASES[name]
        nw = planned_waves(F, hidden, B, L)
        r = step(name, pw=oracle_step(name)["pw"] if use_pw else None)
        r["waves"] = nw
        _STEPS[key] = r
    return _STEPS[key]


def assert_same_bits(a, b):
    for k in ("scores", "raw_grads", "params", "state"):
        assert np.array_equal(a[k], b[k]), "%s differs: %d of %d entries, max |diff| %.3e" % (
            k, int((a[k] != b[k]).sum()), a[k].size, float(np.abs(a[k].astype(np.float64) - b[k]).max()))
    assert np.array_equal(a["loss"], b["loss"]) and np.array_equal(a["norm"], b["norm"]), (a["loss"], b["loss"], a["norm"], b["norm"])


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_sixteen_waves_same_bits_as_eight(name, set_knobs):
    want = CASES[name][6]
    r8 = step_under(name, set_knobs, ULTR_FB_NW=8)
    r16 = step_under(name, set_knobs, ULTR_FB_NW=16)
    assert r8["waves"] == (8 if want else 0)
    assert r16["waves"] == want, "ultr_fused_fb_waves under ULTR_FB_NW=16: %d" % r16["waves"]
    assert_same_bits(r8, r16)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_sixteen_waves_match_oracle(name, set_knobs):
    r = step_under(name, set_knobs, ULTR_FB_NW=16)
    ref = oracle_step(name)
    n = r["n"]
    tail = r["raw_grads"][n:]
    g = r["raw_grads"][:n] * (1.0 / tail[1])
    print("%s: max |score diff| %.2e, loss %.7g / %.7g, norm %.7g / %.7g, grads max |diff| / max |g| %.2e"
          % (name, np.abs(r["scores"] - ref["scores"]).max(), r["loss"], ref["loss"], r["norm"], ref["norm"],
             np.abs(g - ref["grads"]).max() / np.abs(ref["grads"]).max()))
    np.testing.assert_allclose(r["scores"], ref["scores"], atol=1e-5)
    assert abs(float(r["loss"]) - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"]))
    assert abs(float(r["norm"]) - ref["norm"]) <= 1e-5 * ref["norm"]
    gref = ref["grads"]
    np.testing.assert_allclose(g, gref, rtol=1e-5, atol=1e-5 * float(np.abs(gref).max()))


@gpu
def test_fp32_products_keep_eight_waves(set_knobs):
    """ULTR_FB_H3=0 with ULTR_FB_NW=16: the fp32-product build has no 16-wave form."""
    name = "L10_B3_F136"
    r8 = step_under(name, set_knobs, ULTR_FB_H3=0, ULTR_FB_NW=8)
    r16 = step_under(name, set_knobs, ULTR_FB_H3=0, ULTR_FB_NW=16)
    assert r8["waves"] == 8 and r16["waves"] == 8
    assert_same_bits(r8, r16)


@gpu
def test_reference_fixture_on_sixteen_waves(set_knobs):
    from tests.test_gpu_knobs import product_step
    from tests.hipref import load_golden
    set_knobs(ULTR_FB_NW=16)
    d, m = load_golden("ipw_cfg2")
    assert planned_waves(m["F"], m["hidden"], m["B"], m["L"]) == 16
    r = product_step(m["F"], m["hidden"], m["B"], m["L"], "softmax", m["lr"], d["s0_pre_params"], d["s0_pre_adagrad"], d["s0_features"],
                     d["s0_docids"], d["s0_labels"], None, d["ipw_list"])
    np.testing.assert_allclose(r["scores"], d["s0_scores"], atol=1e-5, rtol=0)
    assert abs(r["loss"] - float(d["s0_loss"])) <= 1e-5 * max(1.0, abs(float(d["s0_loss"])))
    g = d["s0_grads"]
    np.testing.assert_allclose(r["grads"], g, rtol=1e-5, atol=1e-6 * float(np.abs(g).max()))
    assert abs(r["norm"] - float(d["s0_norm"])) <= 1e-5 * float(d["s0_norm"])
    sel = np.abs(g) > 1e-4 * np.abs(g).max()  # (Adagrad's first step is lr x sign(g): entries that are rounding noise excluded)
    np.testing.assert_allclose(r["params"][sel], d["s0_post_params"][sel], atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(r["state"], d["s0_post_adagrad"], rtol=2e-5, atol=2e-6 * float(d["s0_post_adagrad"].max()))


def test_planner_alone(set_knobs):
    """ultr_fused_fb_waves without a GPU: which shapes take the fused kernel, and on how many waves."""
    set_knobs(ULTR_FB_NW=16)
    for name, (F, hidden, B, L, n_pad, use_pw, want) in CASES.items():
        assert planned_waves(F, hidden, B, L) == want, name
    assert planned_waves(136, [256, 256], 256, 10) == 16   # the headline shape
    assert planned_waves(136, [256, 256], 3, 17) == 0      # a list longer than the 16-row tile
    set_knobs(ULTR_FB_NW=8)
    for name, (F, hidden, B, L, n_pad, use_pw, want) in CASES.items():
        assert planned_waves(F, hidden, B, L) == (8 if want else 0), name
    set_knobs(ULTR_FB_NW=16, ULTR_FB_H3=0)
    assert planned_waves(136, [256, 256], 3, 10) == 8      # fp32 products: 8 waves only
    set_knobs(ULTR_FB_NW=16, ULTR_FB_H3=1, ULTR_NO_FUSED_FB=1)
    assert planned_waves(136, [256, 256], 3, 10) == 0      # the separate kernels
