"""ultr_setrank_forward / ultr_setrank_backward keep no state between calls: a SetRank step computes the same bits whatever the
thread called between its forward and its backward (stage calls of other engines on other paths, calls that were refused), and
the ULTR_SR_* knobs are those of the last ultr_config_reload(): a step after a reload is the step of an engine that never saw the
earlier values."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.hipref import dev  # noqa: E402
from tests.test_gpu_setrank_dropout import KW, batch, init, make_engine  # noqa: E402

E_BADARG, E_WORKSPACE = -1, -3
N_STEPS = 3
SR_KNOBS = ("ULTR_SR_H3", "ULTR_SR_ATTN_H3", "ULTR_SR_ATTN_H3_MASK", "ULTR_SR_WG_H3", "ULTR_SR_BWD_FUSED", "ULTR_SR_BLOCK")
# (B, L, F, d_model, heads, layers, dff), dropout rate
FUSED = ((3, 100, 24, 256, 4, 1, 64), 0.0)     # the smallest of test_gpu_setrank.BWD_FUSED_SHAPES: every fused launch, both directions
SEPARATE = ((3, 37, 20, 48, 6, 1, 20), 0.0)    # d_model no multiple of 32: separate launches, general row kernels, PAD documents
DROPOUT = ((16, 10, 136, 64, 4, 2, 32), 0.1)   # a dropout step: separate launches, five mask sites, the extra scratch


@pytest.fixture
def default_knobs(monkeypatch):
    from ultra_pytorch_amd import _lib
    for name in SR_KNOBS:
        monkeypatch.delenv(name, raising=False)
    _lib.load().ultr_config_reload()
    yield monkeypatch
    monkeypatch.undo()
    _lib.load().ultr_config_reload()


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).reshape(-1).view(np.uint32).copy()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class Case:
    """One engine with its inputs; every instance of a case starts from the same values (and, with dropout, the same key)."""

    def __init__(self, case, params=None, state=None):
        from ultra_pytorch_amd import hip_ops
        (B, L, F, dm, H, nl, dff), rate = case
        self.B, self.L = B, L
        self.shape = hip_ops.SetRankShape(F, dm, H, nl, dff, rate=rate)
        self.eng = make_engine(self.shape, B, L, seed=31, step=0, **KW)
        feats, ids, y, ipw = batch(B, L, F)
        self.feats, self.n_docs, self.ids, self.y, self.ipw = dev(feats), feats.shape[0], dev(ids, torch.int32), dev(y, torch.float32), dev(ipw)
        if params is None:
            p0 = init(self.shape)
            p0 += np.random.RandomState(3).normal(scale=0.02, size=p0.shape).astype(np.float32)  # LayerNorm parameters, biases off (1, 0)
            params, state = dev(p0), dev(np.zeros_like(p0))
        self.params, self.state = params.clone(), state.clone()

    def forward(self):
        self.eng.forward(self.params, self.feats, self.n_docs, self.ids, train=True)

    def loss_backward(self):
        self.eng.loss(self.y, ipw_table=self.ipw)
        self.eng.backward(self.params, self.feats, self.n_docs, self.ids)

    def update(self):
        e = self.eng
        e.update(self.params, self.state)
        torch.cuda.synchronize()
        return dict(scores=bits(e.scores), grads=bits(e.grads), params=bits(self.params), state=bits(self.state), scalars=bits(e.scalars))

    def step(self):
        self.forward()
        self.loss_backward()
        return self.update()

    def refused_backward(self, short_scratch):
        """A backward of this engine that the library refuses before it launches anything: dscores = NULL (ULTR_E_BADARG), or a
        dropout step whose scratch is one float short (ULTR_E_WORKSPACE)."""
        from ultra_pytorch_amd import hip_ops
        e, sh, lib = self.eng, self.shape, self.shape.lib
        st, n_parts = ctypes.c_void_p(hip_ops.raw_stream()), hip_ops.loss_part_count(self.B)
        if not short_scratch:
            return lib.ultr_setrank_backward(ctypes.byref(sh.desc), ptr(self.params), self.B, self.L, ptr(e.saved), None, ptr(e.loss_ws),
                                             n_parts, ptr(e.sr_ws), ptr(e.grads), st)
        d = hip_ops.setrank_dropout(sh.rate, sh.dropout_seed, 0, 0, e.drop_ws)
        assert d.scratch_bytes == sh.dropout_workspace_bytes(self.B * self.L)
        d.scratch_bytes -= 4
        return lib.ultr_setrank_backward_dropout(ctypes.byref(sh.desc), ptr(self.params), self.B, self.L, ptr(e.saved), ptr(e.dscores),
                                                 ptr(e.loss_ws), n_parts, ptr(e.sr_ws), ptr(e.grads), ctypes.byref(d), st)


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(a[key], b[key]), "%s: step %d, %s differs" % (what, k, key)


def test_a_step_does_not_depend_on_calls_between_its_forward_and_backward(default_knobs):
    cases = dict(fused=FUSED, separate=SEPARATE, dropout=DROPOUT)
    ref = {}
    for name, case in cases.items():
        alone = Case(case)
        ref[name] = [alone.step() for _ in range(N_STEPS)]
        alone.eng.close()
    for name in ref:  # the steps do something: finite, moving parameters
        assert np.isfinite(ref[name][-1]["grads"].view(np.float32)).all()
        assert not np.array_equal(ref[name][0]["params"], ref[name][-1]["params"])

    a, b, c = Case(FUSED), Case(SEPARATE), Case(DROPOUT)
    got = dict(fused=[], separate=[], dropout=[])
    for k in range(N_STEPS):
        if k > 0:
            assert a.refused_backward(short_scratch=False) == E_BADARG
            assert c.refused_backward(short_scratch=True) == E_WORKSPACE
        a.forward()
        b.forward()
        c.forward()
        b.loss_backward()
        a.loss_backward()
        c.loss_backward()
        got["fused"].append(a.update())
        got["separate"].append(b.update())
        got["dropout"].append(c.update())
    for name in cases:
        same(got[name], ref[name], name + " engine between the other engines' calls")
    for x in (a, b, c):
        x.eng.close()


def test_knobs_are_those_of_the_last_reload(default_knobs):
    from ultra_pytorch_amd import _lib
    lib = _lib.load()
    a = Case(FUSED)
    first = a.step()
    p1, s1 = a.params.clone(), a.state.clone()
    default = Case(FUSED, p1, s1)  # the second step under the default knobs: what the flipped step must NOT be
    second_default = default.step()
    default_knobs.setenv("ULTR_SR_BLOCK", "0")
    default_knobs.setenv("ULTR_SR_BWD_FUSED", "0")
    lib.ultr_config_reload()
    second = a.step()
    fresh = Case(FUSED, p1, s1)  # never ran under the default knobs
    want = fresh.step()
    same([second], [want], "the step after the reload")
    assert not np.array_equal(first["params"], second["params"])
    assert not np.array_equal(second["grads"], second_default["grads"]), "the separate launches sum in another order: the knobs did nothing?"
    for x in (a, default, fresh):
        x.eng.close()
