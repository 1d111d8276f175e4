"""ultr_train_step / ultr_feed_train_step keep no state between calls: a step computes the same bits whatever the thread called
since the previous step (stage calls of another engine, a whole step of another engine, a step that was rejected), and a feed
step that was rejected leaves no draw behind for a later step's update launch to pick up."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.hipref import dev  # noqa: E402

E_BADARG = -1
N_STEPS = 3


@pytest.fixture
def wide_whenever_legal(monkeypatch):
    """ULTR_FWD_WIDE=2, as tests/test_gpu_wide_tiles.py sets it for the wide-tile kernels"""
    from ultra_pytorch_amd import _lib
    monkeypatch.setenv("ULTR_FWD_WIDE", "2")
    _lib.load().ultr_config_reload()
    yield
    monkeypatch.undo()
    _lib.load().ultr_config_reload()


def bits(t):
    a = t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32).copy()


class Case:
    """One engine with its inputs; every instance starts from the same initial values."""

    def __init__(self, algo, F, hidden, B, L, act, feats, ids, y, p0, aux0=None):
        from ultra_pytorch_amd import engine, hip_ops, synthetic
        self.shape = hip_ops.DnnShape(F, hidden, act)
        self.eng = engine.StepEngine(self.shape, B, L, torch.device("cuda"), algo=algo, learning_rate=0.05, max_gradient_norm=5.0)
        self.feats, self.n_docs, self.ids, self.y = dev(feats), feats.shape[0], dev(ids, torch.int32), dev(y)
        self.params = dev(p0.copy())
        self.state = None if algo == "dla" else dev(np.zeros_like(p0))
        self.aux = None if aux0 is None else dev(aux0.copy())
        self.ipw = dev(np.asarray(synthetic.load_ipw(), np.float32)) if algo == "softmax" else None

    def record(self, loss=None):
        e = self.eng
        torch.cuda.synchronize()
        r = dict(params=bits(self.params), grads=bits(e.grads), scalars=bits(e.scalars), host=e._hs_u[:11].copy())
        if self.state is not None:
            r["state"] = bits(self.state)
        if self.aux is not None:
            r["aux"] = bits(self.aux)
        if loss is not None:
            r["loss"] = bits(np.asarray([loss], np.float32))
        return r

    def train_step(self):
        e = self.eng
        e.train_step(self.params, self.state, self.feats, self.n_docs, self.ids, self.y, aux=self.aux, ipw_table=self.ipw)
        loss = e.read_loss()
        e.read_scalars()
        return self.record(loss)

    def stages(self):
        e = self.eng
        e.forward(self.params, self.feats, self.n_docs, self.ids, train=True)
        e.loss(self.y, aux=self.aux, ipw_table=self.ipw)
        e.backward(self.params, self.feats, self.n_docs, self.ids)
        e.update(self.params, self.state, self.aux)
        return self.record()

    def rejected_step(self):
        """This engine's step with labels = NULL: a softmax step that ultr_train_step refuses before it launches anything"""
        from ultra_pytorch_amd import _lib, hip_ops
        bad = _lib.StepArgs.from_buffer_copy(self.eng._args)
        bad.labels = None
        return self.shape.lib.ultr_train_step(ctypes.byref(bad), hip_ops.raw_stream())


def make_a():
    from ultra_pytorch_amd import hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model import init_flat_params
    B, L, F, hidden = 9, 1, 8, [8]  # the smallest shape of test_fused_forward_backward_step: the fused forward+loss+backward launch
    feats, ids, y = synthetic.make_batch(np.random.RandomState(5), B, L, F)
    return Case("softmax", F, hidden, B, L, "elu", feats, ids, y, init_flat_params(hip_ops.DnnShape(F, hidden, "elu"), seed=3).numpy())


def wide_shape_name():
    """The smallest shape (rows x weights) of tests/test_gpu_wide_tiles.py that takes the wide-tile backward"""
    from tests.test_gpu_wide_tiles import SHAPES, backward_tile_rows

    def work(name):
        F, hidden, B, L, act, n_pad = SHAPES[name]
        dims = [F] + list(hidden)
        return B * L * sum(a * b for a, b in zip(dims[:-1], dims[1:]))

    def wide(name):
        F, hidden, B, L, act, n_pad = SHAPES[name]
        return backward_tile_rows(F, hidden, act, B * L) > 1000
    return min(filter(wide, SHAPES), key=work)


def make_a2():
    from tests.test_gpu_wide_tiles import SHAPES, backward_tile_rows, inputs
    name = wide_shape_name()
    F, hidden, B, L, act, n_pad = SHAPES[name]
    assert backward_tile_rows(F, hidden, act, B * L) > 1000
    feats, ids, y, params = inputs(name)
    return Case("softmax", F, hidden, B, L, act, feats, ids, y, params)


def make_b():
    from ultra_pytorch_amd import hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model import init_flat_params
    B, L, F, hidden = 37, 7, 24, [16, 8]  # separate kernels: the weight-gradient launch carries the early loss report
    rng = np.random.RandomState(7)
    feats, ids, y = synthetic.make_batch(rng, B, L, F, n_pad=2)
    aux = rng.normal(scale=0.2, size=L + 1).astype(np.float32)
    return Case("dla", F, hidden, B, L, "elu", feats, ids, y, init_flat_params(hip_ops.DnnShape(F, hidden, "elu"), seed=4).numpy(), aux0=aux)


def same(a, b, what):
    assert len(a) == len(b), what
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra.keys() == rb.keys()
        for key in ra:
            assert np.array_equal(ra[key], rb[key]), "%s: record %d, %s differs" % (what, k, key)


@pytest.mark.parametrize("make", [make_a, make_a2], ids=["fused", "wide_backward"])
def test_a_step_does_not_depend_on_what_the_thread_called_between_steps(make, wide_whenever_legal):
    alone = make()
    ref = [alone.train_step() for _ in range(N_STEPS)]
    b_alone = make_b()
    b_ref = []
    for _ in range(N_STEPS - 1):
        b_ref += [b_alone.stages(), b_alone.train_step()]

    a, b = make(), make_b()
    got, b_got = [], []
    for k in range(N_STEPS):
        if k > 0:
            b_got += [b.stages(), b.train_step()]
            assert a.rejected_step() == E_BADARG
        got.append(a.train_step())
    same(got, ref, "the step between other calls")
    same(b_got, b_ref, "the other engine's calls")
    for c in (alone, b_alone, a, b):
        c.eng.close()


def test_a_rejected_feed_step_leaves_no_draw_behind():
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    a = make_a()
    B, L, F = a.eng.B, a.eng.L, 8
    rng = np.random.RandomState(2)
    nq, lmax = 40, 3  # a resident set of a few dozen queries, lists of 1 .. 3 documents padded with -1
    lens = rng.randint(1, lmax + 1, size=nq)
    lists = np.full((nq, lmax), -1, np.int32)
    n_docs = 0
    for q in range(nq):
        lists[q, :lens[q]] = np.arange(n_docs, n_docs + lens[q])
        n_docs += int(lens[q])
    labels = np.where(lists >= 0, rng.randint(0, 5, size=(nq, lmax)), 0).astype(np.float32)
    res = dict(lists=dev(lists), labels=dev(labels), exam=dev(np.asarray([1.0, 0.6, 0.3], np.float32)),
               cprob=dev(np.asarray([0.1, 0.3, 0.5, 0.7, 0.9], np.float32)))
    a.feats, a.n_docs = dev(rng.uniform(-1, 1, size=(n_docs, F)).astype(np.float32)), n_docs

    def click_args(step, docids, clicks, qidx):
        c = _lib.ClickArgs()
        c.lists, c.labels, c.n_queries, c.lmax, c.n_docs = res["lists"].data_ptr(), res["labels"].data_ptr(), nq, lmax, n_docs
        c.exam_prob, c.n_exam, c.click_prob, c.n_rel = res["exam"].data_ptr(), 3, res["cprob"].data_ptr(), 5
        c.click_model, c.seed, c.step, c.batch, c.list_size, c.max_tries = 0, 11, step, B, L, 20
        c.docids, c.clicks, c.query_idx = docids.data_ptr(), clicks.data_ptr(), qidx.data_ptr()
        return c

    def buffers():
        return (torch.full((L, B), -7, dtype=torch.int32, device="cuda"), torch.full((L, B), -3.0, dtype=torch.float32, device="cuda"),
                torch.full((B,), -7, dtype=torch.int32, device="cuda"))

    def untouched(bufs):
        torch.cuda.synchronize()
        return bool((bufs[0] == -7).all()) and bool((bufs[1] == -3.0).all()) and bool((bufs[2] == -7).all())

    # the batch of the step itself: drawn on the spot
    cur = buffers()
    assert lib.ultr_click_batch_args(ctypes.byref(click_args(0, *cur)), hip_ops.raw_stream()) == 0
    a.ids, a.y = cur[0], cur[1]
    a.train_step()  # (a valid step, no draw behind it: the engine's argument block now describes this step)
    nxt_bufs, ref_bufs = buffers(), buffers()
    nxt = click_args(1, *nxt_bufs)
    bad = _lib.StepArgs.from_buffer_copy(a.eng._args)
    bad.labels = None
    st = hip_ops.raw_stream()
    assert lib.ultr_feed_train_step(ctypes.byref(bad), ctypes.byref(nxt), st) == E_BADARG
    assert untouched(nxt_bufs)
    assert lib.ultr_train_step(a.eng._aref, st) == 0
    assert untouched(nxt_bufs)
    assert lib.ultr_feed_train_step(a.eng._aref, ctypes.byref(nxt), st) == 0
    assert lib.ultr_click_batch_args(ctypes.byref(click_args(1, *ref_bufs)), st) == 0
    assert not untouched(ref_bufs)
    for got, want in zip(nxt_bufs, ref_bufs):
        assert np.array_equal(bits(got), bits(want))
    a.eng.close()
