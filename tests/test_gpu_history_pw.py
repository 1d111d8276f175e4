"""ultr_history_pw on the GPU, bit for bit against its numpy restatement (tests/history_pw_ref.py): the three packed segment widths
(8 / 16 / 32 lanes), the first unpacked length (33), the chunk boundary (64 / 65) and a list of three chunks (130: two carries),
with both all_positions values, on a table of distinct values - and every bad-argument code."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import history_pw_ref as R  # noqa: E402
from tests.hipref import dev  # noqa: E402

SHAPES = [(1, 1), (9, 7), (8, 10), (256, 10), (5, 32), (3, 33), (4, 64), (3, 65), (2, 130)]


def label_patterns(B, L, seed):
    """{name: labels [L, B]}: every pattern fills ALL lists of the batch (the seeded random one differs per list)."""
    rng = np.random.RandomState(seed)
    z = np.zeros((L, B), np.float32)
    pats = {"none": z.copy(), "all": np.ones((L, B), np.float32)}
    first, last = z.copy(), z.copy()
    first[0], last[L - 1] = 1.0, 1.0
    pats["first"], pats["last"] = first, last
    if L > 64:
        c = z.copy()
        c[63], c[64] = 1.0, 1.0  # the last position of chunk 0 and the first of chunk 1
        pats["63_and_64"] = c
    v = (rng.uniform(size=(L, B)) < 0.4).astype(np.float32)
    pats["values"] = np.where(v > 0, 2.0, -1.0).astype(np.float32)  # 2.0 is a click, -1.0 is not
    pats["random"] = (rng.uniform(size=(L, B)) < rng.uniform(0.05, 0.7, size=(1, B))).astype(np.float32)
    return pats


def run_kernel(labels, table, all_positions):
    from ultra_pytorch_amd import hip_ops
    L, B = labels.shape
    out = torch.full((B, L), -7.0, dtype=torch.float32, device="cuda")
    hip_ops.history_pw(dev(labels), dev(table), out, all_positions)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("B,L", SHAPES)
def test_matches_the_restatement_bit_for_bit(B, L):
    table = R.distinct_table(np.random.RandomState(100 * B + L), L)
    for name, labels in label_patterns(B, L, seed=B + 31 * L).items():
        for all_positions in (False, True):
            got = run_kernel(labels, table, all_positions)
            want = R.history_pw(labels, table, all_positions)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, all_positions)


def test_bad_arguments_launch_nothing():
    from ultra_pytorch_amd import _lib, hip_ops
    lib = _lib.load()
    B, L = 3, 5
    labels, table = dev(np.ones((L, B), np.float32)), dev(np.ones((L, L), np.float32))
    out = torch.full((B, L), -7.0, dtype=torch.float32, device="cuda")

    def call(**kw):
        a = _lib.HistoryPwArgs()
        a.labels, a.table, a.pw_out = labels.data_ptr(), table.data_ptr(), out.data_ptr()
        a.batch, a.list_size, a.all_positions = B, L, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.ultr_history_pw(ctypes.byref(a), hip_ops.raw_stream())

    assert lib.ultr_history_pw(None, hip_ops.raw_stream()) == -1
    for bad in (dict(labels=None), dict(table=None), dict(pw_out=None), dict(batch=0), dict(batch=-1), dict(list_size=0),
                dict(list_size=-3), dict(all_positions=2), dict(all_positions=-1)):
        assert call(**bad) == -1, bad  # ULTR_E_BADARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()
    assert call() == 0 and call(all_positions=1) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 1.0).all()
    with pytest.raises(ValueError):
        hip_ops.history_pw(labels, dev(np.ones((L, L + 1), np.float32)), out, False)
