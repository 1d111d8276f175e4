"""The metric launches' output bits, frozen: ultr_metrics_report, ultr_metrics_long, ultr_ndcg_report and ultr_ndcg (ndcg_list_kernel,
metrics_long_kernel and ndcg_mean_kernel, csrc/ultr_metrics.hip) against tests/golden/metrics_frozen.npz - the batch means, the
per-list block, the order, the masked scores and, where the launch writes one, the host report, as recorded by
tests/golden/make_metrics_frozen.py before the two kernels were given one ranking core.  The other metric tests hold the kernels to a
float64 restatement within a tolerance and to each other bit for bit; this one holds each of them to its own earlier bits, so a change
that moves both kernels together is seen too.

The fixture records this hardware's v_exp_f32 / v_log_f32 results from the library as build.py builds it (gfx950, -O3, no packed
fp32): a change that is MEANT to alter the arithmetic - another order of additions, another exp2 or log2 - regenerates it with
    python tests/golden/make_metrics_frozen.py
on the GPU and says so; anything else that fails here changed bits it should not have."""
import os

import numpy as np
import pytest

from tests.test_gpu_metrics import Ndcg
from tests.test_gpu_metrics_all import TOPN_4, TOPN_16, TOPN_ODD, Launch, _dev, make_inputs, nan_inputs, ndcg_report
from tests.test_gpu_metrics_long import LongLaunch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_frozen.npz")
N_DOCS, MAX_LABEL = 1000, 5.0
WHAT = ("means", "per_list", "order", "masked", "host_report")  # (ultr_ndcg_report as the tests call it and ultr_ndcg: the first four)

# one list of one document; a partial workgroup, one chunk short of full; 18 workgroups with a two-list last one, more lists than
# lanes in the batch means, two chunks; make_inputs' edge rows (B >= 8) and three chunks (the ERR carry crosses chunks twice)
SHAPES = [(1, 1, TOPN_4), (5, 63, TOPN_16), (70, 65, TOPN_4), (9, 129, TOPN_ODD)]
# (entry, B, L, topn, NaN scores with invalid labels)
CASES = [(entry, B, L, topn, False) for entry in ("report", "long", "ndcg_report") for B, L, topn in SHAPES]
CASES += [("ndcg", 5, 63, TOPN_16, False),      # the two launches: per-list values, then ndcg_mean_kernel
          ("long", 3, 814, TOPN_16, False),     # one past the routing threshold
          ("long", 3, 1025, TOPN_ODD, False),   # one past the long kernel's 1024 threads
          ("report", 8, 130, TOPN_4, True), ("long", 8, 130, TOPN_4, True)]


def case_id(case):
    entry, B, L, topn, nan = case
    return "%s_B%d_L%d_k%d%s" % (entry, B, L, len(topn), "_nan" if nan else "")


def _bits(a):
    """Floats as their uint32 views: NaNs compare, and -0 is not +0."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run_case(case):
    """{what: array} of one case's launch on seeded inputs."""
    entry, B, L, topn, nan = case
    s, y, ids = nan_inputs(B, L, True) if nan else make_inputs(B * 7 + L, B, L, N_DOCS)
    args = _dev(s, y, ids)
    if entry in ("report", "long"):
        k = (Launch if entry == "report" else LongLaunch)(B, L, topn, max_label=MAX_LABEL)
        got = k.run(*args, N_DOCS)
        assert not isinstance(got, int), "return code %r" % (got,)
        got = tuple(got) + (k.host.numpy().copy(),)
    elif entry == "ndcg_report":
        got = ndcg_report(*args, N_DOCS, B, L, topn)
    else:
        got = Ndcg(B, L, topn).run(*args, N_DOCS)
        assert not isinstance(got, int), "return code %r" % (got,)
    return {what: _bits(a) for what, a in zip(WHAT, got)}


@pytest.fixture(scope="module")
def frozen():
    with np.load(FIXTURE) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_metric_launch_bits_are_the_recorded_ones(case, frozen):
    got = run_case(case)
    want = {k.split("/", 1)[1]: v for k, v in frozen.items() if k.split("/", 1)[0] == case_id(case)}
    assert sorted(want) == sorted(got), "the fixture's arrays of this case"
    for what in got:
        assert got[what].dtype == want[what].dtype, what
        np.testing.assert_array_equal(got[what], want[what], err_msg="%s of %s" % (what, case_id(case)))
