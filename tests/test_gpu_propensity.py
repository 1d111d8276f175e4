"""ultr_propensity_count on the GPU: its click table integer for integer against the numpy restatement of the session law
(tests/propensity_ref.py), split into calls and repeated; the estimator on the golden dataset against the position-biased
model's true weights (6 sigma of the analytic count statistics) and against the table the reference's own loop produced from
10^7 sessions of Python's random stream (tests/golden/propensity_ref.npz, 6 sqrt(2) sigma: two independent estimates); the error
codes; and the command line end to end into an IPWrank step."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import propensity_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "ultra_pytorch_amd", "data")
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODELS = {"pbm": ("pbm_0.1_1.0_4_1.0.json", R.PBM), "cascade": ("cascade_0.1_1.0_4_1.0.json", R.CASCADE),
          "ubm": ("ubm_0.1_1_4_1.0.json", R.UBM)}
HI_SEED = 0x123456789ABCDEF0
N_SESSIONS = 4099  # no multiple of a segment, wave or workgroup share


def _desc(name):
    with open(os.path.join(DATA, name)) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def tables(model):
    """(exam float32 flat, n_exam, click_prob float32, model id) as the estimator uploads them."""
    d = _desc(MODELS[model][0])
    ep = d["exam_prob"]
    n = len(ep)
    if MODELS[model][1] == R.UBM:
        ep = [[(row[c] if c < len(row) else 0.0) for c in range(n)] for row in ep]
    return np.asarray(ep, np.float32).reshape(-1), n, np.asarray(d["click_prob"], np.float32), MODELS[model][1]


@functools.lru_cache(maxsize=None)
def dataset(lmax):
    """7 label lists of lengths 0, 1, lmax - 1, lmax and three in between; labels 0 .. 4 and one above n_rel - 1; the padding holds
    garbage the kernel must not read as a label of the list."""
    rng = np.random.RandomState(lmax)
    lengths = np.array([lmax, 0, 1, lmax - 1, (lmax + 1) // 2, 2, lmax], np.int32)
    labels = rng.randint(0, 5, size=(7, lmax)).astype(np.float32)
    labels[0, lmax // 2] = 6.0
    labels[np.arange(lmax)[None, :] >= lengths[:, None]] = 4.0
    return labels, lengths


@functools.lru_cache(maxsize=None)
def expected(model, lmax, first_session):
    labels, lengths = dataset(lmax)
    exam, n_exam, cprob, mid = tables(model)
    return R.click_count(labels, lengths, exam, n_exam, cprob, mid, HI_SEED, first_session, N_SESSIONS)


def device_count(model, lmax, calls, seed=HI_SEED):
    """The table after the calls [(first_session, n_sessions), ...] into one zeroed table."""
    from ultra_pytorch_amd import hip_ops
    labels, lengths = dataset(lmax)
    exam, n_exam, cprob, mid = tables(model)
    dev = torch.device("cuda")
    dl, dn = torch.from_numpy(labels).to(dev), torch.from_numpy(lengths).to(dev)
    de, dc = torch.from_numpy(exam).to(dev), torch.from_numpy(cprob).to(dev)
    table = torch.zeros(lmax, lmax, dtype=torch.int64, device=dev)
    for first, n in calls:
        hip_ops.propensity_count(dl, dn, de, n_exam, dc, mid, seed, first, n, table)
    torch.cuda.synchronize()
    return table.cpu().numpy()


@pytest.mark.parametrize("first_session", [0, 2 ** 32 - 5])
@pytest.mark.parametrize("lmax", [5, 12, 24, 70])  # segments of 8, 16 and 32 lanes, and one wavefront per session
@pytest.mark.parametrize("model", ["pbm", "cascade", "ubm"])
def test_click_count_is_exact(model, lmax, first_session):
    want = expected(model, lmax, first_session)
    got = device_count(model, lmax, [(first_session, N_SESSIONS)])
    assert want.sum() > 0 and want[lmax - 1].sum() > 0 and want[0, 0] > 0
    if model == "cascade":
        assert want.sum() <= N_SESSIONS
    print("clicks", int(want.sum()), "differing cells", int((got != want).sum()))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("lmax", [5, 70])
@pytest.mark.parametrize("model", ["pbm", "cascade", "ubm"])
def test_calls_add_up(model, lmax):
    first = 2 ** 32 - 5
    want = expected(model, lmax, first)
    parts = device_count(model, lmax, [(first, 1), (first + 1, 2048), (first + 2049, 2050)])
    assert np.array_equal(parts, want)
    twice = device_count(model, lmax, [(first, N_SESSIONS), (first, N_SESSIONS)])
    assert np.array_equal(twice, 2 * want)  # added to, never cleared


class GoldenData(object):
    def __init__(self):
        g = np.load(os.path.join(GOLDEN, "propensity_ref.npz"))
        self.lengths, self.padded = g["lengths"], g["labels"]
        self.labels = [[int(v) for v in row[:n]] for row, n in zip(g["labels"], g["lengths"])]
        self.rank_list_size = int(g["labels"].shape[1])
        self.ref_ipw, self.ref_sessions = g["IPW_list"], int(g["sessions"])


def _estimate(data, sessions):
    from ultra_pytorch_amd.utils import click_models as CM
    from ultra_pytorch_amd.utils.propensity_estimator import RandomizedPropensityEstimator
    est = RandomizedPropensityEstimator()
    cm = CM.loadModelFromJson(_desc("pbm_0.1_1.0_4_1.0.json"))
    est.estimateParametersFromModel(cm, data, session_num=sessions, seed=0)
    assert est.click_model is cm and len(est.IPW_list) == data.rank_list_size
    assert est.click_count.dtype == np.int64 and est.click_count.shape == (data.rank_list_size,) * 2
    return est


def test_estimator_recovers_the_pbm_weights():
    data, d = GoldenData(), _desc("pbm_0.1_1.0_4_1.0.json")
    S = 1 << 20
    est = _estimate(data, S)
    assert est.IPW_list == R.ipw_formula(est.click_count)
    e_first, e_agg, true = R.pbm_expectation(data.padded, data.lengths, d["exam_prob"], d["click_prob"], S)
    bound = R.six_sigma(est.IPW_list, e_first, e_agg)
    print("|err| / bound", np.abs(np.asarray(est.IPW_list) - true) / bound)
    assert np.all(np.abs(np.asarray(est.IPW_list) - true) <= bound)


def test_estimator_matches_the_reference_table():
    """10^7 sessions here against the reference's 10^7: the length-indexed counting and the y >= x sums are the reference's."""
    data, d = GoldenData(), _desc("pbm_0.1_1.0_4_1.0.json")
    S = data.ref_sessions
    assert S == 10_000_000
    est = _estimate(data, S)
    assert est.IPW_list == R.ipw_formula(est.click_count)
    e_first, e_agg, _ = R.pbm_expectation(data.padded, data.lengths, d["exam_prob"], d["click_prob"], S)
    bound = np.sqrt(2.0) * R.six_sigma(est.IPW_list, e_first, e_agg)
    print("|diff| / bound", np.abs(np.asarray(est.IPW_list) - data.ref_ipw) / bound)
    assert np.all(np.abs(np.asarray(est.IPW_list) - data.ref_ipw) <= bound)


def test_errors_launch_nothing():
    from ultra_pytorch_amd import _lib, hip_ops
    from ultra_pytorch_amd.utils import click_models as CM
    from ultra_pytorch_amd.utils.propensity_estimator import RandomizedPropensityEstimator
    lib, dev = _lib.load(), torch.device("cuda")
    exam, n_exam, cprob, mid = tables("pbm")
    de, dc = torch.from_numpy(exam).to(dev), torch.from_numpy(cprob).to(dev)

    def args(lmax, table, n_sessions=64):
        a = _lib.PropensityArgs()
        labels = torch.ones(3, lmax, dtype=torch.float32, device=dev)
        lengths = torch.full((3,), lmax, dtype=torch.int32, device=dev)
        a.labels, a.lengths, a.n_queries, a.lmax = labels.data_ptr(), lengths.data_ptr(), 3, lmax
        a.exam_prob, a.n_exam, a.click_prob, a.n_rel, a.click_model = de.data_ptr(), n_exam, dc.data_ptr(), int(dc.numel()), mid
        a.seed, a.first_session, a.n_sessions = 1, 0, n_sessions
        a.click_count = None if table is None else table.data_ptr()
        return a, (labels, lengths)

    stream = ctypes.c_void_p(hip_ops.raw_stream())
    table = torch.zeros(8, 8, dtype=torch.int64, device=dev)
    a, keep = args(8, None)
    assert lib.ultr_propensity_count(ctypes.byref(a), stream) == -1          # null table
    a, keep = args(8, table, n_sessions=-1)
    assert lib.ultr_propensity_count(ctypes.byref(a), stream) == -1          # n_sessions < 0
    assert lib.ultr_propensity_count(None, stream) == -1
    too_long = _lib.PROPENSITY_MAX_L + 1
    big = torch.zeros(too_long, too_long, dtype=torch.int64, device=dev)
    a, keep = args(too_long, big)
    assert lib.ultr_propensity_count(ctypes.byref(a), stream) == -2          # lmax past the supported bound
    with pytest.raises(_lib.UltrHipError, match="unsupported shape"):
        hip_ops.propensity_count(keep[0], keep[1], de, n_exam, dc, mid, 1, 0, 64, big)
    a, keep = args(_lib.PROPENSITY_MAX_L, torch.zeros(_lib.PROPENSITY_MAX_L, _lib.PROPENSITY_MAX_L, dtype=torch.int64, device=dev), 0)
    assert lib.ultr_propensity_count(ctypes.byref(a), stream) == 0           # no sessions: a no-op at the bound itself
    torch.cuda.synchronize()
    assert int(table.sum()) == 0 and int(big.sum()) == 0

    class Data(object):
        rank_list_size, labels = 3, [[1, 0], [0, 1, 2, 3]]

    with pytest.raises(ValueError, match="longer than rank_list_size"):
        RandomizedPropensityEstimator().estimateParametersFromModel(CM.loadModelFromJson(_desc("pbm_0.1_1.0_4_1.0.json")), Data())


def test_longest_supported_list():
    """lmax = ULTR_PROPENSITY_MAX_L: the largest LDS histogram, two full chunks of 64 positions."""
    from ultra_pytorch_amd import _lib
    lmax = _lib.PROPENSITY_MAX_L
    labels, lengths = dataset(lmax)
    exam, n_exam, cprob, mid = tables("cascade")
    want = R.click_count(labels, lengths, exam, n_exam, cprob, mid, HI_SEED, 0, 515)
    assert np.array_equal(device_count("cascade", lmax, [(0, 515)]), want) and want[lmax - 1].sum() > 0


def test_command_line_end_to_end(tmp_path):
    from tests.test_gpu_plugins import build, make_feed
    from ultra_pytorch_amd.learning_algorithm.ipw_rank import load_ipw_list
    from ultra_pytorch_amd.utils import data_utils
    toy = os.path.join(GOLDEN, "ultra_toy_data") + "/"
    cm_json = os.path.join(DATA, "cascade_0.1_1.0_4_1.0.json")
    run = subprocess.run([sys.executable, "-m", "ultra_pytorch_amd.utils.propensity_estimator", cm_json, toy, str(tmp_path),
                          "--sessions", "200000", "--seed", "3"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = os.path.join(str(tmp_path), "randomized_cascade_0.1_1.0_4_1.0.json")
    assert os.listdir(str(tmp_path)) == [os.path.basename(out)]
    data = json.load(open(out))
    assert set(data) == {"click_model", "IPW_list"} and data["click_model"] == json.load(open(cm_json))
    train = data_utils.read_data(toy, "train")
    ipw = load_ipw_list(out)
    assert ipw == data["IPW_list"] and len(ipw) == train.rank_list_size and abs(ipw[0] - 1.0) < 1e-6 and all(np.isfinite(ipw))
    L, B, F = train.rank_list_size, 4, train.feature_size
    algo = build({"algo": "ipw", "hidden": [8], "L": L, "F": F, "algo_hparams": "propensity_estimator_json=%s" % out})
    assert list(algo.IPW_list) == ipw
    rng = np.random.RandomState(0)
    feats = rng.uniform(-1, 1, size=(B * L, F)).astype(np.float32)
    docids = np.arange(B * L, dtype=np.int32).reshape(B, L).T.copy()
    clicks = (rng.uniform(size=(L, B)) < 0.4).astype(np.float32)
    clicks[0] = 1.0
    loss = algo.train(make_feed(algo, feats, docids, clicks))[0]
    assert np.isfinite(float(loss))
