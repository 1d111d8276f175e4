"""GPU box: what the Oracle propensity estimator costs per training call at config 2 (136 features, DNN [256, 256], list 10, batch
256, DeviceClickFeed on the shipped user-browsing click model): us per `algo.train(feed.get_batch(ds)[0])` of IPWrank with

    randomized   the shipped randomized_pbm table                       (the default path)
    oracle_pbm   the Oracle on the position-biased model                (its [L] table through the same argument: no other launch)
    oracle_ubm   the Oracle on the user-browsing model                  (ultr_history_pw in front of every step)

The three alternate in one process, each warmed, --rounds times --steps calls per leg (a leg lasts well over a second); the medians
and every leg are printed as one JSON line.  A second line times history_pw_kernel alone: back-to-back launches between two events.
Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ultra_pytorch_amd import hip_ops  # noqa: E402
from ultra_pytorch_amd.input_layer.device_click_feed import DeviceClickFeed  # noqa: E402
from ultra_pytorch_amd.utils import find_class  # noqa: E402

F, L, B = 136, 10, 256
DATA = os.path.join(ROOT, "ultra_pytorch_amd", "data")
UBM, PBM = "ubm_0.1_1_4_1.0.json", "pbm_0.1_1.0_4_1.0.json"


class DS:
    pass


def dataset(nq=2000):
    rng = np.random.RandomState(99)
    ds = DS()
    ds.feature_size = F
    ds.features = rng.uniform(-1, 1, size=(nq * L, F)).astype(np.float32)
    ds.dids = list(range(nq * L))
    ds.initial_list = np.arange(nq * L, dtype=np.int64).reshape(nq, L).tolist()
    rel = rng.randint(0, 5, size=(nq, L))
    rel[:, 0] = np.maximum(rel[:, 0], 1)
    ds.labels = rel.tolist()
    return ds


def oracle_json(tmp, model_file):
    path = os.path.join(tmp, "oracle_" + model_file)
    with open(path, "w") as f:
        json.dump({"click_model": json.load(open(os.path.join(DATA, model_file)))}, f)
    return path


def make(ds, hparams):
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.IPWrank", "learning_algorithm_hparams": hparams,
           "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=[256,256]",
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3, 5, 10]}
    algo = find_class(exp["learning_algorithm"])(ds, exp)
    return algo, DeviceClickFeed(algo, B, "click_model_json=./example/ClickModel/" + UBM, seed=1)


def leg(algo, feed, ds, n):
    t0 = time.perf_counter()
    for _ in range(n):
        algo.train(feed.get_batch(ds)[0])
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40000)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("oracle_pw_rate.py needs a GPU")
    ds = dataset()
    out = sys.stdout
    sys.stdout = open(os.devnull, "w")  # train() prints its loss line per call
    with tempfile.TemporaryDirectory() as tmp:
        otype = "propensity_estimator_type=ultra.utils.propensity_estimator.OraclePropensityEstimator,propensity_estimator_json="
        legs = {"randomized": make(ds, ""), "oracle_pbm": make(ds, otype + oracle_json(tmp, PBM)),
                "oracle_ubm": make(ds, otype + oracle_json(tmp, UBM))}
    for algo, feed in legs.values():
        leg(algo, feed, ds, args.warmup)
    us = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, (algo, feed) in legs.items():
            us[k].append(leg(algo, feed, ds, args.steps))
    sys.stdout = out
    med = {k: statistics.median(v) for k, v in us.items()}
    print(json.dumps({"shape": {"F": F, "hidden": [256, 256], "L": L, "B": B}, "steps_per_leg": args.steps, "rounds": args.rounds,
                      "us_per_train_call_median": med, "us_per_train_call_legs": us,
                      "oracle_ubm_minus_randomized_us": med["oracle_ubm"] - med["randomized"]}))
    # the weight launch alone
    algo, feed = legs["oracle_ubm"]
    labels = feed.get_batch(ds)[0]["labels"]
    table = torch.from_numpy(algo.propensity_estimator.weight_table(L)[1]).cuda()
    buf = torch.zeros(B, L, device="cuda")
    for _ in range(200):
        hip_ops.history_pw(labels, table, buf, False)
    n, e0, e1 = 5000, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        hip_ops.history_pw(labels, table, buf, False)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"kernel": "history_pw_kernel<16>", "B": B, "L": L, "launches": n,
                      "us_per_launch_back_to_back": 1e3 * e0.elapsed_time(e1) / n}))


if __name__ == "__main__":
    main()
