#!/usr/bin/env python3
"""Time one full evaluation pass over a synthetic validation set on the GPU, three ways:

  validation_set      BaseAlgorithm.validation_set with a DeviceDirectLabelFeed (one call, one host read: engine.EvalSetEngine)
  host_feed_loop      the driver's loop over DirectLabelFeed.get_next_batch + validation() + utils.merge_Summary (unchanged)
  device_feed_loop    the same loop over DeviceDirectLabelFeed.get_next_batch (one pick launch + validation() per batch)

at list size 10 and 100, 8192 queries, batch 256.  Every path is warmed up, then timed `--repeats` times with a host clock around a
pass that ends in a device synchronisation; the line per (list size, path) carries the median and the spread (min .. max).  The three
summaries of a list size are compared before anything is timed: validation_set must equal device_feed_loop exactly, the largest
difference to the host loop is recorded with every line.

    python tools/eval_set_rate.py [--out FILE.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class SyntheticSet:
    """n_queries lists of exactly L documents drawn from a pool of n_docs feature rows (a padded Raw_data look-alike)."""

    def __init__(self, n_queries, L, F, n_docs, seed):
        rng = np.random.RandomState(seed)
        self.feature_size, self.rank_list_size = F, L
        self.features = np.concatenate([rng.uniform(-1, 1, size=(n_docs, F)).astype(np.float32), np.zeros((1, F), np.float32)])
        self.dids = ["d%d" % i for i in range(n_docs)]
        self.qids = ["q%d" % q for q in range(n_queries)]
        self.initial_list = rng.randint(0, n_docs, size=(n_queries, L)).tolist()
        self.labels = rng.randint(0, 5, size=(n_queries, L)).tolist()


def loop(algo, feed, ds):
    from ultra_pytorch_amd.utils import merge_Summary
    it, summaries, sizes = 0, [], []
    while it < len(ds.initial_list):
        input_feed, info_map = feed.get_next_batch(it, ds, check_validation=False)
        _, _, summary = algo.validation(input_feed)
        summaries.append(copy.deepcopy(summary))
        sizes.append(len(info_map["input_list"]))
        it += sizes[-1]
    return merge_Summary(summaries, sizes)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lists", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3, help="the host-feed loop is slow: fewer timed passes")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_set_rate.py measures on the GPU: none found")
    from ultra_pytorch_amd import input_layer
    from ultra_pytorch_amd.utils import find_class
    from ultra_pytorch_amd.utils import metrics
    metrics.RankingMetricKey.MAX_LABEL = 4.0
    F, results = 136, []
    for L in args.lists:
        ds = SyntheticSet(args.queries, L, F, 65536, seed=L)
        exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.IPWrank", "learning_algorithm_hparams": "",
               "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=[512, 256, 128]",
               "max_candidate_num": L, "selection_bias_cutoff": min(10, L), "metrics": ["ndcg", "err"], "metrics_topn": [1, 3, 5, 10]}
        algo = find_class(exp["learning_algorithm"])(ds, exp)
        dfeed = input_layer.DeviceDirectLabelFeed(algo, args.batch, "")
        hfeed = input_layer.DirectLabelFeed(algo, args.batch, "")
        paths = [("validation_set", lambda: algo.validation_set(dfeed, ds)[0], args.repeats),
                 ("device_feed_loop", lambda: loop(algo, dfeed, ds), args.repeats),
                 ("host_feed_loop", lambda: loop(algo, hfeed, ds), args.host_repeats)]
        got = {name: fn() for name, fn, _ in paths}
        assert got["validation_set"] == got["device_feed_loop"], "validation_set differs from the per-batch loop"
        worst = max(abs(got["validation_set"][k] - got["host_feed_loop"][k]) for k in got["host_feed_loop"])
        for name, fn, reps in paths:
            t = timed(fn, args.warmup if name != "host_feed_loop" else 1, reps)
            r = {"list_size": L, "queries": args.queries, "batch": args.batch, "path": name, "passes": reps,
                 "median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t),
                 "queries_per_s": args.queries / statistics.median(t), "host_vs_device_max_metric_diff": worst}
            results.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
