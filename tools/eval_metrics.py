"""GPU box: validation() queries/s THROUGH THE PLUGIN API (IPWrank.validation on a device feed, the summary read on the host after
every batch) with config 2's model at list size 10 and at 100 candidates, for metrics = ["ndcg"], ["mrr", "ndcg"] and all eight.
Public API only: the same file measures an older checkout (its host path for the metrics its launch does not compute).
   python tools/eval_metrics.py [--root CHECKOUT] [--reps 3] [--batches 300] [--list-size L [L ...]] [--sets TAG [TAG ...]] [--host]
prints one JSON line: {"list_size_10": {"ndcg": [queries/s per repetition], ...}, "list_size_100": {...}}
--list-size: these list sizes instead (every list PAD-tailed at a random length >= L / 2), e.g. 900 1251 4096 for the long-list kernel
of the metric launch; a set whose validation() raises in the measured checkout reads "raises: ...".  --host: next to every set the
host alternative under "<tag>_host" - the forward alone, the scores, doc ids and labels copied, utils.metrics on the CPU (what
validation() does beyond ultr_metrics_max_list(), and all an older checkout has beyond its metric launch's list size)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to measure")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batches", type=int, default=300)
ap.add_argument("--list-size", type=int, nargs="+", default=None, help="list sizes to measure (default: config 2's 10, and 100)")
ap.add_argument("--sets", nargs="+", default=None, help="metric sets to measure: ndcg mrr_ndcg all_eight (default: all three)")
ap.add_argument("--host", action="store_true", help="also time the forward alone + utils.metrics on copied scores")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from ultra_pytorch_amd import hip_ops, synthetic  # noqa: E402
from ultra_pytorch_amd.utils import find_class, metrics  # noqa: E402

SETS = {"ndcg": ["ndcg"], "mrr_ndcg": ["mrr", "ndcg"],
        "all_eight": ["ndcg", "dcg", "mrr", "err", "map", "arp", "precision", "ordered_pair_accuracy"]}


class DataSet:
    def __init__(self, feature_size):
        self.feature_size = feature_size


def batches(cfg, L, device):
    """bench.py eval_leg's batches: at 100 candidates a random tail of every list is PAD."""
    F, B = cfg["F"], cfg["B"]
    rng, out = np.random.RandomState(77 + L), []
    for _ in range(4 if B * L <= 100000 else 2):  # (136 floats per document: two batches of 4096-document lists are 1.1 GB)
        feats, ids, y = synthetic.make_batch(rng, B, L, F, clicks=False)
        if L > cfg["L"]:
            lens = rng.randint(L // 2, L + 1, size=B)
            padm = np.arange(L)[:, None] >= lens[None, :]
            ids = np.where(padm, feats.shape[0], ids).astype(np.int32)
            y = np.where(padm, 0.0, y).astype(np.float32)
        out.append({"device_feed": True, "features": torch.from_numpy(feats).to(device), "n_docs": feats.shape[0],
                    "docids": torch.from_numpy(ids).to(device), "labels": torch.from_numpy(y).to(device), "batch_size": B})
    return out


def host_alternative(algo, feed, names, topn, scores):
    """The forward alone, then what a checkout without a metric launch for this list size does: copy, mask and utils.metrics on the CPU."""
    B, L = feed["batch_size"], feed["docids"].shape[0]
    hip_ops.dnn_forward(algo.model.shape, algo.model.flat_params, feed["features"], feed["n_docs"], feed["docids"], B, L, scores)
    pad = feed["docids"].t().cpu() == feed["n_docs"]
    masked = torch.where(pad, torch.full((), -100000.0), scores.cpu())
    lab = feed["labels"].t().contiguous().cpu()
    return {"%s_%d" % (m, n): float(v) for m in names for n, v in zip(topn, metrics.make_ranking_metric_fn(m, topn)(lab, masked, None))}


def main():
    cfg = bench.CONFIGS["2"]
    device = torch.device("cuda")
    metrics.RankingMetricKey.MAX_LABEL = 4.0
    result = {}
    sets = {tag: SETS[tag] for tag in (args.sets or SETS)}
    for L in (args.list_size or (cfg["L"], 100)):
        feeds = batches(cfg, L, device)
        algos = {}
        for tag, names in sets.items():
            exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.IPWrank", "learning_algorithm_hparams": "",
                   "ranking_model": "ultra_pytorch_amd.ranking_model.DNN",
                   "ranking_model_hparams": "hidden_layer_sizes=%s" % json.dumps(cfg["hidden"]),
                   "max_candidate_num": L, "selection_bias_cutoff": min(10, L), "metrics": names, "metrics_topn": [1, 3, 5, 10]}
            algos[tag] = find_class(exp["learning_algorithm"])(DataSet(cfg["F"]), exp)
        runs = {tag: (lambda feed, algo=algo: algo.validation(feed)[2]) for tag, algo in algos.items()}
        if args.host:
            scores = torch.empty(cfg["B"], L, device=device)
            for tag, algo in algos.items():
                runs[tag + "_host"] = lambda feed, algo=algo, tag=tag: host_alternative(algo, feed, sets[tag], [1, 3, 5, 10], scores)
        rates = {tag: [] for tag in runs}
        for rep in range(args.reps + 1):  # repetition 0 warms every shape up and is dropped; the sets alternate inside a repetition
            for tag, run in runs.items():
                if isinstance(rates[tag], str):
                    continue
                n = min(20, args.batches) if rep == 0 else args.batches
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    for i in range(n):
                        summary = run(feeds[i % len(feeds)])
                except Exception as e:  # an older checkout at a list size its launches do not take
                    if not args.list_size:
                        raise
                    rates[tag] = "raises: %s" % str(e)[:120]
                    continue
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / n
                if rep:
                    rates[tag].append(round(cfg["B"] / dt, 1))
                names = sets[tag[:-5] if tag.endswith("_host") else tag]
                assert all(np.isfinite(v) for v in summary.values()) and len(summary) == 4 * len(names)
        result["list_size_%d" % L] = rates
    print(json.dumps(result))


if __name__ == "__main__":
    main()
