#!/usr/bin/env python3
"""Training-step time of PDGD against the IPW (softmax) and LambdaRank steps, at BASELINE config 2's shape (136-d, DNN[256,256],
B 256, L 10) and config 4's (700-d, DNN[512,256,128], B 256, L 50), with PBM-like click density (~30 % of positions clicked).

The engines of one shape live in one process and are timed in alternating blocks of --block steps (device events around each
block, steps queued back to back), so clock and thermal drift hit all alike.  Then the host online loop at config 2's shape:
StochasticOnlineSimulationFeed.get_batch (GPU scoring, Plackett-Luce draw, click simulation on the host) + PDGD.train, per batch
(feed-bound; reported, no target).  Then the device online loop (input_layer.DeviceStochasticOnlineSimulationFeed /
DeviceDeterministicOnlineSimulationFeed: pick, scoring forward, re-rank and clicks on the GPU) + PDGD.train at config 2's and
config 4's shapes, per batch: device events around --device-online batches queued back to back, one synchronise at the end.
Prints one JSON line.

    python tools/bench_pdgd.py [--blocks 20] [--block 50] [--warmup 200] [--online 20] [--device-online 200]
                               [--out profiles/pdgd_bench.json]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cfg2": (136, [256, 256], 256, 10), "cfg4": (700, [512, 256, 128], 256, 50)}


def time_shape(F, hidden, B, L, args):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    feats, ids, _ = synthetic.make_batch(rng, B, L, F)
    clicks = (rng.uniform(size=(L, B)) < 0.3).astype(np.float32)
    f, i, yy = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev), torch.tensor(clicks, device=dev)
    ipw = torch.tensor(synthetic.load_ipw(), dtype=torch.float32, device=dev)
    shape = hip_ops.DnnShape(F, hidden, "elu")
    p0 = O.init_params(F, hidden, seed=2)
    runs = {}
    for algo in ("softmax", "lambdarank", "pdgd"):
        kw = dict(l2_loss=0.005, max_gradient_norm=1.0, cutoff=L) if algo == "pdgd" else {}
        eng = engine.StepEngine(shape, B, L, dev, algo=algo, **kw)
        p, st = torch.tensor(p0, device=dev), torch.zeros(p0.shape[0], device=dev)
        aux = torch.ones(2 * L, device=dev) if algo == "lambdarank" else None

        def step(eng=eng, p=p, st=st, aux=aux):
            eng.train_step(p, st, f, feats.shape[0], i, yy, aux=aux, ipw_table=ipw)

        runs[algo] = (eng, step)
    for eng, step in runs.values():
        for _ in range(args.warmup):
            step()
        eng.read_loss()
    torch.cuda.synchronize()
    times = {a: [] for a in runs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.blocks):
        for algo, (eng, step) in runs.items():
            e0.record()
            for _ in range(args.block):
                step()
            e1.record()
            e1.synchronize()
            times[algo].append(1e3 * e0.elapsed_time(e1) / args.block)
    res = {"shape": dict(F=F, hidden=hidden, B=B, L=L)}
    for a, t in times.items():
        res[a + "_step_us"] = dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))
    res["pdgd_over_lambdarank"] = res["pdgd_step_us"]["median"] / res["lambdarank_step_us"]["median"]
    res["pdgd_over_ipw"] = res["pdgd_step_us"]["median"] / res["softmax_step_us"]["median"]
    for eng, _ in runs.values():
        eng.close()
    return res


class _DS:
    def __init__(self, n_queries, L, F, seed):
        rng = np.random.RandomState(seed)
        self.feature_size = F
        self.features = rng.uniform(-1, 1, size=(n_queries * L, F)).astype(np.float32)
        self.initial_list = [list(range(q * L, (q + 1) * L)) for q in range(n_queries)]
        self.labels = [[int(v) for v in rng.randint(0, 5, size=L)] for _ in range(n_queries)]
        self.rank_list_size = L


def time_online(n_batches):
    from ultra_pytorch_amd.input_layer import StochasticOnlineSimulationFeed
    from ultra_pytorch_amd.utils import find_class
    F, hidden, B, L = SHAPES["cfg2"]
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.PDGD", "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=%s" % json.dumps(hidden),
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3]}
    ds = _DS(2000, L, F, 0)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        algo = find_class(exp["learning_algorithm"])(ds, exp)
        feed = StochasticOnlineSimulationFeed(algo, B, "")
        random.seed(0)
        np.random.seed(0)
        tf = ts = 0.0
        for t in range(n_batches + 2):
            t0 = time.perf_counter()
            f, _ = feed.get_batch(ds, check_validation=True)
            t1 = time.perf_counter()
            algo.train(f)
            t2 = time.perf_counter()
            if t >= 2:
                tf, ts = tf + (t1 - t0), ts + (t2 - t1)
    return {"online_batches": n_batches, "feed_ms": 1e3 * tf / n_batches, "train_ms": 1e3 * ts / n_batches,
            "batch_ms": 1e3 * (tf + ts) / n_batches}


def time_device_online(name, n_batches, mode, warmup=20):
    from ultra_pytorch_amd import input_layer
    from ultra_pytorch_amd.utils import find_class
    F, hidden, B, L = SHAPES[name]
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm.PDGD", "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=%s" % json.dumps(hidden),
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3]}
    ds = _DS(2000, L, F, 0)
    import contextlib
    import io
    cls = input_layer.DeviceStochasticOnlineSimulationFeed if mode == "stochastic" else input_layer.DeviceDeterministicOnlineSimulationFeed
    with contextlib.redirect_stdout(io.StringIO()):
        algo = find_class(exp["learning_algorithm"])(ds, exp)
        feed = cls(algo, B, "", seed=0)
        for _ in range(warmup):
            algo.train(feed.get_batch(ds, check_validation=True)[0])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        losses = []
        for _ in range(n_batches):
            f, _ = feed.get_batch(ds, check_validation=True)
            losses.append(algo.train(f)[0])
        e1.record()
        e1.synchronize()
        wall = time.perf_counter() - t0
    return {"batches": n_batches, "mode": mode, "batch_ms": e0.elapsed_time(e1) / n_batches, "wall_batch_ms": 1e3 * wall / n_batches,
            "finite_losses": bool(np.all(np.isfinite(losses)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--online", type=int, default=20)
    ap.add_argument("--device-online", type=int, default=200)
    ap.add_argument("--shapes", default="cfg2,cfg4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "blocks": args.blocks, "block_steps": args.block, "warmup": args.warmup}
    for name in args.shapes.split(","):
        res[name] = time_shape(*SHAPES[name], args)
    if args.online > 0:
        res["online_cfg2"] = time_online(args.online)
    if args.device_online > 0:
        for name in args.shapes.split(","):
            for mode in ("stochastic", "deterministic"):
                res["device_online_%s_%s" % (name, mode)] = time_device_online(name, args.device_online, mode)
        if "online_cfg2" in res and "device_online_cfg2_stochastic" in res:
            res["device_online_speedup_cfg2"] = res["online_cfg2"]["batch_ms"] / res["device_online_cfg2_stochastic"]["batch_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
