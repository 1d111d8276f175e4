#!/usr/bin/env python3
"""Training-step time of DBGD (one candidate), MGD and NSGD (four candidates each) against PDGD's step, at BASELINE config 2's shape (136-d,
DNN[256,256], B 256, M 10) and the reference's online example's model (136-d, DNN[512,256,128], B 256, M 10), with the default
'Stochastic' multileave and PBM clicks.

The four engines of one shape live in one process and are timed in alternating blocks of --block steps (device events around each
block, steps queued back to back), so clock and thermal drift hit all alike.  Then the device online loop
(input_layer.DeviceStochasticOnlineSimulationFeed get_batch + DBGD.train / MGD.train / NSGD.train) per batch: device events around --online batches,
one synchronise at the end.  Prints one JSON line.

    python tools/bench_dbgd.py [--blocks 20] [--block 50] [--warmup 100] [--online 200] [--out profiles/dbgd_bench.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cfg2": (136, [256, 256], 256, 10), "online_example": (136, [512, 256, 128], 256, 10)}


def _click_tables(dev):
    from ultra_pytorch_amd.utils import click_models
    desc = json.load(open(os.path.join(ROOT, "ultra_pytorch_amd", "data", "pbm_0.1_1.0_4_1.0.json")))
    hm = click_models.loadModelFromJson(desc)
    return (torch.tensor(hm.exam_prob, dtype=torch.float32, device=dev), len(hm.exam_prob),
            torch.tensor(desc["click_prob"], dtype=torch.float32, device=dev))


def time_shape(F, hidden, B, L, args):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    feats, ids, _ = synthetic.make_batch(rng, B, L, F)
    clicks = (rng.uniform(size=(L, B)) < 0.3).astype(np.float32)
    f, i, yy = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev), torch.tensor(clicks, device=dev)
    shape = hip_ops.DnnShape(F, hidden, "elu")
    p0 = O.init_params(F, hidden, seed=2)
    exam, n_exam, cprob = _click_tables(dev)
    runs = {}
    for name, R in (("pdgd", None), ("dbgd", 1), ("mgd", 4), ("nsgd", 4)):
        p, st = torch.tensor(p0, device=dev), torch.zeros(p0.shape[0], device=dev)
        if R is None:
            eng = engine.StepEngine(shape, B, L, dev, algo="pdgd", l2_loss=0.005, max_gradient_norm=1.0, cutoff=L)

            def step(eng=eng, p=p, st=st):
                eng.train_step(p, st, f, feats.shape[0], i, yy)
        else:
            # a small learning rate keeps the weights where the timed kernels run at any step count
            cls = engine.NsgdEngine if name == "nsgd" else engine.DbgdEngine
            eng = cls(shape, B, L, L, R, dev, noise_rate=0.01, learning_rate=0.01, click_model=0, exam=exam, n_exam=n_exam,
                      cprob=cprob, seed=1)

            def step(eng=eng, p=p, st=st):
                eng.train_step(p, st, f, feats.shape[0], i, yy)
        runs[name] = (eng, step)
    for eng, step in runs.values():
        for _ in range(args.warmup):
            step()
        eng.read_loss()
    torch.cuda.synchronize()
    times = {a: [] for a in runs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.blocks):
        for name, (eng, step) in runs.items():
            e0.record()
            for _ in range(args.block):
                step()
            e1.record()
            e1.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / args.block)
    res = {"shape": dict(F=F, hidden=hidden, B=B, M=L)}
    for a, t in times.items():
        res[a + "_step_us"] = dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))
    res["dbgd_over_pdgd"] = res["dbgd_step_us"]["median"] / res["pdgd_step_us"]["median"]
    res["mgd_over_pdgd"] = res["mgd_step_us"]["median"] / res["pdgd_step_us"]["median"]
    res["nsgd_minus_mgd_us"] = res["nsgd_step_us"]["median"] - res["mgd_step_us"]["median"]
    return res


class _DS:
    def __init__(self, n_queries, L, F, seed):
        rng = np.random.RandomState(seed)
        self.feature_size = F
        self.features = rng.uniform(-1, 1, size=(n_queries * L, F)).astype(np.float32)
        self.initial_list = [list(range(q * L, (q + 1) * L)) for q in range(n_queries)]
        self.labels = [[int(v) for v in rng.randint(0, 5, size=L)] for _ in range(n_queries)]
        self.rank_list_size = L


def time_device_online(name, algo_name, n_batches, warmup=20):
    from ultra_pytorch_amd import input_layer
    from ultra_pytorch_amd.utils import find_class
    F, hidden, B, L = SHAPES[name]
    exp = {"learning_algorithm": "ultra_pytorch_amd.learning_algorithm." + algo_name, "learning_algorithm_hparams": "",
           "ranking_model": "ultra_pytorch_amd.ranking_model.DNN", "ranking_model_hparams": "hidden_layer_sizes=%s" % json.dumps(hidden),
           "max_candidate_num": L, "selection_bias_cutoff": L, "metrics": ["ndcg"], "metrics_topn": [1, 3]}
    ds = _DS(2000, L, F, 0)
    with contextlib.redirect_stdout(io.StringIO()):
        algo = find_class(exp["learning_algorithm"])(ds, exp)
        feed = input_layer.DeviceStochasticOnlineSimulationFeed(algo, B, "", seed=0)
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
    return {"algo": algo_name, "batches": n_batches, "batch_ms": e0.elapsed_time(e1) / n_batches, "wall_batch_ms": 1e3 * wall / n_batches,
            "finite_losses": bool(np.all(np.isfinite(losses)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--online", type=int, default=200)
    ap.add_argument("--shapes", default="cfg2,online_example")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "blocks": args.blocks, "block_steps": args.block, "warmup": args.warmup}
    for name in args.shapes.split(","):
        res[name] = time_shape(*SHAPES[name], args)
    if args.online > 0:
        for name in args.shapes.split(","):
            for algo_name in ("PDGD", "DBGD", "MGD", "NSGD"):
                res["device_online_%s_%s" % (name, algo_name.lower())] = time_device_online(name, algo_name, args.online)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
