#!/usr/bin/env python3
"""Training-step time of PRSrank against LambdaRank at BASELINE config 4's shape (700-d, DNN[512,256,128], B 256, L 50).

Both engines live in one process and are timed in alternating blocks of --block steps (device events around each block,
steps queued back to back as a training loop queues them), so clock and thermal drift hit both alike.  Prints one JSON
line: per-algorithm median / min of the block means in microseconds, and the ratio PRS / LambdaRank.

    python tools/bench_prs.py [--blocks 20] [--block 50] [--warmup 200] [--out profiles/prs_vs_lambdarank_cfg4.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, HIDDEN, B, L = 700, [512, 256, 128], 256, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    dev = torch.device("cuda", 0)
    feats, ids, y = synthetic.make_batch(np.random.RandomState(0), B, L, F)
    f, i, yy = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev), torch.tensor(y, device=dev)
    ipw = torch.tensor(synthetic.load_ipw(), dtype=torch.float32, device=dev)
    shape = hip_ops.DnnShape(F, HIDDEN, "elu")
    p0 = O.init_params(F, HIDDEN, seed=2)
    runs = {}
    for algo in ("lambdarank", "prs"):
        eng = engine.StepEngine(shape, B, L, dev, algo=algo)
        p, st = torch.tensor(p0, device=dev), torch.zeros(p0.shape[0], device=dev)
        aux = torch.ones(2 * L, device=dev) if algo == "lambdarank" else None

        def step(eng=eng, p=p, st=st, aux=aux):
            eng.train_step(p, st, f, feats.shape[0], i, yy, aux=aux, ipw_table=ipw)

        runs[algo] = (eng, step)
    for algo, (eng, step) in runs.items():
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
    losses = {a: float(eng.read_loss()) for a, (eng, _) in runs.items()}
    res = {"shape": dict(F=F, hidden=HIDDEN, B=B, L=L), "blocks": args.blocks, "block_steps": args.block, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "last_loss": losses}
    for a, t in times.items():
        res[a + "_step_us"] = dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))
    res["prs_over_lambdarank"] = res["prs_step_us"]["median"] / res["lambdarank_step_us"]["median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")
    for eng, _ in runs.values():
        eng.close()


if __name__ == "__main__":
    main()
