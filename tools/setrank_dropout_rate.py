#!/usr/bin/env python3
"""Time SetRank training steps with and without dropout at BASELINE config 5's geometry (B = 1024, L = 100, F = 220, d_model 256,
8 heads, 2 layers, dff 64, fp16 attention operands), three cases in ONE process, interleaved:

  a  rate 0, default plan               the fused persistent launches (what bench.py --config 5 times)
  b  rate 0, separate launches          ULTR_SR_BLOCK=0 ULTR_SR_BWD_FUSED=0: the plan a dropout step builds on
  c  rate 0.1                           the dropout step (separate launches + the row kernels of csrc/ultr_sr_dropout.hip)

(c) is to be read against (b): the difference is what dropout itself costs; (b) against (a) is what leaving the fused launches costs.

The knobs are process-wide and read when an engine is built, so every timed block builds its own engine under its case's
environment.  A block is `--warmup` steps, a synchronisation, then `--steps` steps under a host clock that stops behind a device
synchronisation; the blocks run round-robin a b c a b c ... `--rounds` times (boxes drift by 1 - 3 %: compare inside one call).
One JSON line per case: median, min and max of its blocks in ms per step.

    python tools/setrank_dropout_rate.py [--out FILE.json] [--md FILE.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEPARATE = {"ULTR_SR_BLOCK": "0", "ULTR_SR_BWD_FUSED": "0"}
CASES = [("a", "rate 0, default plan", 0.0, {}),
         ("b", "rate 0, separate launches (ULTR_SR_BLOCK=0 ULTR_SR_BWD_FUSED=0)", 0.0, SEPARATE),
         ("c", "rate 0.1", 0.1, {})]


def block(case, args, data):
    from ultra_pytorch_amd import engine, hip_ops
    _, _, rate, env = case
    saved_env = {k: os.environ.get(k) for k in SEPARATE}
    for k in SEPARATE:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        shape = hip_ops.SetRankShape(args.features, 256, 8, 2, 64, attention_dtype=args.attention, rate=rate)
        shape.dropout_seed = 1
        eng = engine.SetRankStepEngine(shape, args.batch, args.list_size, torch.device("cuda"), algo="softmax", learning_rate=0.05)
        p0, feats, ids, y, tab = data
        p, st = p0.clone(), torch.zeros_like(p0)
        for _ in range(args.warmup):
            eng.train_step(p, st, feats, feats.shape[0], ids, y, ipw_table=tab)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.train_step(p, st, feats, feats.shape[0], ids, y, ipw_table=tab)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        loss = float(eng.read_loss())
        eng.close()
        del eng
        torch.cuda.empty_cache()
        return dt, loss
    finally:
        for k, v in saved_env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--list-size", type=int, default=100)
    ap.add_argument("--features", type=int, default=220)
    ap.add_argument("--attention", default="fp16")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("setrank_dropout_rate.py measures on the GPU: none found")
    from ultra_pytorch_amd import hip_ops, synthetic
    from ultra_pytorch_amd.ranking_model.SetRank import init_setrank_params
    rng = np.random.RandomState(5)
    feats, ids, y = synthetic.make_batch(rng, args.batch, args.list_size, args.features, n_pad=2)
    shape0 = hip_ops.SetRankShape(args.features, 256, 8, 2, 64)
    dev = torch.device("cuda")
    data = (init_setrank_params(shape0, seed=9).to(dev), torch.from_numpy(np.asarray(feats, np.float32)).to(dev),
            torch.from_numpy(ids).to(dev, torch.int32).contiguous(), torch.from_numpy(y).to(dev, torch.float32).contiguous(),
            torch.from_numpy(np.asarray(synthetic.load_ipw(), np.float32)).to(dev))
    times = {c[0]: [] for c in CASES}
    losses = {}
    for _ in range(args.rounds):
        for case in CASES:
            dt, loss = block(case, args, data)
            times[case[0]].append(dt)
            losses[case[0]] = loss
    results = []
    for key, what, rate, env in CASES:
        t = times[key]
        r = {"case": key, "what": what, "rate": rate, "env": env, "batch": args.batch, "list_size": args.list_size,
             "attention": args.attention, "blocks": len(t), "steps_per_block": args.steps, "median_ms": 1e3 * statistics.median(t),
             "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t), "last_loss": losses[key]}
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        by = {r["case"]: r for r in results}
        with open(args.md, "w") as f:
            f.write("# SetRank training step with dropout, config 5's geometry\n\n")
            f.write("`tools/setrank_dropout_rate.py`: B = %d, L = %d, F = %d, d_model 256, 8 heads, 2 layers, dff 64, %s attention operands, "
                    "one MI355X.  %d blocks per case, interleaved a b c in one process; a block is %d warm-up steps and %d timed steps "
                    "under a host clock that stops behind a device synchronisation.\n\n" % (
                        args.batch, args.list_size, args.features, args.attention, args.rounds, args.warmup, args.steps))
            f.write("| case | median ms/step | min | max |\n|---|---|---|---|\n")
            for r in results:
                f.write("| (%s) %s | %.3f | %.3f | %.3f |\n" % (r["case"], r["what"], r["median_ms"], r["min_ms"], r["max_ms"]))
            f.write("\n(c) is to be read against (b): dropout itself costs %+.3f ms per step (%+.1f %%) on the separate launches it runs on; "
                    "leaving the fused persistent launches, (b) against (a), costs %+.3f ms (%+.1f %%).  No bar is set on either.\n" % (
                        by["c"]["median_ms"] - by["b"]["median_ms"], 100.0 * (by["c"]["median_ms"] / by["b"]["median_ms"] - 1.0),
                        by["b"]["median_ms"] - by["a"]["median_ms"], 100.0 * (by["b"]["median_ms"] / by["a"]["median_ms"] - 1.0)))


if __name__ == "__main__":
    main()
