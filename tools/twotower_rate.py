#!/usr/bin/env python3
"""Time one TwoTower training step next to the RegressionEM step - the nearest existing algorithm: pointwise, aux[L] - in the same
process (figures: profiles/twotower.md).

The model: the flagship DNN, 136 features, hidden [512, 256, 128], at batch 256 x 10 documents and batch 512 x 50, Adagrad.  Per
shape one JSON line:

  twotower_product_ms / twotower_sum_ms / regem_ms   engine.StepEngine.train_step through ultr_train_step: ultr_dnn_forward -> the loss
              kernel (ultr_twotower_loss / ultr_regem_loss) -> ultr_dnn_backward -> ultr_apply_update
  loss_twotower_ms / loss_regem_ms   the loss launch alone (hip_ops.twotower_loss / regem_loss on the scores of one forward)
  each        median / min / max over `--repeats` (>= 30) repetitions after `--warmup` calls; a repetition is `--iters` calls between two
              device synchronisations on a host clock, divided by `--iters`.  The algorithms alternate inside a round, `--rounds` rounds
              give the run-to-run spread.

    python tools/twotower_rate.py [--repeats 30] [--iters 200] [--rounds 3] [--out FILE.json]
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

MODEL = (136, [512, 256, 128])
SHAPES = ((256, 10), (512, 50))


def timed(fn, warmup, repeats, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / iters)
    return {"median": statistics.median(out), "min": min(out), "max": max(out), "repeats": repeats, "iters": iters}


def row(B, L, args):
    from oracle import ultr_oracle as O
    from ultra_pytorch_amd import engine, hip_ops, synthetic
    dev = torch.device("cuda")
    F, hidden = MODEL
    shape = hip_ops.DnnShape(F, hidden, "elu")
    feats, ids, clicks = synthetic.make_batch(np.random.RandomState(L), B, L, F, n_pad=2 if L > 10 else 0)
    f, i, y = torch.tensor(feats, device=dev), torch.tensor(ids, device=dev), torch.tensor(clicks, device=dev)
    n_docs = feats.shape[0]
    p0 = torch.tensor(O.init_params(F, hidden, seed=1), device=dev)
    w = (args.warmup, args.repeats, args.iters)
    out = {"batch": B, "list_size": L, "rows": B * L, "n_params": shape.n_params}
    runs = {}
    for name, algo, kw, aux0 in (("regem", "regem", {}, 0.9), ("twotower_product", "twotower", dict(tower_combination="product"), float(np.log(9.0))),
                                 ("twotower_sum", "twotower", dict(tower_combination="sum"), 0.0)):
        eng = engine.StepEngine(shape, B, L, dev, algo=algo, **kw)
        p = p0.clone()
        st = torch.zeros(max(engine.opt_state_floats(algo, "ada", L, shape.n_params), 1), device=dev)
        aux = torch.full((L,), aux0, device=dev)
        runs[name] = (eng, p, st, aux)
    for name, (eng, p, st, aux) in runs.items():  # alternating: one algorithm after the other inside the round
        out[name + "_ms"] = timed(lambda: eng.train_step(p, st, f, n_docs, i, y, aux=aux), *w)
        assert np.isfinite(eng.read_scalars()[0]), name
    eng, p, st, aux = runs["twotower_product"]
    eng.forward(p, f, n_docs, i, train=True)
    out["loss_twotower_ms"] = timed(lambda: eng.loss(y, aux=aux, docids=i, n_docs=n_docs), *w)
    eng, p, st, aux = runs["regem"]
    eng.forward(p, f, n_docs, i, train=True)
    out["loss_regem_ms"] = timed(lambda: eng.loss(y, aux=aux), *w)
    for eng, _, _, _ in runs.values():
        eng.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if args.repeats < 30:
        raise SystemExit("twotower_rate.py takes the median of at least 30 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("twotower_rate.py measures on the GPU: none found")
    rows = []
    for rnd in range(args.rounds):
        for B, L in SHAPES:
            r = row(B, L, args)
            r["round"] = rnd
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
